// mcs_mb_bands.h -- multi-band band pass (mcs_mb_bdesc_*, mcs_mb_bands*): the band descriptors, the lane
// helpers and the band walker in its three window forms.
#pragma once

#include "mcs_blend.h"

namespace mcs {

// ---- band pass: descriptors once per plan, then per chunk of captures ------------------------
// Band descriptors: grid (bands), block 256.  Per (array row r, lane l) the global-memory window
// descriptor (mb_desc) of the band's owner at mosaic (c0 + l, Y0 - 14 + r), positions reflected
// into the mosaic as mb_prep does (BORDER_DEFAULT: a lane or row past a mosaic edge holds the
// sample of its reflected position).
template <int CN, int INTERP>
__device__ __forceinline__ void mb_bdesc(const KMbBandArgs &a)
{
    const KParams &P = a.P;
    const MbBand B = a.bands[blockIdx.x];
    int cam, w, h;
    slot_info(P, B.slot, cam, w, h);
    const int y0 = B.row * kBlendTileH - kBlendHalo + kMbFirst;
    uint64_t *o = a.bdesc + (int64_t)blockIdx.x * kMbBandDescRows * kMbBandLanes;
    for (int i = threadIdx.x; i < kMbBandDescRows * kMbBandLanes; i += blockDim.x) {
        const int r = i / kMbBandLanes, l = i % kMbBandLanes;
        const int x = refl(B.c0 + l, P.out_w), y = refl(y0 + r, P.out_h);
        const uint2 v = mb_desc<CN>(mb_src<INTERP>(P, B.slot, x, y), w, h);
        o[i] = (uint64_t)v.x | ((uint64_t)v.y << 32);
    }
}

// Value of lane l + 1 / l - 1 of the wave (DPP wave_shl:1 / wave_shr:1; the end lanes get 0).
// (bound_ctrl: a lane without a source reads 0 -- the edge lanes' value -- so no `old` register
// has to be zeroed before every DPP move)
__device__ __forceinline__ uint32_t lane_next(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x130, 0xf, 0xf, true);
}
__device__ __forceinline__ uint32_t lane_prev(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x138, 0xf, 0xf, true);
}
// Value of lane `src` (byte address src * 4: ds_bpermute).
__device__ __forceinline__ int lane_at(int v, int src4)
{
    return __builtin_amdgcn_ds_bpermute(src4, v);
}

// CN consecutive ints (one wide store: 4-byte aligned).
template <int CN>
__device__ __forceinline__ void mb_store_ch(__attribute__((address_space(1))) uint8_t *p,
                                            const int (&v)[CN])
{
    typedef __attribute__((address_space(1))) int gi;
    typedef int i3 __attribute__((ext_vector_type(3), aligned(4)));
    typedef int i4 __attribute__((ext_vector_type(4), aligned(4)));
    if (CN == 3) {
        i3 t;
        t.x = v[0], t.y = v[CN > 1 ? 1 : 0], t.z = v[CN > 2 ? 2 : 0];
        *(__attribute__((address_space(1))) i3 *)p = t;
    } else if (CN == 4) {
        i4 t;
        t.x = v[0], t.y = v[CN > 1 ? 1 : 0], t.z = v[CN > 2 ? 2 : 0], t.w = v[CN > 3 ? 3 : 0];
        *(__attribute__((address_space(1))) i4 *)p = t;
    } else {
#pragma unroll
        for (int k = 0; k < CN; k++) ((gi *)p)[k] = v[k];
    }
}

// Scratch targets of one emitted entry: up to two listed tiles of the band's row whose arrays
// hold the column (base = (list index * slots + local slot) * chunk, col = column in the tile's
// array); base -1 = none.
struct MbTarget {
    int base[2], col[2];
};
static_assert(kBlendTileW == 32, "mb_bands: tile columns are found by shifts");

__device__ __forceinline__ void mb_target(const KMbBandArgs &a, int s, int row, int tx, int col,
                                          MbTarget &T, int k)
{
    T.base[k] = -1;
    T.col[k] = 0;
    if (tx < 0 || tx >= a.gxb) return;
    const int bt = a.tile_bt[row * a.gxb + tx];
    if (bt < 0) return;
    const uint32_t mask = (uint32_t)a.list[2 + 2 * bt];
    if (!((mask >> s) & 1u)) return;
    const int j = __popc(mask & ((1u << s) - 1u));
    T.base[k] = (bt * a.slots + j) * a.chunk;
    T.col[k] = col;
}

// One band, FR captures: grid (bands, ceil(nf / FR)), block 64 (one wave).  Per level-0 row: the
// lane's replicate-border sample (the owner's frame through L1/L2; descriptors three rows ahead,
// windows two rows ahead), unpacked to 16-bit lanes and accumulated into the vertical 5-tap sums
// of the level-1 rows it feeds (three rolling accumulators).  Per finished level-1 row: the
// horizontal 5-tap over the neighbour lanes (DPP), giving level 1 at the even lanes; its
// R1-region entries go to the scratch, and the row is accumulated per channel into the vertical
// sums of level 2.  Per finished level-2 row: the horizontal 5-tap over lanes 2 and 4 apart
// (ds_bpermute), level 2 at every fourth lane.  Only entries at real mosaic positions are stored
// (the blend reads no others).  Integer sums, exact: the values of mb_levels' LDS passes.
// Rows and columns of a unit past the top / left mosaic edge hold reflected level-0 samples, and
// the reduces computed there are the reflected entries (reflect-101 about 0 commutes with the
// 2x decimation).  At the bottom / right edges it does not (for even level sizes), so BR units
// give level 2 the reflected level-1 rows (a history of four) and columns (source lanes).

// CN consecutive ints by one buffer store (offset past the range: nothing written).
template <int CN>
__device__ __forceinline__ void mb_buffer_store_ch(__amdgpu_buffer_rsrc_t rs, uint32_t off,
                                                   const int (&v)[CN])
{
    typedef unsigned int u2v __attribute__((ext_vector_type(2)));
    typedef unsigned int u3v __attribute__((ext_vector_type(3)));
    typedef unsigned int u4v __attribute__((ext_vector_type(4)));
    if constexpr (CN == 1) {
        __builtin_amdgcn_raw_buffer_store_b32((uint32_t)v[0], rs, off, 0, 0);
    } else if constexpr (CN == 2) {
        const u2v t = {(uint32_t)v[0], (uint32_t)v[CN > 1 ? 1 : 0]};
        __builtin_amdgcn_raw_buffer_store_b64(t, rs, off, 0, 0);
    } else if constexpr (CN == 3) {
        const u3v t = {(uint32_t)v[0], (uint32_t)v[CN > 1 ? 1 : 0], (uint32_t)v[CN > 2 ? 2 : 0]};
        __builtin_amdgcn_raw_buffer_store_b96(t, rs, off, 0, 0);
    } else {
        const u4v t = {(uint32_t)v[0], (uint32_t)v[CN > 1 ? 1 : 0], (uint32_t)v[CN > 2 ? 2 : 0],
                       (uint32_t)v[CN > 3 ? 3 : 0]};
        __builtin_amdgcn_raw_buffer_store_b128(t, rs, off, 0, 0);
    }
}

// LDS band pass: vector memory operations issued at body row ph (after its LDS reads): the
// stores of the entries finished by the previous row (2 targets per capture: level 1 after odd
// rows, level 2 after rows 4j + 1), the group DMAs (rows 4j, one per capture), the descriptor DMA.
template <int FR>
constexpr int mb_lds_ops(int ph)
{
    return ((ph & 1) ? 2 * FR : 0) + (ph % 4 == 1 ? 2 * FR : 0) + (ph % 4 == 0 ? FR : 0) + 1;
}
// The vmcnt bound before row ph's LDS reads: no more operations outstanding than were issued after
// the latest one that row needs -- its descriptor (issued NL rows earlier, last in that row) and
// its source groups (issued >= kMbLdsGLead rows earlier, before that row's descriptor).  First
// body pass, ph < NL: the descriptor came in the prologue, followed by the prologue's later
// descriptors and this pass's rows (the groups those rows may read are all prologue groups).
template <int FR, int NL>
constexpr int mb_lds_wait(int ph, bool first)
{
    int d = 0, g = 1;
    for (int j = 1; j < NL; j++) d += mb_lds_ops<FR>((ph - j + 12) % 12);
    for (int j = 1; j < kMbLdsGLead; j++) g += mb_lds_ops<FR>((ph - j + 12) % 12);
    int w = d < g ? d : g;
    if (first) {
        int w0 = NL - 1 - ph;
        for (int j = 0; j < ph; j++) w0 += mb_lds_ops<FR>(j);
        w = w0 < w ? w0 : w;
    }
    return w > 63 ? 63 : w;
}

// Window modes (WM): 0 = unaligned 8-byte global loads; 1 (AL) = dword-aligned 12-byte global
// loads (mb_desc's sh), funnel-shifted in registers (the texture addresser splits unaligned
// loads: serial band pass 270 -> ~220 us, tools/experiments/gpu_r03_bandalign.sh); 2 = the
// band's source rows staged in an LDS ring by LDS-DMA, 4 rows per wave instruction (KMbBandArgs
// bgrp), the windows read from LDS (descriptor .x = the two windows' ring offsets): one 16-byte
// chunk per lane instead of four 12-byte gathers per lane and row.  Mode 2 needs a band whose
// source rows advance with its rows (mcs_prepare.cpp band_lds_tables checks the ring schedule);
// the other bands of an aligned launch take mode 1.  In mode 2 the descriptors come by LDS-DMA
// too (16 B per lane and row: windows, meta, the offset of the group issued after that row), so
// the loop holds no ordinary global load: the compiler's own vmcnt waits for ordinary loads
// would otherwise drain the LDS-DMAs every row.
template <int CN, int FR, bool BR, int WM, bool GAIN = false>
__device__ __forceinline__ void mb_bands_body(const KMbBandArgs &a, int bi, lds_u8 *ring, int pr)
{
    constexpr bool AL = WM >= 1, LD = WM == 2;
    typedef __attribute__((address_space(1))) const uint8_t gu8;
    struct __attribute__((packed)) U2 {
        uint32_t x, y;
    };
    struct U3 {
        uint32_t x, y, z;
    };
    typedef __attribute__((address_space(1))) const U2 gu2;
    typedef __attribute__((address_space(1))) const U3 gu3;
    typedef std::conditional_t<AL, uint3, uint2> Win;
    typedef __attribute__((address_space(1))) uint2 g2u;
    const KParams &P = a.P;
    const int l = threadIdx.x;
    const MbBand B = a.bands[bi];
    const int fl0 = pr * FR;
    if (fl0 >= a.nf) return;
    int cam, w, h;
    slot_info(P, B.slot, cam, w, h);
    // (GAIN: the band's owner camera is uniform over the wave: its q halves live in SGPRs; the
    // gain is VALU between the window reads and the udot2 -- no memory operation, so the counted
    // waits of the LDS-ring form hold as they are)
    const GainQ gq = GAIN ? gain_pair(gain_q_of(P, cam)) : GainQ();
    const uint32_t pitch = (uint32_t)(w * CN);
    const gu8 *fb[FR];
#pragma unroll
    for (int i = 0; i < FR; i++)
        fb[i] = (const gu8 *)(P.cams[cam] +
                              (int64_t)(a.f0 + min(fl0 + i, a.nf - 1)) * P.cam_fstride[cam]);
    const int W = P.out_w, H = P.out_h;
    const int w1 = (W + 1) / 2, h1 = (H + 1) / 2, w2 = (w1 + 1) / 2, h2 = (h1 + 1) / 2;
    const int Y0 = B.row * kBlendTileH, Y1 = Y0 / 2 - kMbO1, Y2 = Y0 / 4 - kMbO2;
    const int x = B.c0 + l;
    // level-1 column x / 2 on even lanes 2..60, level-2 column x / 4 on lanes 8, 12, .., 56
    // (complete there), stored when inside the mosaic
    MbTarget T1, T2;
    T1.base[0] = T1.base[1] = T2.base[0] = T2.base[1] = -1;
    T1.col[0] = T1.col[1] = T2.col[0] = T2.col[1] = 0;
    if ((l & 1) == 0 && l >= 2 && l <= 61 && x >= 0 && (x >> 1) < w1) {
        // R1 region of tile tx: columns [16 tx - 1, 16 tx + 16]
        const int qx = x >> 1, tx = (qx + kMbOR) >> 4;
        mb_target(a, B.slot, B.row, tx, qx - (tx * (kBlendTileW / 2) - kMbOR), T1, 0);
        if (((qx + kMbOR) & 15) < kMbNRX - 16)
            mb_target(a, B.slot, B.row, tx - 1, qx - ((tx - 1) * (kBlendTileW / 2) - kMbOR), T1, 1);
    }
    if ((l & 3) == 0 && l >= 8 && l <= 56 && x >= 0 && (x >> 2) < w2) {
        // level-2 array of tile tx: columns [8 tx - 2, 8 tx + 9]
        const int z = x >> 2, tx = (z + kMbO2) >> 3;
        mb_target(a, B.slot, B.row, tx, z - (tx * (kBlendTileW / 4) - kMbO2), T2, 0);
        if (((z + kMbO2) & 7) < kMbN2X - 8)
            mb_target(a, B.slot, B.row, tx - 1, z - ((tx - 1) * (kBlendTileW / 4) - kMbO2), T2, 1);
    }
    // level-2 horizontal sources: level-1 columns qx - 2 .. qx + 2 (lanes 2 apart), reflected
    // at the right mosaic edge (BR)
    int src[4];
#pragma unroll
    for (int t = 0; t < 4; t++) {
        int q = (x >> 1) + (t < 2 ? t - 2 : t - 1);
        if (BR && q >= w1) q = 2 * w1 - 2 - q;
        src[t] = min(max(2 * q - B.c0, 0), kMbBandLanes - 1) * 4;
    }
    // scratch byte offsets (32-bit: the scratch is < 4 GiB) of this lane's targets, capture fl0,
    // array row 0
    uint32_t o1[2], o2[2];
#pragma unroll
    for (int k = 0; k < 2; k++) {
        o1[k] = T1.base[k] < 0 ? 0u : (uint32_t)((T1.base[k] + fl0) * (kMbNRX * kMbNRY) +
                                                 mb_g1_at(T1.col[k], 0)) * 8u;
        o2[k] = T2.base[k] < 0 ? 0u : (uint32_t)((T2.base[k] + fl0) * (kMbN2X * kMbN2Y * CN) +
                                                 mb_g2_at<CN>(T2.col[k], 0, 0)) * 4u;
    }
    typedef __attribute__((address_space(1))) uint8_t g8;
    g8 *const g1b = (g8 *)a.g1, *const g2b = (g8 *)a.g2;
    const uint64_t *dsc = a.bdesc + (int64_t)bi * kMbBandDescRows * kMbBandLanes + l;
    const int nst = min(FR, a.nf - fl0);
    // Rolling vertical sums, indexed by row % 3 (compile-time inside the 12-row body): level-1
    // rows (packed u16: lo = channels 0, 2; hi = 1, 3), level-2 rows (one int per channel).  A
    // row's sum starts with '=' at its first input row, so the rows before the array (and the
    // padding rows after it) only ever feed rows that are not stored.
    uint32_t Vl[FR][3], Vh[FR][3];
    int V2[FR][3][CN];
    uint32_t hl[FR][BR ? 4 : 1], hh[FR][BR ? 4 : 1];   // BR: the last four level-1 rows
#pragma unroll
    for (int i = 0; i < FR; i++)
#pragma unroll
        for (int q = 0; q < 3; q++) {
            Vl[i][q] = Vh[i][q] = 0u;
#pragma unroll
            for (int k = 0; k < CN; k++) V2[i][q][k] = 0;
            if (q < (BR ? 4 : 1)) hl[i][q] = hh[i][q] = 0u;
        }
    if (BR) {
#pragma unroll
        for (int i = 0; i < FR; i++) hl[i][BR ? 3 : 0] = hh[i][BR ? 3 : 0] = 0u;
    }
    auto load_win = [&](uint64_t dv, Win (&r0)[FR], Win (&r1)[FR]) {
        if constexpr (LD) return;
        const uint32_t dx = (uint32_t)dv;
        const uint32_t d = AL ? (uint32_t)(dv >> 47) & 15u : (uint32_t)(dv >> 44) & 7u;
        uint32_t o = (dx & 0x7fffffffu) - d, ob = o + ((dx >> 31) ? pitch : 0u);
#pragma unroll
        for (int i = 0; i < FR; i++) {
            if constexpr (AL) {
                const U3 ra = *(const gu3 *)(fb[i] + o), rb = *(const gu3 *)(fb[i] + ob);
                r0[i] = make_uint3(ra.x, ra.y, ra.z);
                r1[i] = make_uint3(rb.x, rb.y, rb.z);
            } else {
                const U2 ra = *(const gu2 *)(fb[i] + o), rb = *(const gu2 *)(fb[i] + ob);
                r0[i] = make_uint2(ra.x, ra.y);
                r1[i] = make_uint2(rb.x, rb.y);
            }
        }
    };
    // Finished entries wait one row in registers before they are stored: gfx9 counts stores
    // in vmcnt, so the wait for a row's window loads also waits for every store issued after
    // those loads -- a store issued early in the next row has that row's work to complete.
    int pend1 = -1, pend2 = -1;   // array row of the pending level-1 / level-2 entries (-1: none)
    uint32_t p1l[FR], p1h[FR];
    int p2[FR][CN];
    // LDS mode: the entries of every level-1 / level-2 row are stored, at fixed rows of the body
    // (level 1 after odd rows, level 2 after rows 4j + 1), as buffer stores whose lanes without a
    // target (or rows outside the arrays: ok1 / ok2 false) carry an out-of-range offset and write
    // nothing -- so every row issues a fixed number of vector memory operations and the waits
    // before its LDS reads can count them (mb_lds_wait)
    bool ok1 = false, ok2 = false;
    const __amdgpu_buffer_rsrc_t rs1 = __builtin_amdgcn_make_buffer_rsrc((void *)a.g1, 0, 0x7fffffff, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs2 = __builtin_amdgcn_make_buffer_rsrc((void *)a.g2, 0, 0x7fffffff, 0x00020000);
    auto flush_ld = [&](auto PHc) {
        constexpr int ph = decltype(PHc)::value;
        constexpr uint32_t none = 0xfffffff0u;
        if constexpr (ph & 1) {
#pragma unroll
            for (int f = 0; f < FR; f++) {
                const uint32_t ro =
                    (uint32_t)(f * (kMbNRX * kMbNRY) + mb_g1_at(0, pend1 - kMbRS)) * 8u;
                typedef unsigned int u2v __attribute__((ext_vector_type(2)));
                const u2v v = {p1l[f], p1h[f]};
#pragma unroll
                for (int k = 0; k < 2; k++)
                    __builtin_amdgcn_raw_buffer_store_b64(
                        v, rs1, (ok1 && f < nst && T1.base[k] >= 0) ? o1[k] + ro : none, 0, 0);
            }
        }
        if constexpr (ph % 4 == 1) {
#pragma unroll
            for (int f = 0; f < FR; f++) {
                const uint32_t ro =
                    (uint32_t)(f * (kMbN2X * kMbN2Y * CN) + mb_g2_at<CN>(0, pend2, 0)) * 4u;
#pragma unroll
                for (int q = 0; q < 2; q++) {
                    const uint32_t off = (ok2 && f < nst && T2.base[q] >= 0) ? o2[q] + ro : none;
                    mb_buffer_store_ch<CN>(rs2, off, p2[f]);
                }
            }
        }
    };
    auto flush = [&]() {
        if (pend1 >= 0) {
#pragma unroll
            for (int f = 0; f < FR; f++) {
                if (f >= nst) break;
                const uint32_t ro =
                    (uint32_t)(f * (kMbNRX * kMbNRY) + mb_g1_at(0, pend1 - kMbRS)) * 8u;
#pragma unroll
                for (int k = 0; k < 2; k++)
                    if (T1.base[k] >= 0) *(g2u *)(g1b + (o1[k] + ro)) = make_uint2(p1l[f], p1h[f]);
            }
            pend1 = -1;
        }
        if (pend2 >= 0) {
#pragma unroll
            for (int f = 0; f < FR; f++) {
                if (f >= nst) break;
                const uint32_t ro =
                    (uint32_t)(f * (kMbN2X * kMbN2Y * CN) + mb_g2_at<CN>(0, pend2, 0)) * 4u;
#pragma unroll
                for (int q = 0; q < 2; q++)
                    if (T2.base[q] >= 0) mb_store_ch<CN>(g2b + (o2[q] + ro), p2[f]);
            }
            pend2 = -1;
        }
    };
    // finished level-1 vertical sums (vl, vh) of array row i = 2m + P2 (m % 3 = M3), capture f
    auto level1_done = [&](int i, auto P2c, auto M3c, int f, uint32_t vl, uint32_t vh) {
        constexpr int P2 = decltype(P2c)::value, M3 = decltype(M3c)::value;
        // horizontal: level-1 entry at lane x = 2 qx reads lanes x - 2 .. x + 2
        const uint32_t l1 = lane_prev(vl), l2 = lane_prev(l1), r1 = lane_next(vl),
                       r2 = lane_next(r1);
        const uint32_t h1_ = lane_prev(vh), h2_ = lane_prev(h1_), s1 = lane_next(vh),
                       s2 = lane_next(s1);
        uint32_t gl = mad6_u32(vl, (l2 + r2) + 4u * (l1 + r1));
        uint32_t gh = mad6_u32(vh, (h2_ + s2) + 4u * (h1_ + s1));
        const int qy = Y1 + i;
        if constexpr (LD) {
            pend1 = i;
            ok1 = qy >= 0 && qy < h1 && i >= kMbRS && i < kMbRS + kMbNRY;
            p1l[f] = gl;
            p1h[f] = gh;
        } else if (qy >= 0 && qy < h1 && i >= kMbRS && i < kMbRS + kMbNRY) {
            pend1 = i;   // (stored at the next row, see flush)
            p1l[f] = gl;
            p1h[f] = gh;
        }
        if (BR) {
            // rows past the bottom edge feed level 2 as their reflections: h1 -> h1 - 2 (two
            // rows back), h1 + 1 -> h1 - 3 (four back); deeper rows feed no stored entry
            if (qy >= h1) {
                const bool d0 = qy == h1;
                gl = d0 ? hl[f][1] : hl[f][BR ? 3 : 0];
                gh = d0 ? hh[f][1] : hh[f][BR ? 3 : 0];
            }
#pragma unroll
            for (int q = (BR ? 3 : 0); q > 0; q--) hl[f][q] = hl[f][q - 1], hh[f][q] = hh[f][q - 1];
            hl[f][0] = gl, hh[f][0] = gh;
        }
        int g[CN];
#pragma unroll
        for (int k = 0; k < CN; k++)
            g[k] = (int)((((k & 1) ? gh : gl) >> ((k & 2) ? 16 : 0)) & 0xffffu);
        // vertical: level-2 array row e reads level-1 rows 2e .. 2e + 4
        if (P2 == 0) {
#pragma unroll
            for (int k = 0; k < CN; k++) V2[f][(M3 + 1) % 3][k] += g[k];   // row m - 2 done
            const int e = (i >> 1) - 2, zy = Y2 + e;
            if (LD) {
                pend2 = e;
                ok2 = e >= 0 && e < kMbN2Y && zy < h2;
            }
            if (LD || (e >= 0 && e < kMbN2Y && zy < h2)) {
                pend2 = e;
#pragma unroll
                for (int k = 0; k < CN; k++) {
                    const int v = V2[f][(M3 + 1) % 3][k];
                    p2[f][k] = (lane_at(v, src[0]) + lane_at(v, src[3])) +
                               4 * (lane_at(v, src[1]) + lane_at(v, src[2])) + 6 * v;
                }
            }
#pragma unroll
            for (int k = 0; k < CN; k++) {
                V2[f][(M3 + 2) % 3][k] += 6 * g[k];
                V2[f][M3][k] = g[k];
            }
        } else {
#pragma unroll
            for (int k = 0; k < CN; k++) {
                V2[f][(M3 + 2) % 3][k] += 4 * g[k];
                V2[f][M3][k] += 4 * g[k];
            }
        }
    };
    // Pipeline over rows: at row r the windows of rows r + 1 .. r + A and the descriptor of row
    // r + A + 1 are in flight (A = kMbBandAhead), A + 1 buffers each indexed by row % (A + 1).
    // The 12-row body makes every buffer and accumulator index a compile-time constant, so no
    // register copy ever reads an in-flight load (such a copy makes the compiler drain all loads
    // at the loop's back edge).
    constexpr int NB = kMbBandBufs, A = kMbBandAhead, ND = kMbBandDescRing;
    uint64_t dq[ND];
    Win wq0[NB][FR], wq1[NB][FR];
    // LDS mode: group g = the band's source rows 4g .. 4g + 3 (from its first) into ring rows
    // (4g .. 4g + 3) mod kMbLdsRows of every capture's ring, one LDS-DMA instruction per capture
    // (lane = 16-byte chunk, byte offsets in the frame from bgrp); groups 0 .. kMbLdsLead / 4 before
    // the loop, group r / 4 + kMbLdsLead / 4 + 1 after row r (r % 4 == 0); descriptor row r + NL
    // after row r.  No ordinary global load in the loop: `s_waitcnt vmcnt(mb_lds_wait)` before a
    // row's LDS reads counts the fixed operations issued after everything that row reads.
    const uint32_t *grp = a.bgrp + (int64_t)bi * kMbLdsGroups * kMbBandLanes + l;
    typedef __attribute__((address_space(3))) const uint32_t lu32;
    lds_u8 *const dring = ring + kMbLdsDescOff;
    constexpr int NL = kMbLdsDescRing;
    const uint4 *d16 = a.bdesc16 + (int64_t)bi * kMbLdsDescRows * kMbBandLanes + l;
    auto issue_desc = [&](int row) {   // descriptor row `row` into ring slot row % NL
        __builtin_amdgcn_global_load_lds(d16 + row * kMbBandLanes,
                                         dring + (row % NL) * kMbBandLanes * 16, 16, 0, 0);
        asm volatile("" ::: "memory");
    };
    // (one buffer resource per capture frame: the chunks a row's samples do not read carry an
    // out-of-range offset and fetch nothing, while the instruction count stays fixed)
    __amdgpu_buffer_rsrc_t rsf[FR];
#pragma unroll
    for (int f = 0; f < FR; f++)
        rsf[f] = __builtin_amdgcn_make_buffer_rsrc((void *)fb[f], 0, (int)(pitch * (uint32_t)h),
                                                   0x00020000);
    auto issue_group = [&](int g, uint32_t off) {
#pragma unroll
        for (int f = 0; f < FR; f++)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(
                rsf[f], ring + f * kMbLdsRingBytes + ((4 * g) % kMbLdsRows) * kMbLdsSpan, 16, off, 0,
                0, 0);
        asm volatile("" ::: "memory");   // (the next row's descriptor load stays after the DMAs)
    };
    if constexpr (LD) {
        uint32_t go[kMbLdsLead / 4 + 1];
#pragma unroll
        for (int g = 0; g <= kMbLdsLead / 4; g++) go[g] = grp[g * kMbBandLanes];
#pragma unroll
        for (int g = 0; g <= kMbLdsLead / 4; g++) issue_group(g, go[g]);
#pragma unroll
        for (int i = 0; i < NL; i++) issue_desc(i);
    } else {
#pragma unroll
        for (int i = 0; i < ND; i++) dq[i] = dsc[i * kMbBandLanes];
    }
#pragma unroll
    for (int i = 0; i < A; i++) load_win(dq[i], wq0[i], wq1[i]);
    for (int r12 = 0; r12 < kMbBandRows; r12 += 12) {
        static_for<12>([&](auto PHc) {
            constexpr int ph = decltype(PHc)::value;
            const int r = r12 + ph;
            constexpr int b0 = ph % NB, bA = (ph + A) % NB, d0 = ph % ND, dA = (ph + A) % ND;
            uint32_t wa, wb, meta, dxr;
            if constexpr (LD) {
                if (ph < NL && r12 == 0)
                    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(mb_lds_wait<FR, NL>(ph, true)) : "memory");
                else
                    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(mb_lds_wait<FR, NL>(ph, false)) : "memory");
                // (ring descriptor: windows + shift, and the doubled weights precomputed on the
                // host, band_lds_tables)
                const lu32 *dd = (const lu32 *)(dring + (ph % NL) * kMbBandLanes * 16 + l * 16);
                dxr = dd[0];
                wa = dd[1];
                wb = dd[3];
                meta = 0u;
            } else {
                dxr = (uint32_t)dq[d0];
                meta = (uint32_t)(dq[d0] >> 32);
                mb_weights2(meta, wa, wb);
            }
            const uint32_t dd = AL ? 0u : (meta >> 12) & 7u;
            // per capture the sample's channels as packed u16 pairs: pl = (ch 0, ch 2), ph = (ch
            // 1, ch 3), each channel from byte 2 of its mb_tap2 sum
            uint32_t pls[FR], phs[FR];
#pragma unroll
            for (int f = 0; f < FR; f++) {
                uint2 r0, r1;
                if constexpr (LD) {
                    const uint32_t dx = dxr, sh = (dx >> 14) & 3u;
                    const lu32 *pa = (const lu32 *)(ring + f * kMbLdsRingBytes + (dx & 0x3fffu));
                    const lu32 *pb = (const lu32 *)(ring + f * kMbLdsRingBytes + (dx >> 16));
                    r0 = mb_win_shift4(make_uint3(pa[0], pa[1], pa[2]), sh);
                    r1 = mb_win_shift4(make_uint3(pb[0], pb[1], pb[2]), sh);
                } else if constexpr (AL) {
                    const uint32_t sh = (meta >> 15) & 15u;
                    r0 = mb_win_shift<CN>(wq0[b0][f], sh);
                    r1 = mb_win_shift<CN>(wq1[b0][f], sh);
                } else {
                    r0 = wq0[b0][f];
                    r1 = wq1[b0][f];
                }
                uint32_t t[4];
#pragma unroll
                for (int c = 0; c < 4; c++) t[c] = c < CN ? mb_tap2<CN, GAIN>(r0, r1, wa, wb, c, dd, gq) : 0u;
                if constexpr (CN >= 3) pls[f] = __builtin_amdgcn_perm(t[2], t[0], 0x0c060c02u);
                else pls[f] = (t[0] >> 16) & 0xffu;
                if constexpr (CN >= 4) phs[f] = __builtin_amdgcn_perm(t[3], t[1], 0x0c060c02u);
                else if constexpr (CN == 2 || CN == 3) phs[f] = (t[1] >> 16) & 0xffu;
                else phs[f] = 0u;
            }
            // the previous row's finished entries (after this row's window wait), then the loads:
            // windows of row r + A (its descriptor arrived a row ago), descriptor of row r + A + 1
            if constexpr (LD) flush_ld(PHc);
            else flush();
            load_win(dq[dA], wq0[bA], wq1[bA]);
            if constexpr (LD) {
                // this row's descriptor slot is refilled below (issue_desc(r + NL)): its LDS reads
                // must have completed -- in the schedule and in hardware -- before that DMA is
                // issued (without this the compiler sank the weight reads past it: a race)
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                if constexpr (ph % 4 == 0) {
                    const lu32 *dd = (const lu32 *)(dring + (ph % NL) * kMbBandLanes * 16 + l * 16);
                    issue_group(r / 4 + kMbLdsLead / 4 + 1, dd[2]);
                }
                issue_desc(r + NL);
            } else {
                dq[d0] = dsc[(r + ND) * kMbBandLanes];
            }
            // level-0 row r = 2k + (ph & 1), k % 3 = K3; level-1 row k - 2 = 2m + P2, m % 3 = M3
            constexpr int K3 = (ph / 2) % 3;
            constexpr int q = ph / 2 - 2, P2 = q & 1, M3 = ((q - P2) / 2 + 3) % 3;
            const int k = r >> 1;
#pragma unroll
            for (int f = 0; f < FR; f++) {
                const uint32_t pl = pls[f], ph_ = phs[f];
                // vertical: level-1 array row i reads level-0 rows 2i .. 2i + 4
                if ((ph & 1) == 0) {
                    Vl[f][(K3 + 1) % 3] += pl;   // row k - 2 done
                    Vh[f][(K3 + 1) % 3] += ph_;
                    level1_done(k - 2, std::integral_constant<int, P2>(),
                                std::integral_constant<int, M3>(), f, Vl[f][(K3 + 1) % 3],
                                Vh[f][(K3 + 1) % 3]);
                    // (pl, ph_ <= 0x00ff00ff < 2^24: a full-rate 24-bit multiply)
                    Vl[f][(K3 + 2) % 3] += __umul24(pl, 6u);
                    Vh[f][(K3 + 2) % 3] += __umul24(ph_, 6u);
                    Vl[f][K3] = pl;
                    Vh[f][K3] = ph_;
                } else {
                    Vl[f][(K3 + 2) % 3] += 4u * pl;
                    Vh[f][(K3 + 2) % 3] += 4u * ph_;
                    Vl[f][K3] += 4u * pl;
                    Vh[f][K3] += 4u * ph_;
                }
            }
        });
    }
    if constexpr (!LD) flush();   // (LD: the last row stored everything pending)
}

// The band pass of band bi: the aligned launch (AL) runs bands flagged for the LDS ring (MbBand
// pad_ bit 0, band_lds_tables) in mode 2, the others in mode 1.
template <int CN, int FR, bool BR, bool AL, bool GAIN = false>
__device__ __forceinline__ void mb_bands(const KMbBandArgs &a, int bi, lds_u8 *ring, int pr)
{
    if constexpr (AL) {
        const int lds = __builtin_amdgcn_readfirstlane(a.bands[bi].pad_) & 1;
        if (lds) mb_bands_body<CN, FR, BR, 2, GAIN>(a, bi, ring, pr);
        else mb_bands_body<CN, FR, BR, 1, GAIN>(a, bi, ring, pr);
    } else {
        mb_bands_body<CN, FR, BR, 0, GAIN>(a, bi, ring, pr);
    }
}

}  // namespace mcs
