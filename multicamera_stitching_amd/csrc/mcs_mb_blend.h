// mcs_mb_blend.h -- multi-band blend kernel (mcs_mb_blend_*) and its work records.
#pragma once

#include "mcs_blend.h"

namespace mcs {

// ---- blend: grid (listed tiles, nf), block kMbBlThreads ------------------------------------------
template <int CN, int S>
struct MbBlLds {
    uint2 g1[S][kMbNRX * kMbNRY];      // packed as in mb_levels
    int32_t g2[S][CN][kMbN2X * kMbN2Y];   // channel-planar: indices need no * CN
    double b2[CN][kMbN2X * kMbN2Y];
    double r1[CN][kMbNRX * kMbNRY];
};

constexpr int kMbPQ = kMbTilePx / kMbBlThreads;   // tile pixels per thread
static_assert(kMbN2X * kMbN2Y <= kMbBlThreads, "mb_blend: one level-2 entry per thread");

// What a blend thread holds from the block's one round of loads: its work records (mcs_kparams.h;
// iterations past a list's end hold inert records), its pixels' owner samples, and the B2
// operands of level-2 entry `tid`.
template <int CN, int S>
struct MbWork {
    uint2 px[kMbPQ];                              // pixel records
    uint32_t v[kMbPQ];       // their owner samples (the stitch kernel's output), channel k in byte k
    uint32_t r1[kMbR1Iters][mb_r1rec_words(S)];   // R1 records
    int32_t m2[S], d2;                            // m2[j][tid], d2[tid]
};

// Expand weights of a parity class along one axis (exp_taps): odd -> 4 4 (0), even -> 1 6 1.
__device__ __forceinline__ void mb_cls_wt(bool odd, int *wt)
{
    wt[0] = odd ? 4 : 1, wt[1] = odd ? 4 : 6, wt[2] = odd ? 0 : 1;
}

// m1 of owner slot j from an R1 record's packed words (16 bits a slot): a shift by j, never a
// register array indexed by j.
template <int S>
__device__ __forceinline__ uint32_t mb_rec_m1(const uint32_t *w, int j)
{
    if constexpr (S == 2) {
        return (w[2] >> (j * 16)) & 0xffffu;
    } else if constexpr (S == 4) {
        return (uint32_t)(((uint64_t)w[2] | ((uint64_t)w[3] << 32)) >> (j * 16)) & 0xffffu;
    } else {
        const uint64_t lo = (uint64_t)w[2] | ((uint64_t)w[3] << 32);
        const uint64_t hi = (uint64_t)w[4] | ((uint64_t)w[5] << 32);
        return (uint32_t)((j < 4 ? lo : hi) >> ((j & 3) * 16)) & 0xffffu;
    }
}

template <int CN, int S>
__device__ __forceinline__ void mb_blend_tile(const KMbArgs &a, const MbGeo &G, MbBlLds<CN, S> &L,
                                              const MbWork<CN, S> &wk, int ns, int n_r1, int f)
{
    const KParams &P = a.P;
    const int tid = threadIdx.x;
    // B2 = sum m2 g2 / (sum m2 * 65536)
    if (tid < kMbN2X * kMbN2Y) {
        const int e = tid;
        // (integer sums in double: every product < 2^41, every sum < 2^43 -- exact)
        double num[CN];
#pragma unroll
        for (int k = 0; k < CN; k++) num[k] = 0.0;
#pragma unroll
        for (int j = 0; j < S; j++) {
            if (j >= ns) break;
            const double m = (double)wk.m2[j];
#pragma unroll
            for (int k = 0; k < CN; k++) num[k] += m * (double)L.g2[j][k][e];
        }
        const int den = wk.d2;
#pragma unroll
        for (int k = 0; k < CN; k++)
            L.b2[k][e] = den ? num[k] / ((double)den * 65536.0) : 0.0;
    }
    __syncthreads();
    // R1 = B1 + up(B2), B1 = sum m1 (16384 g1 - E(g2)) / (sum m1 * 4194304)
    // (the list is grouped by parity class, mb_prep: the zero-weight third taps of odd
    // coordinates are skipped by whole waves)
#pragma unroll
    for (int it = 0; it < kMbR1Iters; it++) {
        if (it * kMbBlThreads >= n_r1) break;   // (uniform)
        const uint32_t *rw = wk.r1[it];
        const int e = (int)(rw[0] & 1023u);
        if (e == kMbR1Inert) continue;
        const int p1 = (int)((rw[0] >> 10) & 1023u), cls = (int)((rw[0] >> 20) & 3u);
        int wy[3], wx[3];
        mb_cls_wt((cls & 2) != 0, wy);
        mb_cls_wt((cls & 1) != 0, wx);
        const bool y3 = (cls & 2) == 0, x3 = (cls & 1) == 0;
        int tp[9], tw[9];
#pragma unroll
        for (int u = 0; u < 3; u++)
#pragma unroll
            for (int v = 0; v < 3; v++) {
                // (24-bit multiply: full-rate v_mul_u32_u24 instead of quarter-rate v_mul_lo_u32)
                tp[3 * u + v] = (int)__umul24((rw[1] >> (5 * u)) & 31u, kMbN2X) +
                                (int)((rw[1] >> (15 + 4 * v)) & 15u);
                tw[3 * u + v] = wy[u] * wx[v];
            }
        // (integer sums in double: every product < 2^39, every sum < 2^41 -- exact)
        double num[CN];
#pragma unroll
        for (int k = 0; k < CN; k++) num[k] = 0.0;
        for (int j = 0; j < ns; j++) {
            int e2[CN];   // <= 64 * 65536 * 255 < 2^31: exact in int32
#pragma unroll
            for (int k = 0; k < CN; k++) e2[k] = 0;
#pragma unroll
            for (int t = 0; t < 9; t++) {
                if ((t >= 6 && !y3) || (t % 3 == 2 && !x3)) continue;   // zero-weight taps
#pragma unroll
                for (int k = 0; k < CN; k++)   // (tw <= 36, g2 < 2^24: a 24-bit multiply)
                    e2[k] += (int)__umul24((unsigned)tw[t], (unsigned)L.g2[j][k][tp[t]]);
            }
            const uint2 g1 = L.g1[j][p1];
            const double m = (double)mb_rec_m1<S>(rw, j);
#pragma unroll
            for (int k = 0; k < CN; k++) num[k] += m * (double)(16384 * ch16(g1, k) - e2[k]);
        }
        const int den = (int)(rw[0] >> 22);
        double acc[CN];
#pragma unroll
        for (int k = 0; k < CN; k++) acc[k] = 0.0;
#pragma unroll
        for (int t = 0; t < 9; t++) {
            if ((t >= 6 && !y3) || (t % 3 == 2 && !x3)) continue;   // (adds of an exact 0)
            const double wt = (double)tw[t];
#pragma unroll
            for (int k = 0; k < CN; k++) acc[k] += wt * L.b2[k][tp[t]];
        }
#pragma unroll
        for (int k = 0; k < CN; k++) {
            const double b1 = den ? num[k] / ((double)den * 4194304.0) : 0.0;
            L.r1[k][e] = b1 + acc[k] / 64.0;
        }
    }
    __syncthreads();
    // R0 = L0_owner / 16384 + up(R1) over the tile's own pixels; L0 = 16384 g0 - E(g1), g0 = the
    // owner sample already in the mosaic
#pragma unroll
    for (int q = 0; q < kMbPQ; q++) {
        const uint2 pr = wk.px[q];
        const int s = (int)((pr.x >> 11) & 15u);
        if (s == kMbPxSlotInert) continue;
        const int i = (int)(pr.x & 2047u);
        const int x = G.X0 + (i % kBlendTileW), y = G.Y0 + i / kBlendTileW;
        // (global address space: the stores cannot alias the LDS arrays read by later pixels)
        typedef __attribute__((address_space(1))) uint8_t gu8;
        gu8 *po = (gu8 *)(P.out + (int64_t)f * P.out_fstride + (int64_t)y * P.out_pitch + x * CN);
        if (s == kMbPxSlotNone) {
#pragma unroll
            for (int k = 0; k < CN; k++) po[k] = 0;
            continue;
        }
        const int cls = (int)((pr.x >> 15) & 3u);
        int wy[3], wx[3];
        mb_cls_wt((cls & 2) != 0, wy);
        mb_cls_wt((cls & 1) != 0, wx);
        int e1[CN];   // <= 64 * 256 * 255: exact in int32
        double acc[CN];
#pragma unroll
        for (int k = 0; k < CN; k++) e1[k] = 0, acc[k] = 0.0;
        // the taps in the restatement's order (rows outer); an odd coordinate's third tap has
        // weight 0 and is skipped (it would add an exact 0) -- the list is grouped by parity
        // class (mb_prep), so a wave skips it together
#pragma unroll
        for (int u = 0; u < 3; u++) {
            if (u == 2 && wy[2] == 0) break;
#pragma unroll
            for (int v = 0; v < 3; v++) {
                if (v == 2 && wx[2] == 0) break;
                const int p = (int)(((pr.y >> (10 * u)) & 1023u) + ((pr.x >> (17 + 5 * v)) & 31u));
                const int wt = wy[u] * wx[v];
                const uint2 g1 = L.g1[s][p];
                const double wd = (double)wt;
#pragma unroll
                for (int k = 0; k < CN; k++) {
                    e1[k] += wt * ch16(g1, k);
                    acc[k] += wd * L.r1[k][p];
                }
            }
        }
#pragma unroll
        for (int k = 0; k < CN; k++) {
            const int l0 = 16384 * (int)((wk.v[q] >> (8 * k)) & 0xffu) - e1[k];
            const double r0 = (double)l0 / 16384.0 + acc[k] / 64.0;
            const double vf = floor(r0 + 0.5);
            po[k] = (uint8_t)(vf < 0.0 ? 0.0 : (vf > 255.0 ? 255.0 : vf));
        }
    }
}

template <int CN, int S>
__device__ __forceinline__ void mb_blend(const KMbArgs &a, MbBlLds<CN, S> &L)
{
    typedef __attribute__((address_space(1))) const uint8_t cgu8;
    typedef __attribute__((address_space(1))) const uint2 cgu2;
    typedef __attribute__((address_space(1))) const int32_t cgi32;
    const KParams &P = a.P;
    // (tile, capture) units dealt XCD-grouped: a tile's captures share its tables in one L2
    int ux, fl;
    if (!xcd_unit(a.n_list, a.nf, ux, fl)) return;   // (block-uniform, before any barrier)
    const int bt = a.list0 + ux, tid = threadIdx.x;
    // Every global read of the block in one round.  What depends on nothing but the list index
    // and the thread goes first: the first iteration of both record lists and the B2 operands of
    // level-2 entry `tid` (the tables hold zeros for the slots past the tile's owners).
    typedef __attribute__((address_space(1))) const uint32_t cgu32;
    constexpr int RW = mb_r1rec_words(S);
    const cgu32 *rec = (const cgu32 *)a.rec + (int64_t)bt * mb_rec_words(S);
    const cgu2 *rec_px = (const cgu2 *)rec;
    const cgu32 *rec_r1 = rec + 2 * kMbTilePx;
    const cgi32 *tab = (const cgi32 *)a.tab + (int64_t)bt * mb_tab_words(a.slots);
    const cgi32 *t_m2 = tab + a.slots * kMbNRX * kMbNRY;
    const cgi32 *t_d2 = t_m2 + a.slots * kMbN2X * kMbN2Y + kMbNRX * kMbNRY;
    MbWork<CN, S> wk;
    wk.px[0] = rec_px[tid];
#pragma unroll
    for (int w = 0; w < RW; w++) wk.r1[0][w] = rec_r1[tid * RW + w];
    {
        const int e = min(tid, kMbN2X * kMbN2Y - 1);
#pragma unroll
        for (int j = 0; j < S; j++)   // (a slot past the table's: row 0 again, never used)
            wk.m2[j] = t_m2[(j < a.slots ? j : 0) * (kMbN2X * kMbN2Y) + e];
        wk.d2 = t_d2[e];
    }
    // The list entry and the counts (uniform loads) say how far the lists run: a tile's later
    // iterations are whole iterations of records too, loaded only where the list reaches them.
    const uint32_t mask = (uint32_t)a.list[2 + 2 * bt];
    const int ns = __popc(mask), f = a.f0 + fl;
    const MbGeo G = mb_geo(P, a.list[1 + 2 * bt]);
    const cgi32 *tc = t_d2 + kMbN2X * kMbN2Y;
    const int n_px = tc[0], n_r1 = tc[1];
    if (n_px == 0) return;   // uniform: no mixed pixel in this tile (before any barrier)
#pragma unroll
    for (int q = 1; q < kMbPQ; q++) {
        wk.px[q] = make_uint2((uint32_t)kMbPxSlotInert << 11, 0u);
        if (q * kMbBlThreads < n_px) wk.px[q] = rec_px[tid + q * kMbBlThreads];
    }
#pragma unroll
    for (int it = 1; it < kMbR1Iters; it++) {
#pragma unroll
        for (int w = 0; w < RW; w++) wk.r1[it][w] = w == 0 ? (uint32_t)kMbR1Inert : 0u;
        if (it * kMbBlThreads < n_r1) {
#pragma unroll
            for (int w = 0; w < RW; w++) wk.r1[it][w] = rec_r1[(tid + it * kMbBlThreads) * RW + w];
        }
    }
    constexpr int N1 = (kMbNRX * kMbNRY + kMbBlThreads - 1) / kMbBlThreads;
    constexpr int N2 = (kMbN2X * kMbN2Y * CN + kMbBlThreads - 1) / kMbBlThreads;
    // (the eight-owner kernels stage four owners at a time: all eight beside the records would
    // pass 128 registers)
    constexpr int SG = S > 4 ? 4 : S;
#pragma unroll
    for (int j0 = 0; j0 < S; j0 += SG) {
        if (j0 >= ns) break;
        uint2 r1[SG][N1];
        int32_t r2[SG][N2];
#pragma unroll
        for (int j = 0; j < SG; j++) {
            if (j0 + j >= ns) break;
            const int64_t job = ((int64_t)bt * a.slots + j0 + j) * a.chunk + fl;
            const cgu2 *s1 = (const cgu2 *)a.g1 + job * (kMbNRX * kMbNRY);
            const cgi32 *s2 = (const cgi32 *)a.g2 + job * (kMbN2X * kMbN2Y * CN);
#pragma unroll
            for (int q = 0; q < N1; q++)
                r1[j][q] = s1[min(tid + q * kMbBlThreads, kMbNRX * kMbNRY - 1)];
#pragma unroll
            for (int q = 0; q < N2; q++)
                r2[j][q] = s2[min(tid + q * kMbBlThreads, kMbN2X * kMbN2Y * CN - 1)];
        }
        // (the scratch holds an entry's channels together, mb_g2_at; LDS is channel-planar)
#pragma unroll
        for (int j = 0; j < SG; j++) {
            if (j0 + j >= ns) break;
#pragma unroll
            for (int q = 0; q < N1; q++)
                if (tid + q * kMbBlThreads < kMbNRX * kMbNRY)
                    L.g1[j0 + j][tid + q * kMbBlThreads] = r1[j][q];
#pragma unroll
            for (int q = 0; q < N2; q++) {
                const int e = tid + q * kMbBlThreads;
                if (e < kMbN2X * kMbN2Y * CN) L.g2[j0 + j][e % CN][e / CN] = r2[j][q];
            }
        }
    }
    // the owner samples of the thread's pixels: the one read that needs a record (first used in
    // R0, behind both barriers)
#pragma unroll
    for (int q = 0; q < kMbPQ; q++) {
        const uint32_t w = wk.px[q].x;
        const int i = (int)(w & 2047u);
        const int x = G.X0 + (i % kBlendTileW), y = G.Y0 + i / kBlendTileW;
        // (unconditional: an inert record names tile pixel 0, which lies inside the mosaic)
        const cgu8 *po = (const cgu8 *)(P.out + (int64_t)f * P.out_fstride +
                                        (int64_t)y * P.out_pitch + x * CN);
        wk.v[q] = 0;
#pragma unroll
        for (int k = 0; k < CN; k++) wk.v[q] |= (uint32_t)po[k] << (8 * k);
    }
    __syncthreads();
    // (the records hold reflected and clamped indices: interior and edge tiles run the same code)
    mb_blend_tile<CN, S>(a, G, L, wk, ns, n_r1, f);
}

}  // namespace mcs
