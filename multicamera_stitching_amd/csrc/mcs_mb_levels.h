// mcs_mb_levels.h -- multi-band levels kernel (mcs_mb_levels_*): the per-tile fallback of the band pass.
#pragma once

#include "mcs_blend.h"

namespace mcs {

// ---- levels: grid (listed tiles, slots, ceil(nf / kMbLvFrames)), block kMbLvThreads -------------
template <int CN>
struct MbLvLds {
    uint8_t foot[kMbFootBufs][kMbFoot] __attribute__((aligned(16)));   // source footprints
    // (one spare entry past each array: the branch-free stores of out-of-range items land there)
    uint32_t g0[kMbU + 1];             // level 0: channel k in byte k
    uint2 g1[kMbN1X * kMbN1Y + 1];     // 256 G1 <= 65280 as u16 lanes: x = (c0, c2), y = (c1, c3)
    union {
        uint2 hs[kMbUsedY * kMbN1X + 1];   // horizontal pass of level 1 (<= 4080), lanes as g1
        int4 hs2[kMbN1Y * kMbN2X];     // horizontal pass of level 2, one int per channel
    };
};

template <int CN, bool GAIN = false>
__device__ __forceinline__ void mb_levels(const KMbArgs &a, MbLvLds<CN> &L)
{
    constexpr int NT = kMbLvThreads, KJ = (kMbU + NT - 1) / NT;
    const KParams &P = a.P;
    const int bt = blockIdx.x, j = blockIdx.y, tid = threadIdx.x;
    const uint32_t mask = (uint32_t)a.list[2 + 2 * bt];
    if (j >= __popc(mask)) return;   // uniform: the whole block leaves before any barrier
    const MbGeo G = mb_geo(P, a.list[1 + 2 * bt]);
    // the column ranges the tile's mixed pixels depend on (mb_prep): level 0 [a0, a0 + w0),
    // level 1 [a1, a1 + w1), level 2 [a2, a2 + w2); all rows
    const int32_t *rg = a.tab + (int64_t)bt * mb_tab_words(a.slots) +
                        a.slots * (kMbNRX * kMbNRY + kMbN2X * kMbN2Y) + kMbNRX * kMbNRY +
                        kMbN2X * kMbN2Y + 2;
    const int w0 = rg[1] - rg[0] + 1, a1 = rg[2], w1 = rg[3] - rg[2] + 1;
    const int a2 = rg[4], w2 = rg[5] - rg[4] + 1;
    const int n_s = kMbUsedY * w0;                   // level-0 samples (compacted columns)
    if (n_s <= 0) return;                            // no mixed pixel: nothing to do (uniform)
    const unsigned d1m = (65536u + w1 - 1) / w1, d2m = (65536u + w2 - 1) / w2;   // / w1, / w2
    int cam, w, h;
    slot_info(P, mb_slot(mask, j), cam, w, h);
    // (GAIN: the owner's camera is uniform over the block: its q halves live in SGPRs)
    const GainQ gq = GAIN ? gain_pair(gain_q_of(P, cam)) : GainQ();
    const int64_t pitch = (int64_t)w * CN, fbytes = pitch * h;
    const MbFoot F = reinterpret_cast<const MbFoot *>(a.foot)[(int64_t)bt * a.slots + j];
    const bool staged = F.fits;                      // footprint through LDS (else global loads)
    const bool shifted = (h - 1) * pitch >= 16;
    // this owner's sample windows, once for the block's captures (global path with frames of
    // (h - 1) * pitch < 16 bytes: re-read per capture, load8's guarded path)
    uint32_t doff[KJ], dmeta[KJ];
    const uint64_t *dsc = a.desc + ((int64_t)bt * a.slots + j) * kMbU;
#pragma unroll
    for (int kk = 0; kk < KJ; kk++) {
        const int i = tid + kk * NT;
        const uint64_t v = ((staged || shifted) && i < n_s) ? dsc[i] : 0ull;
        doff[kk] = (uint32_t)v;
        dmeta[kk] = (uint32_t)(v >> 32);
    }
    const int w5[5] = {1, 4, 6, 4, 1};
    const int fl0 = blockIdx.z * kMbLvFrames, fl1 = min(a.nf, fl0 + kMbLvFrames);
    // LDS-DMA of capture fl's footprint into buffer b: row r by wave r % 8, lane = 16-byte chunk
    const int wave = __builtin_amdgcn_readfirstlane(tid / kWave), lane = tid % kWave;
    auto stage = [&](int fl, int b) {
        const uint8_t *fb = P.cams[cam] + (int64_t)(a.f0 + fl) * P.cam_fstride[cam];
        for (int r = wave; r < F.rows; r += NT / kWave) {
            const int row = F.rmin + r;
            const uint8_t *src = fb + (int64_t)row * pitch + F.cal - (row == h - 1 ? F.e : 0);
            if (lane < (F.stride >> 4))
                __builtin_amdgcn_global_load_lds(src + 16 * lane,
                                                 ((lds_u8 *)L.foot[b]) + r * F.stride, 16, 0, 0);
        }
    };
    if (staged && fl0 < fl1) stage(fl0, 0);
    for (int fl = fl0; fl < fl1; fl++) {
        const uint8_t *fb = P.cams[cam] + (int64_t)(a.f0 + fl) * P.cam_fstride[cam];
        // level 0.  The descriptors are made opaque per capture so that the compiler does not
        // hoist their decoding out of the loop (which would hold ~5 registers per sample).
        if (staged) {
            // this capture's footprint has landed (every wave's DMA: wait + barrier); the next
            // one streams in while this one is processed
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (kMbFootBufs == 2 && fl + 1 < fl1) stage(fl + 1, (fl + 1 - fl0) & 1);
            const uint8_t *buf = L.foot[kMbFootBufs == 2 ? (fl - fl0) & 1 : 0];
            // all samples into registers first: a level-0 store between them would order the
            // next sample's LDS reads behind it (the compiler cannot tell the arrays apart)
            uint32_t px[KJ];
            mb_opaque(doff);
            mb_opaque(dmeta);
#pragma unroll
            for (int kk = 0; kk < KJ; kk++) {
                const uint2 r0 = lds_window(buf, doff[kk] & 0xffffu);
                const uint2 r1 = lds_window(buf, doff[kk] >> 16);
                uint32_t wa, wb;
                mb_weights(dmeta[kk], wa, wb);
                px[kk] = 0;
#pragma unroll
                for (int k = 0; k < CN; k++) px[kk] |= mb_tap<CN, GAIN>(r0, r1, wa, wb, k, 0u, gq) << (8 * k);
            }
#pragma unroll
            for (int kk = 0; kk < KJ; kk++)
                L.g0[tid + kk * NT < n_s ? (dmeta[kk] >> 16) & 0x1fffu : (uint32_t)kMbU] = px[kk];
        } else if (shifted) {
            struct __attribute__((packed)) U2 {
                uint32_t x, y;
            };
            typedef __attribute__((address_space(1))) const uint8_t gu8;
            typedef __attribute__((address_space(1))) const U2 gu2;
            const gu8 *gfb = (const gu8 *)fb;
            uint32_t px[KJ];
            mb_opaque(doff);
            mb_opaque(dmeta);
#pragma unroll
            for (int kk = 0; kk < KJ; kk++) {
                const uint32_t d = (dmeta[kk] >> 12) & 7u;
                const uint32_t o = (doff[kk] & 0x7fffffffu) - d;
                const uint32_t ob = o + ((doff[kk] >> 31) ? (uint32_t)pitch : 0u);
                const U2 ra = *(const gu2 *)(gfb + o), rb = *(const gu2 *)(gfb + ob);
                const uint2 r0 = make_uint2(ra.x, ra.y), r1 = make_uint2(rb.x, rb.y);
                uint32_t wa, wb;
                mb_weights(dmeta[kk], wa, wb);
                px[kk] = 0;
#pragma unroll
                for (int k = 0; k < CN; k++) px[kk] |= mb_tap<CN, GAIN>(r0, r1, wa, wb, k, d, gq) << (8 * k);
            }
#pragma unroll
            for (int kk = 0; kk < KJ; kk++)
                L.g0[tid + kk * NT < n_s ? (dmeta[kk] >> 16) & 0x1fffu : (uint32_t)kMbU] = px[kk];
        } else {
            for (int i = tid; i < n_s; i += NT) {
                const uint64_t v = dsc[i];
                const uint32_t o = (uint32_t)v & 0x7fffffffu;
                const uint32_t ob = o + (((uint32_t)v >> 31) ? (uint32_t)pitch : 0u);
                const uint2 r0 = load8<2 * CN>(fb, o, fbytes), r1 = load8<2 * CN>(fb, ob, fbytes);
                uint32_t wa, wb, px = 0;
                mb_weights((uint32_t)(v >> 32), wa, wb);
#pragma unroll
                for (int k = 0; k < CN; k++) px |= mb_tap<CN, GAIN>(r0, r1, wa, wb, k, 0u, gq) << (8 * k);
                L.g0[(uint32_t)(v >> 48) & 0x1fffu] = px;
            }
        }
        __syncthreads();
        // single buffer: the next capture's footprint streams in during this one's reduces
        if (kMbFootBufs == 1 && staged && fl + 1 < fl1) stage(fl + 1, 0);
        const int64_t job = ((int64_t)bt * a.slots + j) * a.chunk + fl;
        uint2 *og1 = reinterpret_cast<uint2 *>(a.g1) + job * (kMbNRX * kMbNRY);
        int32_t *og2 = a.g2 + job * (kMbN2X * kMbN2Y * CN);
        if (G.interior) {
            // separable 5-tap reduces, all channels at once in 16-bit lanes up to level 1 (the
            // sums stay below 2^16: exact), then per channel.  Level-1 entry e reads level-0
            // offsets 2e + [0, 5); level-2 entry z reads level-1 entries 2z + [0, 5).
            // (each thread's items are computed before any is stored, so that their LDS reads
            // are not ordered behind the stores; only the needed columns, all rows)
            {
                constexpr int IT = (kMbUsedY * kMbN1X + NT - 1) / NT;
                const int n = kMbUsedY * w1;
                uint2 res[IT];
#pragma unroll
                for (int q = 0; q < IT; q++) {
                    const int i = min(tid + q * NT, n - 1);
                    const int r = (int)(__umul24((unsigned)i, d1m) >> 16);
                    const int e = a1 + i - (int)__umul24((unsigned)r, (unsigned)w1);
                    const uint32_t *g = &L.g0[r * kMbUsedX + 2 * e];
                    uint32_t lo = 0, hi = 0;
#pragma unroll
                    for (int v = 0; v < 5; v++) {
                        const uint32_t t = g[v];
                        lo += (uint32_t)w5[v] * (t & 0x00ff00ffu);
                        hi += (uint32_t)w5[v] * ((t >> 8) & 0x00ff00ffu);
                    }
                    res[q] = make_uint2(lo, hi);
                }
#pragma unroll
                for (int q = 0; q < IT; q++) {
                    const int i = tid + q * NT;
                    const int r = (int)(__umul24((unsigned)i, d1m) >> 16);
                    L.hs[i < n ? r * kMbN1X + a1 + i - (int)__umul24((unsigned)r, (unsigned)w1)
                               : kMbUsedY * kMbN1X] = res[q];
                }
            }
            __syncthreads();
            {
                constexpr int IT = (kMbN1Y * kMbN1X + NT - 1) / NT;
                const int n = kMbN1Y * w1;
                uint2 res[IT];
#pragma unroll
                for (int q = 0; q < IT; q++) {
                    const int i = min(tid + q * NT, n - 1);
                    const int ey = (int)(__umul24((unsigned)i, d1m) >> 16);
                    const int ex = a1 + i - (int)__umul24((unsigned)ey, (unsigned)w1);
                    uint32_t lo = 0, hi = 0;
#pragma unroll
                    for (int u = 0; u < 5; u++) {
                        const uint2 t = L.hs[(2 * ey + u) * kMbN1X + ex];
                        lo += (uint32_t)w5[u] * t.x;
                        hi += (uint32_t)w5[u] * t.y;
                    }
                    res[q] = make_uint2(lo, hi);
                }
#pragma unroll
                for (int q = 0; q < IT; q++) {
                    const int i = tid + q * NT;
                    const int ey = (int)(__umul24((unsigned)i, d1m) >> 16);
                    L.g1[i < n ? ey * kMbN1X + a1 + i - (int)__umul24((unsigned)ey, (unsigned)w1)
                               : kMbN1X * kMbN1Y] = res[q];
                }
            }
            __syncthreads();
            for (int i = tid; i < kMbN1Y * w2; i += NT) {
                const int r = (int)(__umul24((unsigned)i, d2m) >> 16);
                const int e = a2 + i - (int)__umul24((unsigned)r, (unsigned)w2);
                int acc[4] = {0, 0, 0, 0};
#pragma unroll
                for (int v = 0; v < 5; v++) {
                    const uint2 t = L.g1[r * kMbN1X + 2 * e + v];
#pragma unroll
                    for (int k = 0; k < CN; k++) acc[k] += w5[v] * ch16(t, k);
                }
                L.hs2[r * kMbN2X + e] = make_int4(acc[0], acc[1], acc[2], acc[3]);
            }
            __syncthreads();
            for (int i = tid; i < kMbN2Y * w2; i += NT) {
                const int ey = (int)(__umul24((unsigned)i, d2m) >> 16);
                const int ex = a2 + i - (int)__umul24((unsigned)ey, (unsigned)w2);
                int acc[4] = {0, 0, 0, 0};
#pragma unroll
                for (int u = 0; u < 5; u++) {
                    const int4 t = L.hs2[(2 * ey + u) * kMbN2X + ex];
                    acc[0] += w5[u] * t.x;
                    acc[1] += w5[u] * t.y;
                    acc[2] += w5[u] * t.z;
                    acc[3] += w5[u] * t.w;
                }
#pragma unroll
                for (int k = 0; k < CN; k++) og2[mb_g2_at<CN>(ex, ey, k)] = acc[k];
            }
        } else {
            // mosaic-border tiles: 25-tap form with reflection at every level
            const int RX2 = G.RX + kMbFirst, RY2 = G.RY + kMbFirst;
            for (int e = tid; e < kMbN1X * kMbN1Y; e += NT) {
                const int qx = refl(G.X1 + e % kMbN1X, G.w1), qy = refl(G.Y1 + e / kMbN1X, G.h1);
                uint32_t lo = 0, hi = 0;
                for (int u = 0; u < 5; u++) {
                    const int cy = ix2<false>(refl(2 * qy + u - 2, G.H), RY2, kMbUsedY);
#pragma unroll
                    for (int v = 0; v < 5; v++) {
                        const int cx = ix2<false>(refl(2 * qx + v - 2, G.W), RX2, kMbUsedX);
                        const uint32_t t = L.g0[cy * kMbUsedX + cx], wt = w5[u] * w5[v];
                        lo += wt * (t & 0x00ff00ffu);
                        hi += wt * ((t >> 8) & 0x00ff00ffu);
                    }
                }
                L.g1[e] = make_uint2(lo, hi);
            }
            __syncthreads();
            for (int e = tid; e < kMbN2X * kMbN2Y; e += NT) {
                const int zx = refl(G.X2 + e % kMbN2X, G.w2), zy = refl(G.Y2 + e / kMbN2X, G.h2);
                int acc[4] = {0, 0, 0, 0};
                for (int u = 0; u < 5; u++) {
                    const int qy = ix2<false>(refl(2 * zy + u - 2, G.h1), G.Y1, kMbN1Y);
#pragma unroll
                    for (int v = 0; v < 5; v++) {
                        const int qx = ix2<false>(refl(2 * zx + v - 2, G.w1), G.X1, kMbN1X);
                        const uint2 t = L.g1[qy * kMbN1X + qx];
                        const int wt = w5[u] * w5[v];
#pragma unroll
                        for (int k = 0; k < CN; k++) acc[k] += wt * ch16(t, k);
                    }
                }
#pragma unroll
                for (int k = 0; k < CN; k++) og2[mb_g2_at<CN>(e % kMbN2X, e / kMbN2X, k)] = acc[k];
            }
        }
        // the R1 region of g1 (level-1 entries from kMbRS on, both axes)
        for (int e = tid; e < kMbNRX * kMbNRY; e += NT)
            og1[mb_g1_at(e % kMbNRX, e / kMbNRX)] =
                L.g1[(e / kMbNRX + kMbRS) * kMbN1X + e % kMbNRX + kMbRS];
        __syncthreads();   // the next capture overwrites level 0 and the pass arrays
    }
}

}  // namespace mcs
