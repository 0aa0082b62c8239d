// mcs_mb_prep.h -- multi-band prep kernel (mcs_mb_prep_*), once per plan.
#pragma once

#include "mcs_blend.h"

namespace mcs {

// ---- prep (once per plan): grid (listed tiles), block kMbPrepThreads ---------------------------
template <int CN, int INTERP>
__device__ __forceinline__ void mb_prep(const KMbArgs &a)
{
    __shared__ uint8_t own[kMbU];
    __shared__ int32_t m1[kBlendSlots][kMbN1X * kMbN1Y];
    __shared__ int32_t m2[kBlendSlots][kMbN2X * kMbN2Y];
    const KParams &P = a.P;
    const int bt = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const uint32_t mask = (uint32_t)a.list[2 + 2 * bt];
    const int ns = __popc(mask);
    const MbGeo G = mb_geo(P, a.list[1 + 2 * bt]);
    const int w5[5] = {1, 4, 6, 4, 1};
    // owner map of the used neighbourhood as local slot indices (bit rank in `mask`)
    for (int i = tid; i < kMbU; i += nt) {
        const int cx = refl(G.RX + kMbFirst + i % kMbUsedX, G.W);
        const int cy = refl(G.RY + kMbFirst + i / kMbUsedX, G.H);
        const int o = a.owner[(int64_t)cy * G.W + cx];
        own[i] = (uint8_t)((o != kBlendNone && ((mask >> o) & 1u))
                               ? __popc(mask & ((1u << o) - 1u)) : kBlendNone);
    }
    const int RX2 = G.RX + kMbFirst, RY2 = G.RY + kMbFirst;
    // m1 = reduce(owner == slot) over the level-1 array (25-tap form with reflection)
    for (int i = tid; i < kMbN1X * kMbN1Y * ns; i += nt) {
        const int j = i / (kMbN1X * kMbN1Y), e = i % (kMbN1X * kMbN1Y);
        const int qx = refl(G.X1 + e % kMbN1X, G.w1), qy = refl(G.Y1 + e / kMbN1X, G.h1);
        int macc = 0;
        for (int u = 0; u < 5; u++) {
            const int cy = refl(2 * qy + u - 2, G.H);
            for (int v = 0; v < 5; v++) {
                const int cx = refl(2 * qx + v - 2, G.W);
                const int p = ix2<false>(cy, RY2, kMbUsedY) * kMbUsedX + ix2<false>(cx, RX2, kMbUsedX);
                macc += own[p] == j ? w5[u] * w5[v] : 0;
            }
        }
        m1[j][e] = macc;
    }
    __syncthreads();
    // m2 = reduce(m1)
    for (int i = tid; i < kMbN2X * kMbN2Y * ns; i += nt) {
        const int j = i / (kMbN2X * kMbN2Y), e = i % (kMbN2X * kMbN2Y);
        const int zx = refl(G.X2 + e % kMbN2X, G.w2), zy = refl(G.Y2 + e / kMbN2X, G.h2);
        int macc = 0;
        for (int u = 0; u < 5; u++) {
            const int qy = refl(2 * zy + u - 2, G.h1);
            for (int v = 0; v < 5; v++) {
                const int qx = refl(2 * zx + v - 2, G.w1);
                const int p = ix2<false>(qy, G.Y1, kMbN1Y) * kMbN1X + ix2<false>(qx, G.X1, kMbN1X);
                macc += w5[u] * w5[v] * m1[j][p];
            }
        }
        m2[j][e] = macc;
    }
    __syncthreads();
    // table: m1 (R1 region) [slots], m2 [slots], d1 (R1 region), d2
    int32_t *tab = a.tab + (int64_t)bt * mb_tab_words(a.slots);
    int32_t *t_m1 = tab, *t_m2 = tab + a.slots * kMbNRX * kMbNRY;
    int32_t *t_d1 = t_m2 + a.slots * kMbN2X * kMbN2Y, *t_d2 = t_d1 + kMbNRX * kMbNRY;
    for (int e = tid; e < kMbNRX * kMbNRY; e += nt) {
        const int p = (e / kMbNRX + kMbRS) * kMbN1X + e % kMbNRX + kMbRS;
        int d = 0;
        for (int j = 0; j < a.slots; j++) {
            const int v = j < ns ? m1[j][p] : 0;
            t_m1[j * kMbNRX * kMbNRY + e] = v;
            d += v;
        }
        t_d1[e] = d;
    }
    for (int e = tid; e < kMbN2X * kMbN2Y; e += nt) {
        int d = 0;
        for (int j = 0; j < a.slots; j++) {
            const int v = j < ns ? m2[j][e] : 0;
            t_m2[j * kMbN2X * kMbN2Y + e] = v;
            d += v;
        }
        t_d2[e] = d;
    }
    // The blend work lists.  A pixel's collapse equals its owner's sample exactly (bit for bit)
    // when no other owner's level-2 mask reaches a level-2 tap of its level-1 taps: B1 and B2 are
    // then the owner's own l1 / 2^22 and g2 / 2^16 (one-term quotients of exact integers), R1 =
    // g1 / 256 and R0 = g0 exactly (all dyadic, no rounding).  The stitch kernel has written that
    // sample (or the border 0 where no camera covers the pixel), so the blend kernel computes only
    // the other ("mixed") pixels and the R1 entries they read.
    __shared__ int need_r1[kMbNRX * kMbNRY];
    __shared__ int n_px, n_r1;
    // Both lists are stored grouped by the parity class of their expand taps (mb_cls: row
    // parity, column parity -> 3 or 2 taps per axis), so the blend kernel's waves run one
    // fixed-count tap body each (4, 6 or 9 taps instead of 9 with zero-weight padding)
    __shared__ uint8_t px_cls[kMbTilePx];
    __shared__ int cls_n[2][4], cls_at[2][4];
    // per owner slot: mosaic level-1 / level-2 columns the blend reads from it (band pass)
    __shared__ int nq1lo[kBlendSlots], nq1hi[kBlendSlots], nz2lo[kBlendSlots], nz2hi[kBlendSlots];
    int32_t *t_cnt = t_d2 + kMbN2X * kMbN2Y;
    uint16_t *t_px = reinterpret_cast<uint16_t *>(t_cnt + kMbTabCounts);
    uint16_t *t_r1 = t_px + kMbTilePx;
    for (int e = tid; e < kMbNRX * kMbNRY; e += nt) need_r1[e] = 0;
    for (int i = tid; i < kMbTilePx; i += nt) px_cls[i] = 255;
    if (tid < 8) cls_n[tid >> 2][tid & 3] = 0;
    if (tid == 0) n_px = n_r1 = 0;
    if (tid < kBlendSlots) {
        nq1lo[tid] = nz2lo[tid] = 1 << 30;
        nq1hi[tid] = nz2hi[tid] = -(1 << 30);
    }
    __syncthreads();
    for (int i = tid; i < kMbTilePx; i += nt) {
        const int x = G.X0 + i % kBlendTileW, y = G.Y0 + i / kBlendTileW;
        if (x >= G.W || y >= G.H) continue;
        const int o = a.owner[(int64_t)y * G.W + x];
        if (o == kBlendNone) continue;
        const int s = __popc(mask & ((1u << o) - 1u));
        int iy[3], wy[3], ix[3], wx[3];
        exp_taps<false>(y, G.h1, iy, wy);
        exp_taps<false>(x, G.w1, ix, wx);
        bool mixed = false;
        for (int u = 0; u < 3; u++)
            for (int v = 0; v < 3; v++) {
                int zy[3], uy[3], zx[3], ux[3];
                exp_taps<false>(iy[u], G.h2, zy, uy);
                exp_taps<false>(ix[v], G.w2, zx, ux);
                for (int b = 0; b < 3; b++)
                    for (int c = 0; c < 3; c++) {
                        const int e2 = ix2<false>(zy[b], G.Y2, kMbN2Y) * kMbN2X +
                                       ix2<false>(zx[c], G.X2, kMbN2X);
                        for (int j = 0; j < ns; j++)
                            mixed = mixed || (j != s && m2[j][e2] > 0);
                    }
            }
        if (!mixed) continue;
        atomicAdd(&n_px, 1);
        px_cls[i] = (uint8_t)mb_cls(x, y);
        atomicAdd(&cls_n[0][px_cls[i]], 1);
        for (int u = 0; u < 3; u++)
            for (int v = 0; v < 3; v++)
                need_r1[ix2<false>(iy[u], G.YR, kMbNRY) * kMbNRX + ix2<false>(ix[v], G.XR, kMbNRX)] =
                    1;
        // R0 reads the owner's g1 at the pixel's level-1 taps
        atomicMin(&nq1lo[s], min(ix[0], ix[1]));
        atomicMax(&nq1hi[s], max(ix[1], ix[2]));
    }
    __syncthreads();
    for (int e = tid; e < kMbNRX * kMbNRY; e += nt)
        if (need_r1[e]) {
            atomicAdd(&n_r1, 1);
            atomicAdd(&cls_n[1][mb_cls(G.XR + e % kMbNRX, G.YR + e / kMbNRX)], 1);
        }
    __syncthreads();
    if (tid < 2) {
        int at = 0;
        for (int c = 0; c < 4; c++) cls_at[tid][c] = at, at += cls_n[tid][c];
    }
    __syncthreads();
    // (the lists also stay in LDS: the work records below are built from them)
    __shared__ uint16_t l_px[kMbTilePx], l_r1[kMbNRX * kMbNRY];
    for (int i = tid; i < kMbTilePx; i += nt)
        if (px_cls[i] != 255) {
            const int l = atomicAdd(&cls_at[0][px_cls[i]], 1);
            t_px[l] = l_px[l] = (uint16_t)i;
        }
    for (int e = tid; e < kMbNRX * kMbNRY; e += nt)
        if (need_r1[e]) {
            const int l = atomicAdd(&cls_at[1][mb_cls(G.XR + e % kMbNRX, G.YR + e / kMbNRX)], 1);
            t_r1[l] = l_r1[l] = (uint16_t)e;
        }
    // R1 at a listed entry reads owner j's g1 there and g2 at its level-2 taps where m1_j > 0,
    // and B2 at those taps reads g2_j where m2_j > 0 (positions in the mosaic: reflected, as the
    // blend kernel addresses them)
    for (int e = tid; e < kMbNRX * kMbNRY; e += nt) {
        if (!need_r1[e]) continue;
        const int ey = e / kMbNRX, ex = e % kMbNRX;
        const int p = (ey + kMbRS) * kMbN1X + ex + kMbRS;
        const int qx = G.XR + ex, qy = G.YR + ey;
        int zy[3], uy[3], zx[3], ux[3];
        exp_taps<false>(qy, G.h2, zy, uy);
        exp_taps<false>(qx, G.w2, zx, ux);
        for (int j = 0; j < ns; j++) {
            if (m1[j][p] > 0) {
                atomicMin(&nq1lo[j], qx);
                atomicMax(&nq1hi[j], qx);
            }
            for (int b = 0; b < 3; b++)
                for (int c = 0; c < 3; c++)
                    if (m2[j][ix2<false>(zy[b], G.Y2, kMbN2Y) * kMbN2X +
                              ix2<false>(zx[c], G.X2, kMbN2X)] > 0) {
                        atomicMin(&nz2lo[j], zx[c]);
                        atomicMax(&nz2hi[j], zx[c]);
                    }
        }
    }
    __syncthreads();
    // The blend work records (mcs_kparams.h): per listed pixel and per listed R1 entry every index
    // mb_blend would otherwise work out per capture, reflection and clamping included, and the R1
    // entry's mask weights and denominator; the lists' tails padded with inert records.
    {
        const int RS = mb_rec_slots(a.slots), RW = mb_r1rec_words(a.slots);
        uint32_t *rec = a.rec + (int64_t)bt * mb_rec_words(a.slots);
        uint32_t *rec_r1 = rec + 2 * kMbTilePx;
        for (int l = tid; l < kMbTilePx; l += nt) {
            uint32_t w0 = (uint32_t)kMbPxSlotInert << 11, w1 = 0;
            if (l < n_px) {
                const int i = l_px[l];
                const int x = G.X0 + i % kBlendTileW, y = G.Y0 + i / kBlendTileW;
                const int o = a.owner[(int64_t)y * G.W + x];
                const int s = o == kBlendNone ? kMbPxSlotNone : __popc(mask & ((1u << o) - 1u));
                int iy[3], wy[3], ix[3], wx[3];
                exp_taps<false>(y, G.h1, iy, wy);
                exp_taps<false>(x, G.w1, ix, wx);
                w0 = (uint32_t)i | ((uint32_t)s << 11) | ((uint32_t)mb_cls(x, y) << 15);
                for (int v = 0; v < 3; v++) {
                    w0 |= (uint32_t)ix2<false>(ix[v], G.XR, kMbNRX) << (17 + 5 * v);
                    w1 |= (uint32_t)(ix2<false>(iy[v], G.YR, kMbNRY) * kMbNRX) << (10 * v);
                }
            }
            rec[2 * l] = w0;
            rec[2 * l + 1] = w1;
        }
        for (int l = tid; l < kMbRecR1; l += nt) {
            uint32_t *r = rec_r1 + l * RW;
            uint32_t w0 = kMbR1Inert, w1 = 0;
            int p = 0;
            if (l < n_r1) {
                const int e = l_r1[l];
                const int qx = refl(G.XR + e % kMbNRX, G.w1), qy = refl(G.YR + e / kMbNRX, G.h1);
                int iy[3], wy[3], ix[3], wx[3];
                exp_taps<false>(qy, G.h2, iy, wy);
                exp_taps<false>(qx, G.w2, ix, wx);
                const int py = ix2<false>(qy, G.YR, kMbNRY), px = ix2<false>(qx, G.XR, kMbNRX);
                p = (py + kMbRS) * kMbN1X + px + kMbRS;   // (m1 is held over the level-1 array)
                int d = 0;
                for (int j = 0; j < ns; j++) d += m1[j][p];
                w0 = (uint32_t)e | ((uint32_t)(py * kMbNRX + px) << 10) |
                     ((uint32_t)mb_cls(qx, qy) << 20) | ((uint32_t)d << 22);
                for (int v = 0; v < 3; v++) {
                    w1 |= (uint32_t)ix2<false>(iy[v], G.Y2, kMbN2Y) << (5 * v);
                    w1 |= (uint32_t)ix2<false>(ix[v], G.X2, kMbN2X) << (15 + 4 * v);
                }
            }
            r[0] = w0;
            r[1] = w1;
            for (int j = 0; j < RS; j += 2) {
                const uint32_t ma = l < n_r1 && j < ns ? (uint32_t)m1[j][p] : 0u;
                const uint32_t mb = l < n_r1 && j + 1 < ns ? (uint32_t)m1[j + 1][p] : 0u;
                r[2 + j / 2] = ma | (mb << 16);
            }
        }
    }
    // Column ranges of the level arrays the mixed pixels depend on (interior tiles; mosaic-border
    // tiles keep the full arrays): R1 entries -> their level-2 taps -> the level-1 entries the R1
    // region and those taps reduce from -> the level-0 samples.  mb_levels computes only these.
    __shared__ int r1lo, r1hi, rng[6];
    if (tid == 0) r1lo = kMbNRX, r1hi = -1;
    __syncthreads();
    for (int e = tid; e < kMbNRX * kMbNRY; e += nt)
        if (need_r1[e]) {
            atomicMin(&r1lo, e % kMbNRX);
            atomicMax(&r1hi, e % kMbNRX);
        }
    __syncthreads();
    if (tid == 0) {
        int a0_ = 0, b0_ = kMbUsedX - 1, a1_ = 0, b1_ = kMbN1X - 1, a2_ = 0, b2_ = kMbN2X - 1;
        if (n_px == 0) {
            a0_ = a1_ = a2_ = 0;
            b0_ = b1_ = b2_ = -1;
        } else if (G.interior) {
            int zlo = 1 << 30, zhi = -(1 << 30);
            for (int q = G.XR + r1lo; q <= G.XR + r1hi; q++) {
                int zi[3], zw[3];
                exp_taps<true>(q, G.w2, zi, zw);
                zlo = min(zlo, min(zi[0], zi[1]));
                zhi = max(zhi, max(zi[1], zi[2]));
            }
            a2_ = max(zlo - G.X2, 0);
            b2_ = min(zhi - G.X2, kMbN2X - 1);
            a1_ = max(min(G.XR + r1lo, 2 * zlo - 2) - G.X1, 0);
            b1_ = min(max(G.XR + r1hi, 2 * zhi + 2) - G.X1, kMbN1X - 1);
            a0_ = max(2 * (a1_ + G.X1) - 2 - (G.RX + kMbFirst), 0);
            b0_ = min(2 * (b1_ + G.X1) + 2 - (G.RX + kMbFirst), kMbUsedX - 1);
        }
        rng[0] = a0_, rng[1] = b0_, rng[2] = a1_, rng[3] = b1_, rng[4] = a2_, rng[5] = b2_;
        t_cnt[0] = n_px;
        t_cnt[1] = n_r1;
        for (int q = 0; q < 6; q++) t_cnt[2 + q] = rng[q];
        for (int j = 0; j < kBlendSlots; j++) {
            int q1lo = nq1lo[j], q1hi = nq1hi[j], z2lo = nz2lo[j], z2hi = nz2hi[j];
            if (n_px == 0 || j >= ns) {
                q1lo = z2lo = 1 << 30;
                q1hi = z2hi = -(1 << 30);
            } else if (q1lo <= q1hi) {
                // the level-2 taps of those g1 entries (L1 = 16384 g1 - E(g2))
                z2lo = min(z2lo, (q1lo - 1) >> 1);
                z2hi = max(z2hi, (q1hi >> 1) + 1);
            }
            t_cnt[kMbTabRanges + 4 * j + 0] = q1lo;
            t_cnt[kMbTabRanges + 4 * j + 1] = q1hi;
            t_cnt[kMbTabRanges + 4 * j + 2] = z2lo;
            t_cnt[kMbTabRanges + 4 * j + 3] = z2hi;
        }
    }
    __syncthreads();
    const int a0 = rng[0], w0 = rng[1] - rng[0] + 1, n_s = kMbUsedY * w0;
    // every owner's source footprint (bounding box of its taps) ...
    __shared__ int f_rmin[kBlendSlots], f_rmax[kBlendSlots], f_bmin[kBlendSlots],
        f_bmax[kBlendSlots];
    __shared__ MbFoot foot[kBlendSlots];
    if (tid < kBlendSlots) {
        f_rmin[tid] = f_bmin[tid] = 0x7fffffff;
        f_rmax[tid] = f_bmax[tid] = -1;
    }
    __syncthreads();
    for (int i = tid; i < n_s * ns; i += nt) {
        const int j = i / n_s, e = i % n_s;
        const int g = mb_sample_index(e, a0, w0);
        const int cx = refl(G.RX + kMbFirst + g % kMbUsedX, G.W);
        const int cy = refl(G.RY + kMbFirst + g / kMbUsedX, G.H);
        const MbSrc q = mb_src<INTERP>(P, mb_slot(mask, j), cx, cy);
        atomicMin(&f_rmin[j], q.ya);
        atomicMax(&f_rmax[j], q.yb);
        atomicMin(&f_bmin[j], q.c * CN);
        atomicMax(&f_bmax[j], q.c * CN + 2 * CN);
    }
    __syncthreads();
    if (tid < ns) {
        int cam, w, h;
        slot_info(P, mb_slot(mask, tid), cam, w, h);
        const int64_t pitch = (int64_t)w * CN;
        MbFoot F;
        F.rmin = f_rmin[tid];
        F.rows = f_rmax[tid] - f_rmin[tid] + 1;
        F.cal = f_bmin[tid] & ~15;
        F.stride = (f_bmax[tid] - F.cal + 15) & ~15;
        F.e = 0;
        // (rows above the last one may run into the next row, never past the frame)
        F.fits = F.rows * F.stride + kLdsSlack <= kMbFoot &&
                 F.stride <= 16 * kWave && F.cal + F.stride <= 2 * pitch;
        if (f_rmax[tid] == h - 1 && F.cal + F.stride > pitch) {
            F.e = (int)(F.cal + F.stride - pitch);
            if ((int64_t)(h - 1) * pitch + F.cal - F.e < 0) F.fits = 0;
        }
        F.pad0 = F.pad1 = 0;
        foot[tid] = F;
        reinterpret_cast<MbFoot *>(a.foot)[(int64_t)bt * a.slots + tid] = F;
    }
    __syncthreads();
    // ... and every needed level-0 sample's windows: LDS offsets in the footprint, or frame
    // offsets; .y bits 16-27 = its index in the 57 x 57 level-0 array
    for (int i = tid; i < n_s * ns; i += nt) {
        const int j = i / n_s, e = i % n_s;
        const int g = mb_sample_index(e, a0, w0);
        const int cx = refl(G.RX + kMbFirst + g % kMbUsedX, G.W);
        const int cy = refl(G.RY + kMbFirst + g / kMbUsedX, G.H);
        const int sj = mb_slot(mask, j);
        const MbSrc q = mb_src<INTERP>(P, sj, cx, cy);
        int cam, w, h;
        slot_info(P, sj, cam, w, h);
        const MbFoot &F = foot[j];
        uint2 v;
        if (F.fits) {
            v.x = mb_foot_off(F, q.ya, q.c * CN, h) | (mb_foot_off(F, q.yb, q.c * CN, h) << 16);
            v.y = q.meta;
        } else {
            v = mb_desc<CN>(q, w, h);
        }
        v.y |= (uint32_t)g << 16;
        a.desc[((int64_t)bt * a.slots + j) * kMbU + e] = (uint64_t)v.x | ((uint64_t)v.y << 32);
    }
}

}  // namespace mcs
