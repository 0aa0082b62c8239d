// mcs_direct_mb.hip -- gfx950 kernels of the direct multi-band render
// (mcs_stitch_direct_multiband): the 3-level multi-band blend of oracle/orc_blend.c for a plan
// without prepared tables, bit for bit (integers and IEEE doubles in the oracle's order, no
// contraction).  A code object of its own: the stitch, feature and sweep objects, and so
// mcs_build_id, do not change with it.
//
// Two launches per call.
//   mcs_direct_mb_own_*   block (64, 8) over the 128 x 16 tiles of the direct path, grid y over
//                         blocks of kDirectFrames captures: every pixel from its owner (SEAM's
//                         arithmetic, 0 where no camera covers), and per 16 x 16 cell of the mosaic
//                         the OR of the owners' slot bits, written (not accumulated) to the work
//                         area by the blockIdx.y == 0 blocks: a cell lies in exactly one tile.
//   mcs_direct_mb_tile_*  one block of kDmbTileThreads per (32 x 64 blend tile, capture).  The OR
//                         of the cells of the tile's grown neighbourhood decides:
//                           <= 1 owner   nothing: the owner pass wrote the exact result
//                                        (mcs_mb_prep.h: a pixel no foreign mask reaches collapses
//                                        to its owner's sample bit for bit);
//                           > 8 owners   the feather rule for the tile's pixels (dense seams);
//                           otherwise    the specification in LDS, the owners one after another
//                                        (DmbLds, mcs_kparams.h), then B2, R1, R0 and the bytes of
//                                        every covered pixel of the tile.
// Arrays per level as in mcs_blend.h: level 0 [O - 14, O + T + 10], level 1 [O/2 - 6, O/2 + T/2 + 4],
// level 2 [O/4 - 2, O/4 + T/4 + 1], the R1 region [O/2 - 1, O/2 + T/2].  The entry at coordinate c
// holds the value at refl(c, n), so a tap is addressed by its unreflected coordinate; indices are
// clamped into the arrays, which only entries nothing reads ever need (entries past the mosaic's
// far edge whose reflection leaves the arrays).
#include "mcs_dev.h"

#include "mcs_blend.h"

namespace mcs {

// 4 * CN output bytes of 4 consecutive pixels as scalar words (see OutWords in mcs_kernels.hip).
struct DmbWords {
    uint32_t w0 = 0, w1 = 0, w2 = 0, w3 = 0;
    __device__ __forceinline__ void or_at(int i, uint32_t v)
    {
        if (i == 0) w0 |= v;
        else if (i == 1) w1 |= v;
        else if (i == 2) w2 |= v;
        else w3 |= v;
    }
    __device__ __forceinline__ uint32_t at(int i) const
    {
        return i == 0 ? w0 : (i == 1 ? w1 : (i == 2 ? w2 : w3));
    }
};

template <int CN>
__device__ __forceinline__ void dmb_put(DmbWords &w, int p, uint32_t v)
{
#pragma unroll
    for (int k = 0; k < CN; k++) {
        const int b = p * CN + k;
        w.or_at(b >> 2, ((v >> (8 * k)) & 0xffu) << (8 * (b & 3)));
    }
}

// Pixels [0, npx) of the group at o: dwords when all 4 are there and o is 4-byte aligned.
template <int CN>
__device__ __forceinline__ void dmb_store(uint8_t *o, const DmbWords &w, int npx, bool aligned)
{
    if (npx == kPx && aligned) {
        uint32_t *o32 = reinterpret_cast<uint32_t *>(o);
#pragma unroll
        for (int i = 0; i < CN; i++) o32[i] = w.at(i);
    } else {
        for (int b = 0; b < npx * CN; b++) o[b] = (uint8_t)(w.at(b >> 2) >> (8 * (b & 3)));
    }
}

// ---- launch 1: owner samples and the cell masks ------------------------------------------------
// blend_owner's rule (mcs_blend.h) with the owner's position kept on the way: the slot loop stays
// wave-uniform (scalar loads of the stage parameters), and no second map is evaluated for a slot
// that differs from lane to lane.
struct DmbOwner {
    int slot, x32, y32, cam, w, h;
};

template <int INTERP>
__device__ __forceinline__ DmbOwner dmb_owner(const KParams &P, int x, int y)
{
    DmbOwner best = {kBlendNone, 0, 0, 0, 1, 1}, hint = best;
    int bestd = -1;
    const int hcam = P.seam_hint ? (int)P.seam_hint[(int64_t)(y >> P.seam_shift) * P.seam_w +
                                                    (x >> P.seam_shift)]
                                 : (int)kBlendNone;
    for (int s = 0; s <= P.n_stages; s++) {
        int x32, y32, cam, w, h;
        slot_xy<INTERP>(P, s, x, y, x32, y32, cam, w, h);
        const int d = slot_dist(x32, y32, w, h);
        const DmbOwner here = {s, x32, y32, cam, w, h};
        if (d >= 0 && cam == hcam) hint = here;
        if (d >= 0 && (d > bestd || (d == bestd && cam < best.cam))) {
            best = here;
            bestd = d;
        }
    }
    return hint.slot != kBlendNone ? hint : best;
}

template <int CN, int INTERP, bool GAIN>
__device__ __forceinline__ void direct_mb_own(const KDirectMbArgs &a)
{
    constexpr int kCells = kTileW / kDmbCell;
    __shared__ uint32_t s_cell[kCells];
    const KParams &P = a.P;
    const int lin = threadIdx.y * kWave + threadIdx.x;
    if (lin < kCells) s_cell[lin] = 0;
    __syncthreads();
    const int gx = (P.out_w + kTileW - 1) / kTileW;
    const int tx = (int)blockIdx.x % gx, ty = (int)blockIdx.x / gx;
    const int xg = (tx * kLanesPerRow + (int)threadIdx.x % kLanesPerRow) * kPx;
    const int y = ty * kTileH + (int)threadIdx.y * kRowsPerWave + (int)threadIdx.x / kLanesPerRow;
    const int f0 = blockIdx.y * kDirectFrames;
    const int nf = min(a.n_frames - f0, kDirectFrames);
    if (xg < P.out_w && y < P.out_h) {
        const int npx = min(kPx, P.out_w - xg);
        int x32[kPx], y32[kPx], cam[kPx], w[kPx], h[kPx];
        uint32_t bits = 0, have = 0;
#pragma unroll
        for (int p = 0; p < kPx; p++) {
            const int x = min(xg + p, P.out_w - 1);
            const DmbOwner o = dmb_owner<INTERP>(P, x, y);
            x32[p] = o.x32, y32[p] = o.y32, cam[p] = o.cam, w[p] = o.w, h[p] = o.h;
            if (o.slot != kBlendNone) {
                bits |= 1u << o.slot;
                have |= 1u << p;
            }
        }
        uint8_t *dst = P.out + (int64_t)y * P.out_pitch + (int64_t)xg * CN;
        const bool aligned = (((uintptr_t)dst | (uintptr_t)P.out_fstride) & 3) == 0;
        for (int f = 0; f < nf; f++) {
            DmbWords wd;
#pragma unroll
            for (int p = 0; p < kPx; p++) {
                uint32_t v = 0;
                if ((have >> p) & 1u)
                    v = sample_replicate<CN, GAIN>(
                        P.cams[cam[p]] + (int64_t)(f0 + f) * P.cam_fstride[cam[p]], w[p], h[p],
                        x32[p], y32[p], GAIN ? gain_q_of(P, cam[p]) : 256u);
                dmb_put<CN>(wd, p, v);
            }
            dmb_store<CN>(dst + (int64_t)(f0 + f) * P.out_fstride, wd, npx, aligned);
        }
        if (bits) atomicOr(&s_cell[(xg - tx * kTileW) / kDmbCell], bits);
    }
    __syncthreads();
    if (blockIdx.y == 0 && lin < kCells) {
        const int cx = tx * kCells + lin;
        if (cx < a.cgx && ty < a.cgy) a.cells[(int64_t)ty * a.cgx + cx] = s_cell[lin];
    }
}

// ---- launch 2: the blend tiles -------------------------------------------------------------------
__device__ __forceinline__ int dmb_ix(int c, int o, int n) { return min(max(c - o, 0), n - 1); }

// sum (uy ux) r over the expand taps of (y, x) in the oracle's order (rows outer), / 64; r holds
// doubles as int64 bits at (row * nx + col) * CN + k of an array with origin (ox, oy).
template <int CN>
__device__ __forceinline__ double dmb_expand_d(const int64_t *r, int y, int x, int ox, int oy,
                                               int nx, int ny, int k)
{
    int iy[3], wy[3], ix[3], wx[3];
    exp_taps<true>(y, 0, iy, wy);
    exp_taps<true>(x, 0, ix, wx);
    double acc = 0.0;
#pragma unroll
    for (int u = 0; u < 3; u++)
#pragma unroll
        for (int v = 0; v < 3; v++)
            acc += (double)(wy[u] * wx[v]) *
                   __builtin_bit_cast(double, r[(dmb_ix(iy[u], oy, ny) * nx + dmb_ix(ix[v], ox, nx)) *
                                                    CN + k]);
    return acc / 64.0;
}

// The feather rule of orc_blend.c (feather_px) for the tile's own pixels (dense seams).  A pixel
// with no slot at positive distance keeps what the owner pass wrote (its owner's sample, or 0).
template <int CN, int INTERP, bool GAIN>
__device__ __forceinline__ void dmb_feather(const KParams &P, const MbGeo &G, int f)
{
    for (int i = threadIdx.x; i < kMbTilePx; i += kDmbTileThreads) {
        const int x = G.X0 + i % kBlendTileW, y = G.Y0 + i / kBlendTileW;
        if (x >= G.W || y >= G.H) continue;
        int64_t den = 0, num[CN];
#pragma unroll
        for (int k = 0; k < CN; k++) num[k] = 0;
        for (int s = 0; s <= P.n_stages; s++) {
            int x32, y32, cam, w, h;
            slot_xy<INTERP>(P, s, x, y, x32, y32, cam, w, h);
            const int d = slot_dist(x32, y32, w, h);
            if (d <= 0) continue;
            const uint32_t v = sample_replicate<CN, GAIN>(
                P.cams[cam] + (int64_t)f * P.cam_fstride[cam], w, h, x32, y32,
                GAIN ? gain_q_of(P, cam) : 256u);
            den += d;
#pragma unroll
            for (int k = 0; k < CN; k++) num[k] += (int64_t)d * (int)((v >> (8 * k)) & 0xffu);
        }
        if (den == 0) continue;
        uint8_t *o = P.out + (int64_t)f * P.out_fstride + (int64_t)y * P.out_pitch + (int64_t)x * CN;
#pragma unroll
        for (int k = 0; k < CN; k++) o[k] = (uint8_t)((num[k] + den / 2) / den);
    }
}

template <int CN, int INTERP, bool GAIN>
__device__ __forceinline__ void direct_mb_tile(const KDirectMbArgs &a, uint8_t *smem)
{
    const KParams &P = a.P;
    const int t = blockIdx.x, f = blockIdx.y, tid = threadIdx.x;
    constexpr int nt = kDmbTileThreads;
    const int tx = t % a.gxb, ty = t / a.gxb;
    // owners of the grown neighbourhood [32 tx - 16, 32 tx + 48) x [64 ty - 16, 64 ty + 80), clipped
    constexpr int kCX = kBlendTileW / kDmbCell, kCY = kBlendTileH / kDmbCell;
    const int cx0 = max(kCX * tx - 1, 0), cx1 = min(kCX * tx + kCX, a.cgx - 1);
    const int cy0 = max(kCY * ty - 1, 0), cy1 = min(kCY * ty + kCY, a.cgy - 1);
    uint32_t mask = 0;
    for (int cy = cy0; cy <= cy1; cy++)
        for (int cx = cx0; cx <= cx1; cx++) mask |= a.cells[(int64_t)cy * a.cgx + cx];
    const int ns = __popc(mask);
    if (ns <= 1) return;
    const MbGeo G = mb_geo(P, t);
    if (ns > kBlendSlots) {
        dmb_feather<CN, INTERP, GAIN>(P, G, f);
        return;
    }

    constexpr DmbLds L = dmb_lds(CN);
    constexpr int N1 = kMbN1X * kMbN1Y, N2 = kMbN2X * kMbN2Y, NR = kMbNRX * kMbNRY;
    int64_t *num1 = reinterpret_cast<int64_t *>(smem + L.num1);
    int64_t *num2 = reinterpret_cast<int64_t *>(smem + L.num2);
    uint32_t *g0 = reinterpret_cast<uint32_t *>(smem + L.g0);
    int32_t *g1 = reinterpret_cast<int32_t *>(smem + L.g1);
    int32_t *g2 = reinterpret_cast<int32_t *>(smem + L.g2);
    int32_t *m2 = reinterpret_cast<int32_t *>(smem + L.m2);
    int32_t *den1 = reinterpret_cast<int32_t *>(smem + L.den1);
    int32_t *den2 = reinterpret_cast<int32_t *>(smem + L.den2);
    int32_t *l0 = reinterpret_cast<int32_t *>(smem + L.l0);
    uint16_t *m1 = reinterpret_cast<uint16_t *>(smem + L.m1);
    uint8_t *own = smem + L.own;
    const int RX2 = G.RX + kMbFirst, RY2 = G.RY + kMbFirst;   // level-0 array origin
    const int w5[5] = {1, 4, 6, 4, 1};

    // owner map of the used neighbourhood as local slots (bit rank in mask); the accumulators
    for (int i = tid; i < kMbU; i += nt) {
        const int cx = refl(RX2 + i % kMbUsedX, G.W), cy = refl(RY2 + i / kMbUsedX, G.H);
        const int o = blend_owner<INTERP>(P, cx, cy, nullptr);
        own[i] = (uint8_t)(o != kBlendNone ? __popc(mask & ((1u << o) - 1u)) : kBlendNone);
    }
    for (int i = tid; i < NR * CN; i += nt) num1[i] = 0;
    for (int i = tid; i < N2 * CN; i += nt) num2[i] = 0;
    for (int i = tid; i < NR; i += nt) den1[i] = 0;
    for (int i = tid; i < N2; i += nt) den2[i] = 0;

    for (int j = 0; j < ns; j++) {
        const int s = mb_slot(mask, j);
        // level 0: the owner's replicate-border samples over the used neighbourhood
        for (int i = tid; i < kMbU; i += nt) {
            const int cx = refl(RX2 + i % kMbUsedX, G.W), cy = refl(RY2 + i / kMbUsedX, G.H);
            int x32, y32, cam, w, h;
            slot_xy<INTERP>(P, s, cx, cy, x32, y32, cam, w, h);
            g0[i] = sample_replicate<CN, GAIN>(P.cams[cam] + (int64_t)f * P.cam_fstride[cam], w, h,
                                               x32, y32, GAIN ? gain_q_of(P, cam) : 256u);
        }
        __syncthreads();   // (first round: also the owner map and the zeroed accumulators)
        // g1 = reduce(g0), m1 = reduce(owner == j)
        for (int e = tid; e < N1; e += nt) {
            const int qx = refl(G.X1 + e % kMbN1X, G.w1), qy = refl(G.Y1 + e / kMbN1X, G.h1);
            int acc[CN], macc = 0;
#pragma unroll
            for (int k = 0; k < CN; k++) acc[k] = 0;
#pragma unroll
            for (int u = 0; u < 5; u++) {
                const int row = dmb_ix(2 * qy + u - 2, RY2, kMbUsedY) * kMbUsedX;
#pragma unroll
                for (int v = 0; v < 5; v++) {
                    const int p = row + dmb_ix(2 * qx + v - 2, RX2, kMbUsedX);
                    const int wt = w5[u] * w5[v];
                    const uint32_t px = g0[p];
#pragma unroll
                    for (int k = 0; k < CN; k++) acc[k] += wt * (int)((px >> (8 * k)) & 0xffu);
                    macc += own[p] == j ? wt : 0;
                }
            }
#pragma unroll
            for (int k = 0; k < CN; k++) g1[e * CN + k] = acc[k];
            m1[e] = (uint16_t)macc;
        }
        __syncthreads();
        // g2 = reduce(g1), m2 = reduce(m1); level-2 numerators sum m2 g2 and denominators
        for (int e = tid; e < N2; e += nt) {
            const int zx = refl(G.X2 + e % kMbN2X, G.w2), zy = refl(G.Y2 + e / kMbN2X, G.h2);
            int acc[CN], macc = 0;
#pragma unroll
            for (int k = 0; k < CN; k++) acc[k] = 0;
#pragma unroll
            for (int u = 0; u < 5; u++) {
                const int row = dmb_ix(2 * zy + u - 2, G.Y1, kMbN1Y) * kMbN1X;
#pragma unroll
                for (int v = 0; v < 5; v++) {
                    const int p = row + dmb_ix(2 * zx + v - 2, G.X1, kMbN1X);
                    const int wt = w5[u] * w5[v];
#pragma unroll
                    for (int k = 0; k < CN; k++) acc[k] += wt * g1[p * CN + k];
                    macc += wt * (int)m1[p];
                }
            }
#pragma unroll
            for (int k = 0; k < CN; k++) {
                g2[e * CN + k] = acc[k];
                num2[e * CN + k] += (int64_t)macc * acc[k];
            }
            m2[e] = macc;
            den2[e] += macc;
        }
        // L0 = 16384 g0 - E(g1) of the tile pixels this owner owns
        for (int i = tid; i < kMbTilePx; i += nt) {
            const int lx = i % kBlendTileW, ly = i / kBlendTileW;
            const int x = G.X0 + lx, y = G.Y0 + ly;
            if (x >= G.W || y >= G.H) continue;
            const int p0 = (ly + kBlendHalo - kMbFirst) * kMbUsedX + lx + kBlendHalo - kMbFirst;
            if (own[p0] != j) continue;
            int iy[3], wy[3], ix[3], wx[3];
            exp_taps<true>(y, 0, iy, wy);
            exp_taps<true>(x, 0, ix, wx);
            int e1[CN];
#pragma unroll
            for (int k = 0; k < CN; k++) e1[k] = 0;
#pragma unroll
            for (int u = 0; u < 3; u++)
#pragma unroll
                for (int v = 0; v < 3; v++) {
                    const int p = dmb_ix(iy[u], G.Y1, kMbN1Y) * kMbN1X + dmb_ix(ix[v], G.X1, kMbN1X);
#pragma unroll
                    for (int k = 0; k < CN; k++) e1[k] += wy[u] * wx[v] * g1[p * CN + k];
                }
            const uint32_t px = g0[p0];
#pragma unroll
            for (int k = 0; k < CN; k++)
                l0[i * CN + k] = 16384 * (int)((px >> (8 * k)) & 0xffu) - e1[k];
        }
        __syncthreads();
        // R1 region: numerators sum m1 (16384 g1 - E(g2)) and denominators
        for (int e = tid; e < NR; e += nt) {
            const int ex = e % kMbNRX, ey = e / kMbNRX;
            const int p1 = (ey + kMbRS) * kMbN1X + ex + kMbRS;
            const int m = m1[p1];
            if (m == 0) continue;
            const int qx = refl(G.XR + ex, G.w1), qy = refl(G.YR + ey, G.h1);
            int iy[3], wy[3], ix[3], wx[3];
            exp_taps<true>(qy, 0, iy, wy);
            exp_taps<true>(qx, 0, ix, wx);
            int64_t e2[CN];
#pragma unroll
            for (int k = 0; k < CN; k++) e2[k] = 0;
#pragma unroll
            for (int u = 0; u < 3; u++)
#pragma unroll
                for (int v = 0; v < 3; v++) {
                    const int p = dmb_ix(iy[u], G.Y2, kMbN2Y) * kMbN2X + dmb_ix(ix[v], G.X2, kMbN2X);
#pragma unroll
                    for (int k = 0; k < CN; k++)
                        e2[k] += (int64_t)(wy[u] * wx[v]) * g2[p * CN + k];
                }
#pragma unroll
            for (int k = 0; k < CN; k++)
                num1[e * CN + k] += (int64_t)m * (16384 * (int64_t)g1[p1 * CN + k] - e2[k]);
            den1[e] += m;
        }
        __syncthreads();   // the next owner overwrites g0, g1, g2, m1
    }

    // B2 = sum m2 g2 / (sum m2 * 65536), in place of its numerators
    for (int i = tid; i < N2 * CN; i += nt) {
        const int den = den2[i / CN];
        const double b2 = den ? (double)num2[i] / ((double)den * 65536.0) : 0.0;
        num2[i] = __builtin_bit_cast(int64_t, b2);
    }
    __syncthreads();
    // R1 = B1 + up(B2), in place of the level-1 numerators
    for (int e = tid; e < NR; e += nt) {
        const int qx = refl(G.XR + e % kMbNRX, G.w1), qy = refl(G.YR + e / kMbNRX, G.h1);
        const int den = den1[e];
#pragma unroll
        for (int k = 0; k < CN; k++) {
            const double b1 = den ? (double)num1[e * CN + k] / ((double)den * 4194304.0) : 0.0;
            const double r1 = b1 + dmb_expand_d<CN>(num2, qy, qx, G.X2, G.Y2, kMbN2X, kMbN2Y, k);
            num1[e * CN + k] = __builtin_bit_cast(int64_t, r1);
        }
    }
    __syncthreads();
    // R0 = L0 / 16384 + up(R1) and the bytes, 4 pixels of a row per lane; a pixel no camera
    // covers is 0, as the owner pass wrote it
    uint8_t *out = P.out + (int64_t)f * P.out_fstride;
    for (int g = tid; g < kMbTilePx / kPx; g += nt) {
        const int lx = (g % (kBlendTileW / kPx)) * kPx, ly = g / (kBlendTileW / kPx);
        const int x0 = G.X0 + lx, y = G.Y0 + ly;
        if (x0 >= G.W || y >= G.H) continue;
        const int npx = min(kPx, G.W - x0);
        DmbWords wd;
#pragma unroll
        for (int p = 0; p < kPx; p++) {
            uint32_t px = 0;
            const int p0 = (ly + kBlendHalo - kMbFirst) * kMbUsedX + lx + p + kBlendHalo - kMbFirst;
            if (p < npx && own[p0] != kBlendNone) {
#pragma unroll
                for (int k = 0; k < CN; k++) {
                    const double r0 = (double)l0[(ly * kBlendTileW + lx + p) * CN + k] / 16384.0 +
                                      dmb_expand_d<CN>(num1, y, x0 + p, G.XR, G.YR, kMbNRX, kMbNRY, k);
                    const double v = floor(r0 + 0.5);
                    px |= (uint32_t)(v < 0.0 ? 0.0 : (v > 255.0 ? 255.0 : v)) << (8 * k);
                }
            }
            dmb_put<CN>(wd, p, px);
        }
        uint8_t *o = out + (int64_t)y * P.out_pitch + (int64_t)x0 * CN;
        dmb_store<CN>(o, wd, npx, ((uintptr_t)o & 3) == 0);
    }
}

}  // namespace mcs

// ---------------------------------------------------------------------------------------------
// Entry points (looked up by mcs_prepare.cpp kernels).  own: block (64, 8), grid (tiles of
// the direct path, ceil(frames / kDirectFrames)); tile: block kDmbTileThreads, grid (blend tiles,
// frames), dmb_lds(CN).bytes of dynamic LDS.  The _g twins: the camera gains on the taps.
#define MCS_DMB_ENTRY(CN, IN, GS, GAIN)                                                        \
    extern "C" __global__ __launch_bounds__(512) void mcs_direct_mb_own_c##CN##_i##IN##GS(     \
        const mcs::KDirectMbArgs a)                                                            \
    {                                                                                          \
        mcs::direct_mb_own<CN, IN, GAIN>(a);                                                   \
    }                                                                                          \
    extern "C" __global__ __launch_bounds__(mcs::kDmbTileThreads) void                         \
        mcs_direct_mb_tile_c##CN##_i##IN##GS(const mcs::KDirectMbArgs a)                       \
    {                                                                                          \
        extern __shared__ __attribute__((aligned(16))) uint8_t smem[];                         \
        mcs::direct_mb_tile<CN, IN, GAIN>(a, smem);                                            \
    }
#define MCS_DMB_ENTRIES(CN)                                                                    \
    MCS_DMB_ENTRY(CN, 0, , false)                                                              \
    MCS_DMB_ENTRY(CN, 1, , false)                                                              \
    MCS_DMB_ENTRY(CN, 0, _g, true)                                                             \
    MCS_DMB_ENTRY(CN, 1, _g, true)
MCS_DMB_ENTRIES(1)
MCS_DMB_ENTRIES(2)
MCS_DMB_ENTRIES(3)
MCS_DMB_ENTRIES(4)
