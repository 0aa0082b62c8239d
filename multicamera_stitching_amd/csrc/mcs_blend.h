// mcs_blend.h -- device code of the blended stitch modes,
// included by mcs_kernels.hip (one code object).  The arithmetic is specified, and restated on
// the CPU, in oracle/orc_blend.c; this code reproduces it bit for bit (integers and IEEE
// doubles in the same order, no contraction).
// This file: seam sampling, owner / classify, feather, and what the multi-band kernels and the
// sweep module (mcs_sweep.hip) share.  The multi-band kernel families have a header each:
// mcs_mb_prep.h, mcs_mb_levels.h, mcs_mb_bands.h, mcs_mb_blend.h.
//
// Layout: the stitch kernels first write every pixel from its "owner" camera (the covering
// camera farthest from its own image edge); then only the tiles where blending changes pixels
// are recomputed here, 32 x 32 output pixels per block:
//   feather   -- tiles with a pixel covered by two cameras at positive edge distance;
//   multiband -- tiles whose neighbourhood (the 3-level pyramid's reach, 16 px halo)
//                holds two owners (the seam band).  Per tile: the owners' warped images over the
//                neighbourhood (replicate border) -> integer Gaussian/Laplacian pyramids in LDS
//                -> mask-weighted blend per level (double) -> collapse -> bytes.
// Both are a few percent of the mosaic's tiles for a linear rig.
#pragma once

namespace mcs {

// Camera slot s of the plan: 0 = camera 0 (integer offset, or its lens), j+1 = stage j's camera.
template <int INTERP>
__device__ __forceinline__ void slot_xy(const KParams &P, int s, int x, int y, int &x32, int &y32,
                                        int &cam, int &w, int &h)
{
    int X, Y;
    if (s == 0) {
        cam = 0;
        w = P.cam0_w;
        h = P.cam0_h;
        if (!cam0_lensed(P)) {
            x32 = (x + P.cam0_offx) * 32;
            y32 = (y + P.cam0_offy) * 32;
            return;
        }
        cam0_lens_map<INTERP>(P, x, y, X, Y);
    } else {
        const KStage &S = P.st[s - 1];
        cam = S.cam;
        w = S.src_w;
        h = S.src_h;
        stage_map<INTERP>(P, S, x, y, X, Y);
    }
    if (INTERP == MCS_INTER_NEAREST) {
        x32 = sat_i16(X) * 32;
        y32 = sat_i16(Y) * 32;
    } else {
        x32 = sat_i16(X >> 5) * 32 + (X & 31);
        y32 = sat_i16(Y >> 5) * 32 + (Y & 31);
    }
}

// Distance to the image edge in 1/32 px, -1 when the position is not covered.
__device__ __forceinline__ int slot_dist(int x32, int y32, int w, int h)
{
    const int xm = 32 * (w - 1) - x32, ym = 32 * (h - 1) - y32;
    if (x32 < 0 || y32 < 0 || xm < 0 || ym < 0) return -1;
    return min(min(x32, y32), min(xm, ym));
}

// Owner slot of output pixel (x, y) (largest edge distance, ties to the lower camera index),
// kBlendNone when no camera covers it.  *pos_mask: slots covering it at positive distance.
template <int INTERP>
__device__ __forceinline__ int blend_owner(const KParams &P, int x, int y, uint32_t *pos_mask)
{
    int best = kBlendNone, bestd = -1, bestcam = 0;
    // graph-cut seams: the label's camera owns the pixel when it covers it
    const int hcam = P.seam_hint ? (int)P.seam_hint[(int64_t)(y >> P.seam_shift) * P.seam_w +
                                                    (x >> P.seam_shift)]
                                 : (int)kBlendNone;
    int hslot = -1;
    uint32_t pm = 0;
    for (int s = 0; s <= P.n_stages; s++) {
        int x32, y32, cam, w, h;
        slot_xy<INTERP>(P, s, x, y, x32, y32, cam, w, h);
        const int d = slot_dist(x32, y32, w, h);
        if (d > 0) pm |= 1u << s;
        if (d >= 0 && cam == hcam) hslot = s;
        if (d >= 0 && (d > bestd || (d == bestd && cam < bestcam))) {
            best = s;
            bestd = d;
            bestcam = cam;
        }
    }
    if (pos_mask) *pos_mask = pm;
    return hslot >= 0 ? hslot : best;
}

// Bilinear sample at (x32, y32) with the taps clamped into the image (BORDER_REPLICATE), the
// remapBilinear fixed point; channel k in byte k.  One 8-byte window load per tap row.  GAIN (the
// _g feather kernel): gain q on every tap byte first (gain_byte).
template <int CN, bool GAIN = false>
__device__ __forceinline__ uint32_t sample_replicate(const uint8_t *fb, int w, int h, int x32,
                                                     int y32, uint32_t q = 256u)
{
    const int sx = x32 >> 5, sy = y32 >> 5, fx = x32 & 31, fy = y32 & 31;
    const int cx = w >= 2 ? min(max(sx, 0), w - 2) : 0;
    const int oa = (min(max(sx, 0), w - 1) - cx) * CN, ob = (min(max(sx + 1, 0), w - 1) - cx) * CN;
    const int ya = min(max(sy, 0), h - 1), yb = min(max(sy + 1, 0), h - 1);
    const int w00 = (32 - fx) * (32 - fy) * 32, w01 = fx * (32 - fy) * 32;
    const int w10 = (32 - fx) * fy * 32, w11 = fx * fy * 32;
    const int64_t pitch = (int64_t)w * CN, fbytes = pitch * h;
    const uint2 r0 = load8<2 * CN>(fb, ya * pitch + (int64_t)cx * CN, fbytes);
    const uint2 r1 = load8<2 * CN>(fb, yb * pitch + (int64_t)cx * CN, fbytes);
    uint32_t r = 0;
#pragma unroll
    for (int k = 0; k < CN; k++) {
        uint32_t p00 = byte_of(r0, oa + k), p01 = byte_of(r0, ob + k);
        uint32_t p10 = byte_of(r1, oa + k), p11 = byte_of(r1, ob + k);
        if constexpr (GAIN) {
            p00 = gain_byte(p00, q), p01 = gain_byte(p01, q);
            p10 = gain_byte(p10, q), p11 = gain_byte(p11, q);
        }
        const int s = (int)p00 * w00 + (int)p01 * w01 + (int)p10 * w10 + (int)p11 * w11;
        r |= (uint32_t)((s + 16384) >> 15) << (8 * k);
    }
    return r;
}

// Camera, size of slot s (uniform).
__device__ __forceinline__ void slot_info(const KParams &P, int s, int &cam, int &w, int &h)
{
    cam = s == 0 ? 0 : P.st[s - 1].cam;
    w = s == 0 ? P.cam0_w : P.st[s - 1].src_w;
    h = s == 0 ? P.cam0_h : P.st[s - 1].src_h;
}

__device__ __forceinline__ int refl(int i, int n)
{
    if (n == 1) return 0;
    while (i < 0 || i >= n) {
        if (i < 0) i = -i;
        if (i >= n) i = 2 * n - 2 - i;
    }
    return i;
}

// ---- seam finder inputs (mcs_plan_find_seams) ------------------------------------------------
// One thread per point of the 2^k grid (P.seam_hint must be NULL: the distance owner).
template <int CN, int INTERP>
__device__ __forceinline__ void seam_sample(const KSeamArgs &a)
{
    const KParams &P = a.P;
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= a.gw * a.gh) return;
    const int x = (q % a.gw) << a.k, y = (q / a.gw) << a.k;
    const int64_t np = (int64_t)a.gw * a.gh;
    const int o = blend_owner<INTERP>(P, x, y, nullptr);
    uint32_t cov = 0;
    for (int s = 0; s <= P.n_stages; s++) {
        int x32, y32, cam, w, h;
        slot_xy<INTERP>(P, s, x, y, x32, y32, cam, w, h);
        if (slot_dist(x32, y32, w, h) < 0) continue;
        cov |= 1u << cam;
        const uint8_t *fb = P.cams[cam];
        const uint32_t v = sample_replicate<CN>(fb, w, h, x32, y32);
        uint8_t *d = a.samples + ((int64_t)cam * np + q) * CN;
#pragma unroll
        for (int k = 0; k < CN; k++) d[k] = (uint8_t)(v >> (8 * k));
    }
    a.cov[q] = (uint16_t)cov;
    int ocam = kBlendNone;
    if (o != kBlendNone) {
        int c, w, h;
        slot_info(P, o, c, w, h);
        ocam = c;
    }
    a.label[q] = (uint8_t)ocam;
}

// ---- prepare (once per plan) -----------------------------------------------------------------
// grid (ceil(W / 32), ceil(H / 32)), block 256: owner map, and per blend tile the owners it holds
// (info[2t]) and the slots covering any of its pixels at positive distance when two do
// (info[2t+1], the feather set).
template <int INTERP>
__device__ __forceinline__ void blend_owner_tile(const KParams &P, uint8_t *owner_map,
                                                 uint32_t *info)
{
    __shared__ uint32_t s_own, s_feather;
    if (threadIdx.x == 0) s_own = s_feather = 0;
    __syncthreads();
    const int X0 = blockIdx.x * kBlendTileW, Y0 = blockIdx.y * kBlendTileH;
    uint32_t own = 0, fea = 0;
    for (int i = threadIdx.x; i < kMbTilePx; i += blockDim.x) {
        const int x = X0 + (i % kBlendTileW), y = Y0 + i / kBlendTileW;
        if (x >= P.out_w || y >= P.out_h) continue;
        uint32_t pm;
        const int o = blend_owner<INTERP>(P, x, y, &pm);
        owner_map[(int64_t)y * P.out_w + x] = (uint8_t)o;
        if (o != kBlendNone) own |= 1u << o;
        if (__popc(pm) >= 2) fea |= pm;
    }
    atomicOr(&s_own, own);
    atomicOr(&s_feather, fea);
    __syncthreads();
    if (threadIdx.x == 0) {
        const int t = blockIdx.y * gridDim.x + blockIdx.x;
        info[2 * t] = s_own;
        info[2 * t + 1] = s_feather;
    }
}

// grid (tiles), block 256: appends (tile, slot mask) to list[1 + 2i] for the tiles the mode
// recomputes; list[0] = count.  multiband: the owners in the tile's neighbourhood (the tile grown
// by kBlendHalo, clipped to the mosaic: reflected positions land inside it), when there are two
// or more.  A neighbourhood with more than kBlendSlots owners (more than the blend kernels hold)
// degrades its tile to the feather rule (orc_blend.c "dense seams"): the tile goes to list2 with
// its feather slot set (none when no pixel has two cameras at positive distance: the owner
// sample the streaming kernel writes IS the feather value there), counted in overflow[0];
// overflow[1] = the most owners any multi-band-listed tile has.
__device__ __forceinline__ void blend_classify(const KParams &P, int mode, const uint8_t *owner,
                                               const uint32_t *info, int *list, int *overflow,
                                               int *list2)
{
    __shared__ uint32_t s_mask;
    const int gx = (P.out_w + kBlendTileW - 1) / kBlendTileW;
    const int t = blockIdx.x, tx = t % gx, ty = t / gx;
    uint32_t mask;
    if (mode == MCS_BLEND_FEATHER) {
        mask = info[2 * t + 1];
    } else {
        if (threadIdx.x == 0) s_mask = 0;
        __syncthreads();
        const int x0 = max(tx * kBlendTileW - kBlendHalo, 0);
        const int x1 = min(tx * kBlendTileW + kBlendTileW + kBlendHalo, P.out_w);
        const int y0 = max(ty * kBlendTileH - kBlendHalo, 0);
        const int y1 = min(ty * kBlendTileH + kBlendTileH + kBlendHalo, P.out_h);
        const int rw = x1 - x0, n = rw * (y1 - y0);
        uint32_t m = 0;
        for (int i = threadIdx.x; i < n; i += blockDim.x) {
            const int o = owner[(int64_t)(y0 + i / rw) * P.out_w + x0 + i % rw];
            if (o != kBlendNone) m |= 1u << o;
        }
        atomicOr(&s_mask, m);
        __syncthreads();
        mask = s_mask;
        if (__popc(mask) < 2) mask = 0;
    }
    if (threadIdx.x == 0 && mode == MCS_BLEND_MULTIBAND && __popc(mask) > kBlendSlots) {
        atomicAdd(overflow, 1);
        const uint32_t fea = info[2 * t + 1];
        if (fea) {
            const int i = atomicAdd(&list2[0], 1);
            list2[1 + 2 * i] = t;
            list2[2 + 2 * i] = (int)fea;
        }
        return;
    }
    if (threadIdx.x == 0 && mask) {
        atomicMax(overflow + 1, __popc(mask));
        const int i = atomicAdd(&list[0], 1);
        list[1 + 2 * i] = t;
        list[2 + 2 * i] = (int)mask;
    }
}

// ---- per frame ---------------------------------------------------------------------------------
// Feather: grid (listed tiles, frames), block 256.
template <int CN, int INTERP, bool GAIN = false>
__device__ __forceinline__ void feather_tile(const KBlendArgs &a)
{
    const KParams &P = a.P;
    const int gx = (P.out_w + kBlendTileW - 1) / kBlendTileW;
    const int t = a.list[1 + 2 * blockIdx.x];
    const uint32_t mask = (uint32_t)a.list[2 + 2 * blockIdx.x];
    const int X0 = (t % gx) * kBlendTileW, Y0 = (t / gx) * kBlendTileH, f = blockIdx.y;
    for (int i = threadIdx.x; i < kMbTilePx; i += blockDim.x) {
        const int x = X0 + (i % kBlendTileW), y = Y0 + i / kBlendTileW;
        if (x >= P.out_w || y >= P.out_h) continue;
        int den = 0, num[CN];
#pragma unroll
        for (int k = 0; k < CN; k++) num[k] = 0;
        for (uint32_t m = mask; m; m &= m - 1) {
            const int s = __ffs(m) - 1;
            int x32, y32, cam, w, h;
            slot_xy<INTERP>(P, s, x, y, x32, y32, cam, w, h);
            const int d = slot_dist(x32, y32, w, h);
            if (d <= 0) continue;
            const uint32_t v = sample_replicate<CN, GAIN>(
                P.cams[cam] + (int64_t)f * P.cam_fstride[cam], w, h, x32, y32,
                GAIN ? gain_q_of(P, cam) : 256u);
            den += d;
#pragma unroll
            for (int k = 0; k < CN; k++) num[k] += d * (int)((v >> (8 * k)) & 0xffu);
        }
        if (den == 0) continue;   // the stitch kernel already wrote the owner's sample
        uint8_t *o = P.out + (int64_t)f * P.out_fstride + (int64_t)y * P.out_pitch + x * CN;
#pragma unroll
        for (int k = 0; k < CN; k++) o[k] = (uint8_t)((num[k] + den / 2) / den);
    }
}

// ---- multi-band (3 levels) -------------------------------------------------------------------
// Per listed tile (a 32 x 32 output tile whose 64 x 64 neighbourhood holds two or more owners)
// the pyramid needs, per owner slot: level 0 over [X0-14, X0+42] (57 of the 64 px), level 1
// g1 over [X0/2-6, X0/2+20] (27), level 2 g2 over [X0/4-2, X0/4+9] (12), and the collapsed
// level 1 R1 over [X0/2-1, X0/2+16] (18, "the R1 region").  Entries at coordinates outside the
// mosaic hold the reflected coordinate's value, so reflected lookups land in range.  Three
// kernels, all with small LDS footprints (many blocks per CU) and no FP64 map in the capture
// loop:
//   mcs_mb_prep_c*_i*   once per plan: per (tile, owner) the source window + folded bilinear
//                       weights of every level-0 sample (mb_desc), and per tile the seam masks
//                       m1 (R1 region), m2, and their sums over the owners (the denominators),
//                       the blend's work lists and their records (mcs_kparams.h);
//   mcs_mb_levels_c*    per (tile, owner, 4 captures): samples -> level 0 (LDS) -> separable
//                       5-tap reduces -> g1 (R1 region, u16) and g2 to a scratch buffer;
//   mcs_mb_blend_c*     per (tile, capture): B2, R1 = B1 + up(B2), R0 = L0_owner + up(R1) over
//                       the tile's pixels; level 0 of the owner is the owner sample the stitch
//                       kernel already wrote (equal to the replicate-border sample wherever the
//                       owner covers the pixel, which it always does).
// Long launches run in chunks of captures so the scratch stays a few tens of MB.
constexpr int kMbO1 = 6, kMbO2 = 2, kMbOR = 1;       // array origins: O/2 - 6, O/4 - 2, O/2 - 1
constexpr int kMbU = kMbUsedX * kMbUsedY;             // level-0 samples per owner
constexpr int kMbFoot = 28672;      // bytes of one LDS footprint buffer
constexpr int kMbFootBufs = 1;      // 2: double buffer, 1: refilled during the reduces
constexpr int kMbRS = kMbO1 - kMbOR;                  // R1 region origin in the level-1 array (5)
// Level scratch of one (tile, owner, capture), row-major (a band's lanes, adjacent columns,
// store contiguous bytes): g1 (R1 region, 8 B entries) at row * kMbNRX + col, g2 with the
// channels of an entry together at (row * kMbN2X + col) * CN + channel.
__device__ __forceinline__ int mb_g1_at(int col, int row) { return row * kMbNRX + col; }
template <int CN>
__device__ __forceinline__ int mb_g2_at(int col, int row, int k)
{
    return (row * kMbN2X + col) * CN + k;
}

// Expand taps of fine index x into a coarse level of size n (IN: no reflection needed).
template <bool IN>
__device__ __forceinline__ void exp_taps(int x, int n, int *idx, int *wt)
{
    if ((x & 1) == 0) {
        idx[0] = IN ? x / 2 - 1 : refl(x / 2 - 1, n), wt[0] = 1;
        idx[1] = IN ? x / 2 : refl(x / 2, n), wt[1] = 6;
        idx[2] = IN ? x / 2 + 1 : refl(x / 2 + 1, n), wt[2] = 1;
        return;
    }
    idx[0] = IN ? (x - 1) / 2 : refl((x - 1) / 2, n), wt[0] = 4;
    idx[1] = IN ? (x + 1) / 2 : refl((x + 1) / 2, n), wt[1] = 4;
    idx[2] = idx[1], wt[2] = 0;   // padding tap: adds an exact 0, keeps the trip count fixed
}

// Parity class of a fine position's expand taps: bit 0 = odd column (2 taps), bit 1 = odd row.
// (Reflection at the level's borders keeps parity: refl(-i) = i, refl(n - 1 + i) = n - 1 - i.)
__device__ __forceinline__ int mb_cls(int x, int y) { return (x & 1) | ((y & 1) << 1); }

// Geometry of one multi-band tile: level sizes and the origins of the arrays held per level.
struct MbGeo {
    int W, H, w1, h1, w2, h2;
    int X0, Y0, RX, RY, X1, Y1, X2, Y2, XR, YR;
    bool interior;
};

__device__ __forceinline__ MbGeo mb_geo(const KParams &P, int t)
{
    MbGeo G;
    G.W = P.out_w;
    G.H = P.out_h;
    G.w1 = (G.W + 1) / 2, G.h1 = (G.H + 1) / 2, G.w2 = (G.w1 + 1) / 2, G.h2 = (G.h1 + 1) / 2;
    const int gx = (G.W + kBlendTileW - 1) / kBlendTileW;
    G.X0 = (t % gx) * kBlendTileW, G.Y0 = (t / gx) * kBlendTileH;
    G.RX = G.X0 - kBlendHalo, G.RY = G.Y0 - kBlendHalo;         // level-0 origin
    G.X1 = G.X0 / 2 - kMbO1, G.Y1 = G.Y0 / 2 - kMbO1;             // level-1 origin
    G.X2 = G.X0 / 4 - kMbO2, G.Y2 = G.Y0 / 4 - kMbO2;             // level-2 origin
    G.XR = G.X0 / 2 - kMbOR, G.YR = G.Y0 / 2 - kMbOR;             // R1 origin
    G.interior = G.RX >= 0 && G.RY >= 0 && G.RX + kBlendTileW + 2 * kBlendHalo <= G.W &&
                 G.RY + kBlendTileH + 2 * kBlendHalo <= G.H;
    return G;
}

// Level coordinate -> reflected coordinate.  IN (interior tile): every coordinate the tile
// touches lies inside its level, so the reflection is the identity and index arithmetic folds.
template <bool IN>
__device__ __forceinline__ int rf(int i, int n) { return IN ? i : refl(i, n); }
template <bool IN>
__device__ __forceinline__ int ix2(int c, int o, int n)
{
    return IN ? c - o : min(max(c - o, 0), n - 1);
}

// Replicate-border bilinear sample of slot s at output (x, y) (sample_replicate): tap rows ya,
// yb, the window's first pixel c, meta = fx' | fy << 6, where fx' is the horizontal fraction
// with the replicate border folded in: both taps on the window's pixel 0 -> 0, both on pixel 1
// -> 32 (the weights then sum onto one pixel, as the clamped taps do).
struct MbSrc {
    int ya, yb, c;
    uint32_t meta;
};

template <int INTERP>
__device__ __forceinline__ MbSrc mb_src(const KParams &P, int s, int x, int y)
{
    int x32, y32, cam, w, h;
    slot_xy<INTERP>(P, s, x, y, x32, y32, cam, w, h);
    const int sx = x32 >> 5, sy = y32 >> 5;
    MbSrc r;
    r.c = w >= 2 ? min(max(sx, 0), w - 2) : 0;
    const bool a_hi = min(max(sx, 0), w - 1) > r.c;       // left tap on pixel 1
    const bool b_hi = min(max(sx + 1, 0), w - 1) > r.c;   // right tap on pixel 1
    const uint32_t fx = a_hi ? 32u : (b_hi ? (uint32_t)(x32 & 31) : 0u);
    r.ya = min(max(sy, 0), h - 1);
    r.yb = min(max(sy + 1, 0), h - 1);
    r.meta = fx | ((uint32_t)(y32 & 31) << 6);
    return r;
}

// Global-memory window descriptor of a sample (frame of w x h x CN): .x = byte offset of tap row
// a in the frame (bit 31: tap row b is the next row, else the same row); .y = meta | d << 12,
// where d = bytes both windows start earlier so that row b's window ends inside the frame (the
// taps then sit at bytes d and d + CN).  Every capture's load is then unconditional.  Frames
// with (h - 1) * w * CN < 16 bytes take load8's guarded path instead.
// Bits 15..18 of .y: the band pass's dword-aligned form (mb_bands<.., AL>): both tap rows read as
// 12-byte windows starting sh bytes before tap a, at a 4-byte boundary (sh <= 12 - 2 CN: the
// taps' 2 CN bytes inside the window; chosen so that row b's window ends inside the frame);
// 15 = no such window.  Valid wherever the host enables
// that form (band_aligned: pitch and frame bytes multiples of 4, frames of >= pitch + 12 bytes).
template <int CN>
__device__ __forceinline__ uint2 mb_desc(const MbSrc &q, int w, int h)
{
    const int64_t pitch = (int64_t)w * CN, fbytes = pitch * h;
    const int64_t oa = q.ya * pitch + (int64_t)q.c * CN, ob = oa + (q.yb > q.ya ? pitch : 0);
    const uint32_t d = (uint32_t)min(max(ob + 8 - fbytes, (int64_t)0), (int64_t)7);
    const int64_t e = fbytes - (ob - oa) - 12;   // last start of row a's window
    int64_t o4 = oa & ~(int64_t)3;
    if (o4 > e) o4 = e & ~(int64_t)3;
    const uint32_t sh = (e >= 0 && oa - o4 <= 12 - 2 * CN) ? (uint32_t)(oa - o4) : 15u;
    return make_uint2((uint32_t)oa | (q.yb > q.ya ? 0x80000000u : 0u),
                      q.meta | (d << 12) | (sh << 15));
}

// The 8 bytes starting sh (<= 10) bytes into a 12-byte window, zero past its end (v_alignbyte
// funnel shifts).
// 6 a + b for packed u16 pairs whose product does not fit 24 bits, as two full-rate shift-adds
// (the compiler otherwise emits the multiply as a v_mad_u64_u32)
__device__ __forceinline__ uint32_t mad6_u32(uint32_t a, uint32_t b)
{
    uint32_t t, r;
    asm("v_lshl_add_u32 %0, %1, 1, %2" : "=v"(t) : "v"(a), "v"(b));
    asm("v_lshl_add_u32 %0, %1, 2, %2" : "=v"(r) : "v"(a), "v"(t));
    return r;
}

// The LDS-ring window (mb_bands_body mode 2): 4-byte aligned in the ring, byte shift sh < 4, so
// the 8 bytes are two alignbytes (no third dword's select as in mb_win_shift).
__device__ __forceinline__ uint2 mb_win_shift4(uint3 v, uint32_t sh)
{
    return make_uint2(__builtin_amdgcn_alignbyte(v.y, v.x, sh & 3u),
                      __builtin_amdgcn_alignbyte(v.z, v.y, sh & 3u));
}

template <int CN>
__device__ __forceinline__ uint2 mb_win_shift(uint3 v, uint32_t sh)
{
    const uint32_t s = sh & 3u;
    const uint32_t a = __builtin_amdgcn_alignbyte(v.y, v.x, s);
    const uint32_t b = __builtin_amdgcn_alignbyte(v.z, v.y, s);
    const uint32_t c = __builtin_amdgcn_alignbyte(0u, v.z, s);
    if (CN <= 2 && (sh & 8u)) return make_uint2(c, 0u);   // (sh > 6 only for 1 or 2 channels)
    return (sh & 4u) ? make_uint2(b, c) : make_uint2(a, b);
}

// Source footprint of one (tile, owner) staged in LDS per capture (mb_levels): rows
// [rmin, rmin + rows), bytes [cal, cal + stride) of each (cal 16-byte aligned, stride a multiple
// of 16), rows `stride` bytes apart in LDS.  The frame's last row is fetched `e` bytes earlier so
// that no 16-byte chunk crosses the frame end.  A sample's LDS descriptor: .x = LDS offsets of
// its two tap-row windows (16 bits each), .y = meta.
struct MbFoot {
    int rmin, rows, cal, stride, e, fits, pad0, pad1;
};

__device__ __forceinline__ uint32_t mb_foot_off(const MbFoot &F, int row, int byte, int h)
{
    return (uint32_t)((row - F.rmin) * F.stride + byte - F.cal + (row == h - 1 ? F.e : 0));
}

// The descriptor's 15-bit weights as u16 pairs on the window's pixels 0 / 1, row a and row b:
// (32 - fx', fx') * 32 (32 - fy) and * 32 fy (each lane <= 32768: no carry between lanes), so
// that mb_tap() gives sample_replicate's (sum p w + 2^14) >> 15 exactly.
__device__ __forceinline__ void mb_weights(uint32_t meta, uint32_t &wa, uint32_t &wb)
{
    const uint32_t fx = meta & 63u, fy = (meta >> 6) & 31u;
    const uint32_t wx = (32u - fx) | (fx << 16);
    wa = wx * ((32u - fy) << 5);
    wb = wx * (fy << 5);
}

// mb_weights with every weight doubled, min(2 w, 65535) (the stitch kernels' w2x): a channel's
// mb_tap2 sum then carries mb_tap's (sum p w + 2^14) >> 15 in its byte 2 -- s = 2 sum p w + 2^15
// < 2^24; the one weight 2 w = 65536 (fx' = 0 or 32 with fy = 0: all on one pixel) clamps to
// 65535, and 65535 p + 2^15 still has p in byte 2 -- so the band pass packs channels with one
// v_perm instead of shifting, masking and or-ing each.
__device__ __forceinline__ void mb_weights2(uint32_t meta, uint32_t &wa, uint32_t &wb)
{
    const uint32_t fx = meta & 63u, fy = (meta >> 6) & 31u;
    const uint32_t ya = (32u - fy) << 6, yb = fy << 6;
    wa = min((32u - fx) * ya, 65535u) | (min(fx * ya, 65535u) << 16);
    wb = min((32u - fx) * yb, 65535u) | (min(fx * yb, 65535u) << 16);
}

// Channel k of a descriptor's sample from its two (shifted) row windows.  GAIN (the _g kernels):
// the owner camera's gain g on the two tap bytes of each row first (gain_half).
template <int CN, bool GAIN = false>
__device__ __forceinline__ uint32_t mb_tap(uint2 r0, uint2 r1, uint32_t wa, uint32_t wb, int k,
                                           uint32_t d, GainQ g = GainQ())
{
    typedef unsigned short us2 __attribute__((ext_vector_type(2)));
    const uint32_t sel = ((uint32_t)k | (0x0cu << 8) | ((uint32_t)(CN + k) << 16) | (0x0cu << 24)) +
                         d * 0x00010001u;
    uint32_t a0 = __builtin_amdgcn_perm(r0.y, r0.x, sel);
    uint32_t a1 = __builtin_amdgcn_perm(r1.y, r1.x, sel);
    if constexpr (GAIN) {
        a0 = gain_half(a0, g.h, g.l);
        a1 = gain_half(a1, g.h, g.l);
    }
    uint32_t v = __builtin_amdgcn_udot2(__builtin_bit_cast(us2, a0), __builtin_bit_cast(us2, wa),
                                        16384u, false);
    v = __builtin_amdgcn_udot2(__builtin_bit_cast(us2, a1), __builtin_bit_cast(us2, wb), v, false);
    return v >> 15;
}

// Channel k of a sample with mb_weights2's doubled weights: the value is byte 2 of the result.
template <int CN, bool GAIN = false>
__device__ __forceinline__ uint32_t mb_tap2(uint2 r0, uint2 r1, uint32_t wa, uint32_t wb, int k,
                                            uint32_t d, GainQ g = GainQ())
{
    typedef unsigned short us2 __attribute__((ext_vector_type(2)));
    const uint32_t sel = ((uint32_t)k | (0x0cu << 8) | ((uint32_t)(CN + k) << 16) | (0x0cu << 24)) +
                         d * 0x00010001u;
    uint32_t a0 = __builtin_amdgcn_perm(r0.y, r0.x, sel);
    uint32_t a1 = __builtin_amdgcn_perm(r1.y, r1.x, sel);
    if constexpr (GAIN) {
        a0 = gain_half(a0, g.h, g.l);
        a1 = gain_half(a1, g.h, g.l);
    }
    const uint32_t v = __builtin_amdgcn_udot2(__builtin_bit_cast(us2, a0),
                                              __builtin_bit_cast(us2, wa), 32768u, false);
    return __builtin_amdgcn_udot2(__builtin_bit_cast(us2, a1), __builtin_bit_cast(us2, wb), v,
                                  false);
}

// Makes a register array opaque to the optimiser (one asm per capture): values derived from it
// are then recomputed per capture instead of being hoisted out of the capture loop and held.
template <int N>
__device__ __forceinline__ void mb_opaque(uint32_t (&v)[N])
{
#pragma unroll
    for (int i = 0; i < N; i += 4) {
        if (i + 3 < N) asm volatile("" : "+v"(v[i]), "+v"(v[i + 1]), "+v"(v[i + 2]), "+v"(v[i + 3]));
        else if (i + 2 < N) asm volatile("" : "+v"(v[i]), "+v"(v[i + 1]), "+v"(v[i + 2]));
        else if (i + 1 < N) asm volatile("" : "+v"(v[i]), "+v"(v[i + 1]));
        else asm volatile("" : "+v"(v[i]));
    }
}

// e / D for 0 <= e < 2^16 / D (multiply-shift, exact in that range: D = 12, 18 here)
template <int D>
__device__ __forceinline__ int div_small(int e)
{
    return (int)(__umul24((unsigned)e, (65536u + D - 1) / D) >> 16);
}

// Sample e of a tile's compacted level-0 columns [a0, a0 + w0) -> its 57 x 57 array index.
__device__ __forceinline__ int mb_sample_index(int e, int a0, int w0)
{
    const int r = e / w0;
    return r * kMbUsedX + a0 + (e - r * w0);
}

// Local slot j (0 .. popc(mask) - 1) -> plan slot: the j-th set bit of mask.
__device__ __forceinline__ int mb_slot(uint32_t mask, int j)
{
    for (int q = 0; q < j; q++) mask &= mask - 1;
    return __ffs(mask) - 1;
}

// u16 lane of channel k in a packed level-1 entry (x = (c0, c2), y = (c1, c3))
__device__ __forceinline__ int ch16(uint2 v, int k)
{
    return (int)((((k & 1) ? v.y : v.x) >> ((k & 2) ? 16 : 0)) & 0xffffu);
}

// f(std::integral_constant<int, 0>()) .. f(std::integral_constant<int, N - 1>()), in order.
template <int I, int N, class F>
__device__ __forceinline__ void static_for_(F &&f)
{
    if constexpr (I < N) {
        f(std::integral_constant<int, I>());
        static_for_<I + 1, N>(f);
    }
}
template <int N, class F>
__device__ __forceinline__ void static_for(F &&f) { static_for_<0, N>(f); }

// XCD-grouped 1-D launch of nx * ny units (x: a band or blend tile, y: its captures): block b
// runs on XCD b % 8 (the dispatcher deals blocks round-robin), and XCD k takes the contiguous
// unit range [k * per, (k + 1) * per), x-major -- so all captures of one band / tile run on one
// XCD one after another, and the band's descriptors (101 KB, the same for every capture) or the
// tile's tables come from that XCD's L2 after the first wave instead of being fetched again by
// every capture (round 3: 0.58 GB of descriptor reads per C2 launch, every band's 32 waves spread
// over the whole launch and over the XCDs).  False past the launch's units.
__device__ __forceinline__ bool xcd_unit(int nx, int ny, int &x, int &y)
{
    const int n = nx * ny, per = (n + 7) >> 3;
    const int u = (int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3);
    if (u >= n) return false;
    x = u / ny;
    y = u - x * ny;
    return true;
}

}  // namespace mcs
