// mcs_gain.h -- device code of exposure gain compensation, included by mcs_kernels.hip after
// mcs_blend.h (one code object): the overlap table of a plan (prepare once per plan and grid
// step), the per-capture overlap sums over it, the same statistics without a table (one launch
// per batch of captures, for a plan that lives for one capture), and the per-camera gain on
// source bytes.
//
// The statistics use the blend's own geometry: a camera slot's position at a grid point is
// slot_xy's, it covers the point iff slot_dist >= 0, and its luminance there is the sum of the
// channel bytes of sample_replicate (the blend's I_s).  Everything is integer, so the sums do
// not depend on the order in which blocks add them.
#pragma once

namespace mcs {

// ---- overlap table (once per plan and step) ---------------------------------------------------
// One thread per point of the 2^k grid; block kOvPrepThreads.  mode 0 counts the entries of every
// segment (one atomic per wave and segment: the ballot's population), mode 1 writes them (the
// wave's entries of a segment are consecutive).  Entry order inside a segment is arbitrary.
template <int INTERP>
__device__ __forceinline__ void overlap_prep(const KOverlapPrepArgs &a)
{
    const KParams &P = a.P;
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = q < a.gw * a.gh;
    const int x = live ? (q % a.gw) << a.k : 0, y = live ? (q / a.gw) << a.k : 0;
    const int lane = threadIdx.x & (kWave - 1);
    // covering slots of this point (slot s: bit s)
    uint32_t cov = 0;
    if (live) {
        for (int s = 0; s <= P.n_stages; s++) {
            int x32, y32, cam, w, h;
            slot_xy<INTERP>(P, s, x, y, x32, y32, cam, w, h);
            if (slot_dist(x32, y32, w, h) >= 0) cov |= 1u << s;
        }
    }
    for (int s = 0; s <= P.n_stages; s++) {
        int cam_s, ws, hs;
        slot_info(P, s, cam_s, ws, hs);
        for (int t = s; t <= P.n_stages; t++) {
            int cam_t, wt, ht;
            slot_info(P, t, cam_t, wt, ht);
            if (t != s && cam_t == cam_s) continue;   // (one slot per camera: nothing to pair)
            const bool in = ((cov >> s) & 1u) && ((cov >> t) & 1u);
            const uint64_t b = __builtin_amdgcn_ballot_w64(in);
            if (b == 0) continue;                     // (wave-uniform)
            // the lower camera first; the diagonal (t == s) is the camera's own segment
            const bool swap = cam_t < cam_s;
            const int seg = swap ? cam_t * MCS_MAX_CAMS + cam_s : cam_s * MCS_MAX_CAMS + cam_t;
            const int leader = __ffsll((unsigned long long)b) - 1;
            const uint32_t n = (uint32_t)__popcll(b);
            uint32_t base = 0;
            if (lane == leader) base = atomicAdd(a.mode == 0 ? &a.count[seg] : &a.cursor[seg], n);
            if (a.mode == 0) continue;
            base = (uint32_t)__shfl((int)base, leader, kWave);
            // (both passes see the same coverage, so e stays below the counted size; the bound
            // keeps a write inside the table whatever happens)
            const uint32_t e = base + (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
            if (in && e < a.count[seg]) {
                uint8_t *seg_tab = a.table + a.seg_off[seg];
                int xs, ys, xt, yt, c0, w0, h0;
                slot_xy<INTERP>(P, s, x, y, xs, ys, c0, w0, h0);
                if (t == s) {
                    reinterpret_cast<int2 *>(seg_tab)[e] = make_int2(xs, ys);
                } else {
                    slot_xy<INTERP>(P, t, x, y, xt, yt, c0, w0, h0);
                    reinterpret_cast<int4 *>(seg_tab)[e] =
                        swap ? make_int4(xt, yt, xs, ys) : make_int4(xs, ys, xt, yt);
                }
            }
        }
    }
}

// ---- overlap sums (per batch of captures) -----------------------------------------------------
// Sum of v over the wave, in every lane (butterfly over ds_bpermute).
__device__ __forceinline__ uint32_t wave_sum(uint32_t v, int lane)
{
#pragma unroll
    for (int m = kWave / 2; m > 0; m >>= 1) v += (uint32_t)lane_at((int)v, (lane ^ m) * 4);
    return v;
}

template <int CN>
__device__ __forceinline__ uint32_t luminance(const uint8_t *fb, int w, int h, int x32, int y32)
{
    const uint32_t v = sample_replicate<CN>(fb, w, h, x32, y32);
    uint32_t l = 0;
#pragma unroll
    for (int k = 0; k < CN; k++) l += (v >> (8 * k)) & 0xffu;
    return l;
}

// grid (units, ceil(n_frames / kOvFrames)), block kOvSumThreads.  The unit's cameras are uniform
// over the block; a lane walks entries tid, tid + kOvSumThreads, ... of the unit with the
// captures' sums in registers, then wave -> LDS -> one 64-bit atomic per (direction, capture).
template <int CN>
__device__ __forceinline__ void overlap_sum(const KOverlapSumArgs &a)
{
    constexpr int kWaves = kOvSumThreads / kWave;
    __shared__ uint32_t part[kWaves][2 * kOvFrames];
    const OvUnit u = a.units[blockIdx.x];
    const int f0 = blockIdx.y * kOvFrames;
    const int nf = min(kOvFrames, a.n_frames - f0);
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const bool diag = u.cam_a == u.cam_b;
    const int wa = a.cam_w[u.cam_a], ha = a.cam_h[u.cam_a];
    const int wb = a.cam_w[u.cam_b], hb = a.cam_h[u.cam_b];
    const int64_t sa = a.cam_fstride[u.cam_a], sb = a.cam_fstride[u.cam_b];
    const uint8_t *fa = a.cams[u.cam_a] + f0 * sa, *fb = a.cams[u.cam_b] + f0 * sb;
    const uint8_t *tab = a.table + u.off;
    uint32_t acc_a[kOvFrames] = {}, acc_b[kOvFrames] = {};
    for (int e = tid; e < u.n; e += kOvSumThreads) {
        int4 p;
        if (diag) {
            const int2 d = reinterpret_cast<const int2 *>(tab)[e];
            p = make_int4(d.x, d.y, 0, 0);
        } else {
            p = reinterpret_cast<const int4 *>(tab)[e];
        }
#pragma unroll
        for (int f = 0; f < kOvFrames; f++) {
            if (f >= nf) break;   // (uniform)
            acc_a[f] += luminance<CN>(fa + f * sa, wa, ha, p.x, p.y);
            if (!diag) acc_b[f] += luminance<CN>(fb + f * sb, wb, hb, p.z, p.w);
        }
    }
#pragma unroll
    for (int f = 0; f < kOvFrames; f++) {
        const uint32_t va = wave_sum(acc_a[f], lane), vb = wave_sum(acc_b[f], lane);
        if (lane == 0) {
            part[wave][2 * f] = va;
            part[wave][2 * f + 1] = vb;
        }
    }
    __syncthreads();
    if (tid >= 2 * kOvFrames) return;
    const int f = tid >> 1, dir = tid & 1;
    if (f >= nf || (diag && dir)) return;
    uint32_t s = 0;
#pragma unroll
    for (int w = 0; w < kWaves; w++) s += part[w][tid];
    // S[f][i][j]: camera i's luminance over the points of pair (i, j)
    const int i = dir ? u.cam_b : u.cam_a, j = dir ? u.cam_a : u.cam_b;
    atomicAdd(&a.S[((int64_t)(f0 + f) * a.n_cams + i) * a.n_cams + j], (unsigned long long)s);
}

// ---- table-free statistics (mcs_plan_overlap_stats_direct) ------------------------------------
// The N and S of the two kernels above in one launch, nothing stored: grid (dov_blocks(points),
// ceil(n_frames / kOvFrames)), block kDovThreads.  A block strides over the grid points, one lane
// per point.  Per point: the covering slots (slot_xy + slot_dist of every slot), then per slot s
// that some lane of the wave covers its luminance in up to kOvFrames captures (two captures per
// dword, 16 bits each) and, for every slot t of another camera -- and t = s, the diagonal --, the
// wave's lanes covered by both: N[cam_s][cam_t] gets their number, S[f][cam_s][cam_t] the sum of
// their luminances (the ordered pairs (s, t) and (t, s) give overlap_prep's two directions).  The
// wave's sums go to the block's 32-bit LDS partials (one ds_add per wave, pair and dword), the
// block's non-zero partials to the 64-bit accumulators at the end.  Blocks of grid row 0 count N.
template <int CN, int INTERP>
__device__ __forceinline__ void direct_overlap(const KDirectOverlapArgs &a)
{
    const KParams &P = a.P;
    __shared__ uint32_t part_n[kOvSegs];
    __shared__ uint32_t part_s[kOvFrames][kOvSegs];
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    part_n[tid] = 0;
#pragma unroll
    for (int f = 0; f < kOvFrames; f++) part_s[f][tid] = 0;
    __syncthreads();
    const int f0 = blockIdx.y * kOvFrames;
    const int nf = min(kOvFrames, a.n_frames - f0);
    const bool count = blockIdx.y == 0;
    const int64_t np = (int64_t)a.gw * a.gh;
    // the block's first point of each round, as (column, row) of the grid: advanced without a
    // division (the step is one division away, once)
    const int64_t step = (int64_t)gridDim.x * kDovThreads;
    const int step_x = (int)(step % a.gw), step_y = (int)(step / a.gw);
    int64_t base = (int64_t)blockIdx.x * kDovThreads;
    int bx = (int)(base % a.gw), by = (int)(base / a.gw);
    for (; base < np; base += step) {
        const bool live = base + tid < np;
        const uint32_t t0 = (uint32_t)(bx + tid);
        const int x = live ? (int)(t0 % (uint32_t)a.gw) << a.k : 0;
        const int y = live ? (by + (int)(t0 / (uint32_t)a.gw)) << a.k : 0;
        bx += step_x;
        by += step_y;
        if (bx >= a.gw) bx -= a.gw, by++;
        uint32_t cov = 0;
        if (live) {
            for (int s = 0; s <= P.n_stages; s++) {
                int x32, y32, cam, w, h;
                slot_xy<INTERP>(P, s, x, y, x32, y32, cam, w, h);
                if (slot_dist(x32, y32, w, h) >= 0) cov |= 1u << s;
            }
        }
        for (int s = 0; s <= P.n_stages; s++) {
            const bool in_s = (cov >> s) & 1u;
            if (__builtin_amdgcn_ballot_w64(in_s) == 0) continue;   // (wave-uniform)
            int cam_s, ws, hs;
            slot_info(P, s, cam_s, ws, hs);
            // luminance of captures (f0, f0 + 1) and (f0 + 2, f0 + 3), 16 bits each
            uint32_t l01 = 0, l23 = 0;
            if (in_s) {
                int xs, ys, c0, w0, h0;
                slot_xy<INTERP>(P, s, x, y, xs, ys, c0, w0, h0);
                const int64_t fs = P.cam_fstride[cam_s];
                const uint8_t *fb = P.cams[cam_s] + f0 * fs;
#pragma unroll
                for (int f = 0; f < kOvFrames; f++) {
                    if (f >= nf) break;   // (uniform)
                    const uint32_t l = luminance<CN>(fb + f * fs, ws, hs, xs, ys) << (16 * (f & 1));
                    if (f < 2) l01 |= l;
                    else l23 |= l;
                }
            }
            for (int t = 0; t <= P.n_stages; t++) {
                int cam_t, wt, ht;
                slot_info(P, t, cam_t, wt, ht);
                if (t != s && cam_t == cam_s) continue;   // (one slot per camera: nothing to pair)
                const bool in = in_s && ((cov >> t) & 1u);
                const uint64_t b = __builtin_amdgcn_ballot_w64(in);
                if (b == 0) continue;                     // (wave-uniform)
                const uint32_t s01 = wave_sum(in ? l01 : 0u, lane);
                const uint32_t s23 = nf > 2 ? wave_sum(in ? l23 : 0u, lane) : 0u;
                if (lane == 0) {
                    const int seg = cam_s * MCS_MAX_CAMS + cam_t;
                    if (count) atomicAdd(&part_n[seg], (uint32_t)__popcll(b));
                    atomicAdd(&part_s[0][seg], s01 & 0xffffu);
                    if (nf > 1) atomicAdd(&part_s[1][seg], s01 >> 16);
                    if (nf > 2) atomicAdd(&part_s[2][seg], s23 & 0xffffu);
                    if (nf > 3) atomicAdd(&part_s[3][seg], s23 >> 16);
                }
            }
        }
    }
    __syncthreads();
    // lane tid owns partial (i, j) = (tid / MCS_MAX_CAMS, tid % MCS_MAX_CAMS)
    const int i = tid / MCS_MAX_CAMS, j = tid % MCS_MAX_CAMS;
    if (i >= a.n_cams || j >= a.n_cams) return;
    const int64_t nn = (int64_t)a.n_cams * a.n_cams, e = (int64_t)i * a.n_cams + j;
    if (count && part_n[tid]) atomicAdd(&a.stats[e], (unsigned long long)part_n[tid]);
#pragma unroll
    for (int f = 0; f < kOvFrames; f++) {
        if (f >= nf) break;
        if (part_s[f][tid])
            atomicAdd(&a.stats[nn + (int64_t)(f0 + f) * nn + e], (unsigned long long)part_s[f][tid]);
    }
}

// ---- gain on source bytes (gain_half, gain_word, gain_byte: mcs_dev.h) -----------------------
// grid (ceil(bytes / kGainChunk) + 1, frames), block kGainThreads.  Per frame the destination's
// 16-byte aligned body moves as 16-byte vectors (the source side of an out-of-place call may be
// unaligned: an unaligned dwordx4 load), its head and tail as bytes by the last block of the row.
// In place: every lane reads its bytes before it writes the same ones.
__device__ __forceinline__ void gain_apply(const KGainArgs &a)
{
    const uint32_t q = a.q_tab ? (uint32_t)a.q_tab[0] : a.q;
    const gain_us2 qh = {(unsigned short)(q >> 8), (unsigned short)(q >> 8)};
    const gain_us2 ql = {(unsigned short)(q & 255u), (unsigned short)(q & 255u)};
    const uint8_t *src = a.src + (int64_t)blockIdx.y * a.src_fstride;
    uint8_t *dst = a.dst + (int64_t)blockIdx.y * a.dst_fstride;
    const int64_t head = min((int64_t)((16 - ((uintptr_t)dst & 15)) & 15), a.bytes);
    const int64_t nvec = (a.bytes - head) >> 4;
    if (blockIdx.x + 1 == gridDim.x) {
        // head [0, head) and tail [head + 16 nvec, bytes): fewer than 32 bytes
        const int64_t tail0 = head + (nvec << 4);
        const int64_t n = head + (a.bytes - tail0);
        if ((int64_t)threadIdx.x < n) {
            const int64_t o = (int64_t)threadIdx.x < head ? threadIdx.x : tail0 + (threadIdx.x - head);
            dst[o] = gain_byte(src[o], q);
        }
        return;
    }
    const int64_t v0 = (int64_t)blockIdx.x * (kGainThreads * kGainVecs) + threadIdx.x;
#pragma unroll
    for (int i = 0; i < kGainVecs; i++) {
        const int64_t v = v0 + i * kGainThreads;
        if (v >= nvec) break;
        uint4 w;
        __builtin_memcpy(&w, src + head + (v << 4), 16);
        w.x = gain_word(w.x, qh, ql);
        w.y = gain_word(w.y, qh, ql);
        w.z = gain_word(w.z, qh, ql);
        w.w = gain_word(w.w, qh, ql);
        *reinterpret_cast<uint4 *>(dst + head + (v << 4)) = w;
    }
}

}  // namespace mcs
