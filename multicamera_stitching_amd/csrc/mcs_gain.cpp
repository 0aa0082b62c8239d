// mcs_gain.cpp -- exposure gain compensation (include/mcs.h "Exposure"): the overlap statistics
// of a plan (table built once per plan and grid step, sums per batch of captures), the gain solve
// (host FP64, Brown & Lowe's objective as OpenCV's detail::GainCompensator states it), the gains a
// plan carries and the kernel that applies one to a camera's source bytes; and the table-free
// statistics of a plan that lives for one capture (mcs_plan_overlap_stats_direct[_async]: one
// launch, nothing kept on the plan).  Device code: mcs_gain.h.
#include <cmath>
#include <cstring>
#include <vector>

#include "mcs_common.h"
#include "mcs_plan_state.h"
#include "mcs_scratch.h"

using namespace mcs::host;

namespace {

constexpr int64_t kOverlapTableLimit = 64ll << 20;

// q = clamp(round-half-even(256 g), 1, 65535); false for a gain that is not finite and positive.
bool quantise_gain(double g, uint16_t *q)
{
    if (!std::isfinite(g) || !(g > 0.0)) return false;
    const double r = std::nearbyint(256.0 * g);   // (round to nearest even: the default mode)
    *q = (uint16_t)(r < 1.0 ? 1.0 : r > 65535.0 ? 65535.0 : r);
    return true;
}

// Builds p->ov for grid step k on stream s (count pass, prefix sum on the host, fill pass).
int build_overlap(const Api *A, mcs_plan *p, const Kernels *kn, int k, hipStream_t s)
{
    drop_overlap(A, p);
    int rc = upload_plan_tables(A, p, s);
    if (rc) return rc;
    const int n = p->fd.n_cams;
    const int gw = (p->fd.out_w + (1 << k) - 1) >> k, gh = (p->fd.out_h + (1 << k) - 1) >> k;
    const int64_t np = (int64_t)gw * gh;
    // count[kOvSegs] u32, cursor[kOvSegs] u32, seg_off[kOvSegs] i64
    const size_t cnt_bytes = mcs::kOvSegs * sizeof(uint32_t);
    std::vector<uint32_t> cnt(mcs::kOvSegs, 0);
    std::vector<int64_t> off(mcs::kOvSegs, 0);
    std::vector<mcs::OvUnit> units;
    mcs::Scratch sc(A, s);
    uint8_t *d_small = nullptr, *d_table = nullptr;
    HIP_TRY(sc.dev(&d_small, 2 * cnt_bytes + mcs::kOvSegs * sizeof(int64_t)));
    mcs::KOverlapPrepArgs a;
    memset(&a, 0, sizeof(a));
    a.P = p->kp;
    a.count = reinterpret_cast<uint32_t *>(d_small);
    a.cursor = a.count + mcs::kOvSegs;
    int64_t *d_off = reinterpret_cast<int64_t *>(d_small + 2 * cnt_bytes);
    a.seg_off = d_off;
    a.gw = gw;
    a.gh = gh;
    a.k = k;
    const unsigned blocks = (unsigned)((np + mcs::kOvPrepThreads - 1) / mcs::kOvPrepThreads);
    int64_t bytes = 0;
    if (np > 0) {   // the count pass
        HIP_TRY(A->hipMemsetAsync(d_small, 0, 2 * cnt_bytes, s));
        a.mode = 0;
        rc = launch_args(A, kn->overlap_prep[p->fd.interp], blocks, 1, mcs::kOvPrepThreads, 1, &a,
                         sizeof(a), s);
        if (rc) return rc;
        HIP_TRY(A->hipMemcpyAsync(cnt.data(), a.count, cnt_bytes, hipMemcpyDeviceToHost, s));
        HIP_TRY(sc.sync());
    }
    for (int i = 0; i < n; i++)
        for (int j = i; j < n; j++) {
            const int seg = i * MCS_MAX_CAMS + j;
            const int64_t c = cnt[seg], esz = i == j ? 8 : 16;
            off[seg] = bytes;
            for (int64_t e = 0; e < c; e += mcs::kOvUnitEntries) {
                mcs::OvUnit u;
                u.off = bytes + e * esz;
                u.cam_a = i;
                u.cam_b = j;
                u.n = (int)std::min<int64_t>(mcs::kOvUnitEntries, c - e);
                u.pad_ = 0;
                units.push_back(u);
            }
            bytes += (c * esz + 15) & ~(int64_t)15;
        }
    const int64_t total = bytes + (int64_t)units.size() * sizeof(mcs::OvUnit);
    if (total > kOverlapTableLimit)
        return mcs::fail(MCS_E_UNSUPPORTED, "the overlap table at step_log2 %d takes %lld "
                         "bytes (limit %lld): use a larger step_log2", k, (long long)total,
                         (long long)kOverlapTableLimit);
    if (!units.empty()) {   // the fill pass (else: no camera covers a grid point)
        HIP_TRY(sc.dev(&d_table, (size_t)total));
        HIP_TRY(A->hipMemcpyAsync(d_off, off.data(), mcs::kOvSegs * sizeof(int64_t),
                                  hipMemcpyHostToDevice, s));
        HIP_TRY(A->hipMemcpyAsync(d_table + bytes, units.data(),
                                  units.size() * sizeof(mcs::OvUnit), hipMemcpyHostToDevice, s));
        a.table = d_table;
        a.mode = 1;
        rc = launch_args(A, kn->overlap_prep[p->fd.interp], blocks, 1, mcs::kOvPrepThreads, 1, &a,
                         sizeof(a), s);
        if (rc) return rc;
        HIP_TRY(sc.sync());
    }
    mcs_plan::Overlap &ov = p->ov;
    ov.step = k;
    ov.d_table = sc.keep(d_table);   // (the plan's from here on: drop_overlap frees it)
    ov.d_units = d_table ? reinterpret_cast<mcs::OvUnit *>(d_table + bytes) : nullptr;
    ov.n_units = (int)units.size();
    ov.table_bytes = bytes;
    for (int i = 0; i < n; i++)
        for (int j = i; j < n; j++)
            ov.N[i * MCS_MAX_CAMS + j] = ov.N[j * MCS_MAX_CAMS + i] = cnt[i * MCS_MAX_CAMS + j];
    return MCS_OK;
}

// The argument checks of the direct entry points after their NULL checks: those of
// mcs_plan_overlap_stats, in its order.
int check_stats_args(const mcs_plan *p, const uint8_t *const *d_cams, int n_frames, int step_log2)
{
    if (p->single)
        return mcs::fail(MCS_E_UNSUPPORTED, "a single-camera remap plan (warp / undistort) has "
                         "no overlaps");
    if (step_log2 < 0 || step_log2 > 4)
        return mcs::fail(MCS_E_INVALID, "step_log2 %d (0..4)", step_log2);
    if (n_frames < 1 || n_frames > 65535) return mcs::fail(MCS_E_INVALID, "n_frames=%d", n_frames);
    bool need[MCS_MAX_CAMS];
    need_mask(p->fd, need);
    for (int i = 0; i < p->fd.n_cams; i++)
        if (need[i] && !d_cams[i]) return mcs::fail(MCS_E_INVALID, "d_cams[%d] NULL", i);
    return MCS_OK;
}

// The table-free statistics of checked arguments on stream s (the device is set): d_stats zeroed,
// then one launch of mcs_direct_overlap_* unless the mosaic is empty.
int enqueue_direct_stats(const Api *A, mcs_plan *p, const uint8_t *const *d_cams,
                         const int64_t *cam_frame_stride, int n_frames, int k,
                         unsigned long long *d_stats, hipStream_t s)
{
    const int n = p->fd.n_cams, C = p->fd.channels;
    const size_t bytes = (size_t)(1 + n_frames) * n * n * sizeof(unsigned long long);
    HIP_TRY(A->hipMemsetAsync(d_stats, 0, bytes, s));
    if (p->fd.out_w <= 0 || p->fd.out_h <= 0) return MCS_OK;
    const Kernels *kn = nullptr;
    int rc = kernels(A, p, &kn);
    if (rc) return rc;
    rc = upload_plan_tables(A, p, s);   // (cylinder / lensed plans: their device tables, once)
    if (rc) return rc;
    mcs::KDirectOverlapArgs a;
    memset(&a, 0, sizeof(a));
    a.P = p->kp;
    for (int i = 0; i < n; i++) {
        a.P.cams[i] = d_cams[i];
        a.P.cam_fstride[i] = cam_fstride(p->fd, cam_frame_stride, i);
    }
    a.P.out = nullptr;
    a.stats = d_stats;
    a.gw = (p->fd.out_w + (1 << k) - 1) >> k;
    a.gh = (p->fd.out_h + (1 << k) - 1) >> k;
    a.k = k;
    a.n_frames = n_frames;
    a.n_cams = n;
    return launch_args(A, kn->direct_overlap[C][p->fd.interp],
                       mcs::dov_blocks((int64_t)a.gw * a.gh),
                       (unsigned)((n_frames + mcs::kOvFrames - 1) / mcs::kOvFrames),
                       mcs::kDovThreads, 1, &a, sizeof(a), s);
}

// The accumulators of mcs_plan_overlap_stats_direct: per calling thread and device, grown on
// demand, kept for the thread's next call (the call synchronises before it returns, so the
// buffer is idle between calls; it is never freed).
struct StatsScratch {
    unsigned long long *d = nullptr;
    size_t bytes = 0;
};
thread_local StatsScratch tl_stats[mcs::kMaxDevices];

}  // namespace

namespace mcs {
namespace host {

void drop_overlap(const Api *A, mcs_plan *p)
{
    if (p->stream) (void)A->hipStreamSynchronize(p->stream);
    if (p->ov.d_table) (void)A->hipFree(p->ov.d_table);
    if (p->ov.d_S) (void)A->hipFree(p->ov.d_S);
    p->ov = mcs_plan::Overlap{};
}

int launch_gain(const Api *A, const Kernels *k, const uint8_t *src, uint8_t *dst, int64_t bytes,
                int64_t src_fstride, int64_t dst_fstride, int n_frames, uint32_t q,
                const uint16_t *d_q, hipStream_t s)
{
    if (bytes <= 0 || n_frames <= 0) return MCS_OK;
    mcs::KGainArgs a;
    memset(&a, 0, sizeof(a));
    a.src = src;
    a.dst = dst;
    a.bytes = bytes;
    a.src_fstride = src_fstride;
    a.dst_fstride = dst_fstride;
    a.q_tab = d_q;
    a.q = q;
    // the vector blocks of the longest body, then the block of the head and tail bytes
    const int64_t per = (int64_t)mcs::kGainThreads * mcs::kGainVecs;
    const unsigned gx = (unsigned)(((bytes >> 4) + per - 1) / per) + 1;
    return launch_args(A, k->gain_apply, gx, (unsigned)n_frames, mcs::kGainThreads, 1, &a,
                       sizeof(a), s);
}

}  // namespace host

int gain_apply_frames(const mcs_plan *plan, const uint8_t *d_src, uint8_t *d_dst, int64_t bytes,
                      int64_t src_frame_stride, int64_t dst_frame_stride, int n_frames,
                      uint32_t q, const uint16_t *d_q, void *stream)
{
    const mcs::Entry A(plan->device);
    if (A.status) return A.status;
    const Kernels *k = nullptr;
    const int rc = kernels(A, plan, &k);
    if (rc) return rc;
    return launch_gain(A, k, d_src, d_dst, bytes, src_frame_stride, dst_frame_stride, n_frames, q,
                       d_q, (hipStream_t)stream);
}

}  // namespace mcs

extern "C" {

int mcs_gain_solve_host(int n_cams, const int64_t *N, const int64_t *S, int channels, double alpha,
                        double beta, double *gains)
{
    mcs::clear_error();
    if (!N || !S || !gains) return mcs::fail(MCS_E_INVALID, "NULL N/S/gains");
    if (n_cams < 1 || n_cams > MCS_MAX_CAMS || channels < 1 || channels > 4)
        return mcs::fail(MCS_E_INVALID, "n_cams %d, channels %d", n_cams, channels);
    if (!std::isfinite(alpha) || !std::isfinite(beta) || alpha < 0.0 || beta < 0.0)
        return mcs::fail(MCS_E_INVALID, "alpha / beta");
    const int n = n_cams;
    // cameras that cover a grid point; the others keep gain 1 and stay out of the system
    int idx[MCS_MAX_CAMS], m = 0;
    for (int i = 0; i < n; i++) {
        gains[i] = 1.0;
        if (N[i * n + i] > 0) idx[m++] = i;
    }
    if (m == 0) return MCS_OK;
    const auto mean = [&](int i, int j) {
        const int64_t c = N[i * n + j];
        return c > 0 ? (double)S[i * n + j] / ((double)channels * (double)c) : 0.0;
    };
    double Am[MCS_MAX_CAMS][MCS_MAX_CAMS + 1] = {};   // [A | b]
    for (int a = 0; a < m; a++)
        for (int b = 0; b < m; b++) {
            const int i = idx[a], j = idx[b];
            const double nij = (double)N[i * n + j];
            Am[a][m] += beta * nij;
            Am[a][a] += beta * nij;
            if (j == i) continue;
            const double Iij = mean(i, j), Iji = mean(j, i);
            Am[a][a] += 2.0 * alpha * Iij * Iij * nij;
            Am[a][b] -= 2.0 * alpha * Iij * Iji * nij;
        }
    // Gaussian elimination, partial pivoting (first largest magnitude), fixed order
    for (int c = 0; c < m; c++) {
        int piv = c;
        for (int r = c + 1; r < m; r++)
            if (std::fabs(Am[r][c]) > std::fabs(Am[piv][c])) piv = r;
        if (!(std::fabs(Am[piv][c]) > 0.0))
            return mcs::fail(MCS_E_INVALID, "singular gain system (beta = 0 without overlaps?)");
        if (piv != c)
            for (int k = c; k <= m; k++) std::swap(Am[c][k], Am[piv][k]);
        for (int r = c + 1; r < m; r++) {
            const double f = Am[r][c] / Am[c][c];
            for (int k = c; k <= m; k++) Am[r][k] -= f * Am[c][k];
        }
    }
    for (int r = m - 1; r >= 0; r--) {
        double v = Am[r][m];
        for (int k = r + 1; k < m; k++) v -= Am[r][k] * gains[idx[k]];
        gains[idx[r]] = v / Am[r][r];
    }
    return MCS_OK;
}

int mcs_plan_set_gains(mcs_plan *p, const double *gains)
{
    mcs::clear_error();
    if (!p) return mcs::fail(MCS_E_INVALID, "NULL plan");
    if (!gains) {
        p->gains_on = false;
        for (uint16_t &q : p->gain_q) q = 0;
        return MCS_OK;
    }
    uint16_t q[MCS_MAX_CAMS] = {};
    for (int i = 0; i < p->fd.n_cams; i++)
        if (!quantise_gain(gains[i], &q[i]))
            return mcs::fail(MCS_E_INVALID, "gain of camera %d is not finite and positive", i);
    memcpy(p->gain_q, q, sizeof(q));
    p->gains_on = true;
    return MCS_OK;
}

int mcs_plan_gains(const mcs_plan *p, uint16_t *q, int *enabled)
{
    if (!p) return mcs::fail(MCS_E_INVALID, "NULL plan");
    if (enabled) *enabled = p->gains_on ? 1 : 0;
    if (q)
        for (int i = 0; i < p->fd.n_cams; i++) q[i] = p->gains_on ? p->gain_q[i] : (uint16_t)256;
    return MCS_OK;
}

int mcs_gain_apply_device(const uint8_t *d_src, uint8_t *d_dst, int64_t bytes,
                          int64_t src_frame_stride, int64_t dst_frame_stride, int n_frames,
                          uint16_t q, int device, void *stream)
{
    mcs::clear_error();
    if (!d_src || !d_dst) return mcs::fail(MCS_E_INVALID, "NULL src/dst");
    if (bytes < 1 || n_frames < 1 || n_frames > 65535 || q < 1)
        return mcs::fail(MCS_E_INVALID, "bytes %lld, n_frames %d, q %d", (long long)bytes, n_frames,
                         (int)q);
    if (device < 0 || device >= mcs::kMaxDevices) return mcs::fail(MCS_E_INVALID, "device=%d", device);
    const int64_t ss = src_frame_stride ? src_frame_stride : bytes;
    const int64_t ds = dst_frame_stride ? dst_frame_stride : bytes;
    if (ss < bytes || ds < bytes) return mcs::fail(MCS_E_INVALID, "frame stride smaller than a frame");
    // in place (the same frames) or disjoint: a lane reads only the bytes it writes
    const uintptr_t s0 = (uintptr_t)d_src, s1 = s0 + (uintptr_t)((n_frames - 1) * ss + bytes);
    const uintptr_t d0 = (uintptr_t)d_dst, d1 = d0 + (uintptr_t)((n_frames - 1) * ds + bytes);
    const bool in_place = s0 == d0 && (ss == ds || n_frames == 1);
    if (!in_place && s0 < d1 && d0 < s1)
        return mcs::fail(MCS_E_INVALID, "src and dst overlap partially (in place: the same "
                         "pointer and frame stride)");
    const mcs::Entry A(device);
    if (A.status) return A.status;
    const Kernels *k = nullptr;
    const int rc = kernels(A, device, &k);
    if (rc) return rc;
    return launch_gain(A, k, d_src, d_dst, bytes, ss, ds, n_frames, q, nullptr,
                       (hipStream_t)stream);
}

int mcs_plan_overlap_stats(mcs_plan *p, const uint8_t *const *d_cams,
                           const int64_t *cam_frame_stride, int n_frames, int step_log2,
                           int64_t *N, int64_t *S, void *stream)
{
    mcs::clear_error();
    if (!p || !d_cams || !N || !S) return mcs::fail(MCS_E_INVALID, "NULL plan/d_cams/N/S");
    if (p->single)
        return mcs::fail(MCS_E_UNSUPPORTED, "a single-camera remap plan (warp / undistort) has "
                         "no overlaps");
    if (step_log2 < 0 || step_log2 > 4)
        return mcs::fail(MCS_E_INVALID, "step_log2 %d (0..4)", step_log2);
    if (n_frames < 1 || n_frames > 65535) return mcs::fail(MCS_E_INVALID, "n_frames=%d", n_frames);
    const int n = p->fd.n_cams, C = p->fd.channels;
    bool need[MCS_MAX_CAMS];
    need_mask(p->fd, need);
    for (int i = 0; i < n; i++)
        if (need[i] && !d_cams[i]) return mcs::fail(MCS_E_INVALID, "d_cams[%d] NULL", i);
    const size_t s_count = (size_t)n_frames * n * n;
    for (int i = 0; i < n * n; i++) N[i] = 0;
    for (size_t i = 0; i < s_count; i++) S[i] = 0;
    if (p->fd.out_w <= 0 || p->fd.out_h <= 0) return MCS_OK;
    const mcs::Entry A(p->device);
    if (A.status) return A.status;
    hipStream_t s = (hipStream_t)stream;
    int rc = MCS_OK;
    if (!s) {
        rc = ensure_stream(A, p);
        if (rc) return rc;
        s = p->stream;
    }
    const Kernels *k = nullptr;
    rc = kernels(A, p, &k);
    if (rc) return rc;
    if (p->ov.step != step_log2) {
        rc = build_overlap(A, p, k, step_log2, s);
        if (rc) return rc;
    }
    mcs_plan::Overlap &ov = p->ov;
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) N[i * n + j] = ov.N[i * MCS_MAX_CAMS + j];
    if (ov.n_units == 0) return MCS_OK;
    const size_t s_bytes = s_count * sizeof(unsigned long long);
    if (ov.s_bytes < s_bytes) {
        if (ov.d_S) {
            HIP_TRY(A->hipStreamSynchronize(s));
            HIP_TRY(A->hipFree(ov.d_S));
            ov.d_S = nullptr;
            ov.s_bytes = 0;
        }
        HIP_TRY(A->hipMalloc((void **)&ov.d_S, s_bytes));
        ov.s_bytes = s_bytes;
    }
    HIP_TRY(A->hipMemsetAsync(ov.d_S, 0, s_bytes, s));
    mcs::KOverlapSumArgs a;
    memset(&a, 0, sizeof(a));
    for (int i = 0; i < n; i++) {
        a.cams[i] = d_cams[i];
        a.cam_fstride[i] = cam_fstride(p->fd, cam_frame_stride, i);
        a.cam_w[i] = p->fd.cam_w[i];
        a.cam_h[i] = p->fd.cam_h[i];
    }
    a.table = ov.d_table;
    a.units = ov.d_units;
    a.S = ov.d_S;
    a.n_cams = n;
    a.n_frames = n_frames;
    rc = launch_args(A, k->overlap_sum[C], (unsigned)ov.n_units,
                     (unsigned)((n_frames + mcs::kOvFrames - 1) / mcs::kOvFrames),
                     mcs::kOvSumThreads, 1, &a, sizeof(a), s);
    if (rc) return rc;
    HIP_TRY(A->hipMemcpyAsync(S, ov.d_S, s_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(A->hipStreamSynchronize(s));
    return MCS_OK;
}

int mcs_plan_overlap_stats_direct_async(mcs_plan *p, const uint8_t *const *d_cams,
                                        const int64_t *cam_frame_stride, int n_frames,
                                        int step_log2, int64_t *d_stats, void *stream)
{
    mcs::clear_error();
    if (!p || !d_cams || !d_stats) return mcs::fail(MCS_E_INVALID, "NULL plan/d_cams/d_stats");
    const int rc = check_stats_args(p, d_cams, n_frames, step_log2);
    if (rc) return rc;
    const mcs::Entry A(p->device);
    if (A.status) return A.status;
    return enqueue_direct_stats(A, p, d_cams, cam_frame_stride, n_frames, step_log2,
                                reinterpret_cast<unsigned long long *>(d_stats),
                                (hipStream_t)stream);
}

int mcs_plan_overlap_stats_direct(mcs_plan *p, const uint8_t *const *d_cams,
                                  const int64_t *cam_frame_stride, int n_frames, int step_log2,
                                  int64_t *N, int64_t *S, void *stream)
{
    mcs::clear_error();
    if (!p || !d_cams || !N || !S) return mcs::fail(MCS_E_INVALID, "NULL plan/d_cams/N/S");
    int rc = check_stats_args(p, d_cams, n_frames, step_log2);
    if (rc) return rc;
    const int n = p->fd.n_cams;
    const size_t nn = (size_t)n * n, count = (1 + (size_t)n_frames) * nn;
    for (size_t i = 0; i < nn; i++) N[i] = 0;
    for (size_t i = 0; i < count - nn; i++) S[i] = 0;
    if (p->fd.out_w <= 0 || p->fd.out_h <= 0) return MCS_OK;
    const mcs::Entry A(p->device);
    if (A.status) return A.status;
    hipStream_t s = (hipStream_t)stream;
    if (!s) {
        rc = ensure_stream(A, p);
        if (rc) return rc;
        s = p->stream;
    }
    StatsScratch &sc = tl_stats[p->device];
    const size_t bytes = count * sizeof(unsigned long long);
    if (sc.bytes < bytes) {
        if (sc.d) HIP_TRY(A->hipFree(sc.d));
        sc.d = nullptr;
        sc.bytes = 0;
        HIP_TRY(A->hipMalloc((void **)&sc.d, bytes));
        sc.bytes = bytes;
    }
    rc = enqueue_direct_stats(A, p, d_cams, cam_frame_stride, n_frames, step_log2, sc.d, s);
    static thread_local std::vector<int64_t> host;
    host.resize(count);
    hipError_t e = hipSuccess;
    if (rc == MCS_OK) e = A->hipMemcpyAsync(host.data(), sc.d, bytes, hipMemcpyDeviceToHost, s);
    const hipError_t e2 = A->hipStreamSynchronize(s);   // (drains the queued work on error too)
    if (rc) return rc;
    if (e != hipSuccess || e2 != hipSuccess)
        return mcs::fail(MCS_E_HIP, "overlap statistics: %s",
                         A->hipGetErrorString(e != hipSuccess ? e : e2));
    memcpy(N, host.data(), nn * sizeof(int64_t));
    memcpy(S, host.data() + nn, (count - nn) * sizeof(int64_t));
    return MCS_OK;
}

int mcs_plan_overlap_stats_host(mcs_plan *p, const uint8_t *const *cams, int step_log2, int64_t *N,
                                int64_t *S)
{
    mcs::clear_error();
    if (!p || !cams || !N || !S) return mcs::fail(MCS_E_INVALID, "NULL plan/cams/N/S");
    if (p->single)
        return mcs::fail(MCS_E_UNSUPPORTED, "a single-camera remap plan (warp / undistort) has "
                         "no overlaps");
    if (step_log2 < 0 || step_log2 > 4)
        return mcs::fail(MCS_E_INVALID, "step_log2 %d (0..4)", step_log2);
    bool need[MCS_MAX_CAMS];
    need_mask(p->fd, need);
    for (int i = 0; i < p->fd.n_cams; i++)
        if (need[i] && !cams[i]) return mcs::fail(MCS_E_INVALID, "cams[%d] NULL", i);
    const mcs::Entry A(p->device);
    if (A.status) return A.status;
    int rc = ensure_stream(A, p);
    if (rc == MCS_OK) rc = ensure_host_buffers(A, p);
    if (rc) return rc;
    const int C = p->fd.channels;
    for (int i = 0; i < p->fd.n_cams; i++) {
        if (!need[i]) continue;
        HIP_TRY(A->hipMemcpyAsync(p->d_cams[i], cams[i],
                                  (size_t)p->fd.cam_w[i] * p->fd.cam_h[i] * C,
                                  hipMemcpyHostToDevice, p->stream));
    }
    return mcs_plan_overlap_stats(p, p->d_cams, nullptr, 1, step_log2, N, S, p->stream);
}

}  // extern "C"
