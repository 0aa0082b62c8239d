// mcs_features.cpp -- C ABI of the per-frame estimation path (include/mcs.h, "Matching"):
// brute-force Hamming kNN-2 on the GPU.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <mutex>

#include <vector>

#include "mcs_common.h"
#include "mcs_feat_int.h"
#include "mcs_fparams.h"
#include "mcs_orb_core.h"
#include "mcs_ransac_core.h"
#include "mcs_scratch.h"

namespace {

using mcs::rt::Api;
using mcs::feat::FeatureKernels;
using mcs::feat::feature_kernels;
using mcs::feat::launch;

FeatureKernels g_fk[mcs::kMaxDevices];
std::mutex g_fk_mu;

// Scratch buffer + stream of the synchronous per-frame entry points (ORB, Hamming kNN-2, RANSAC:
// called for every rig capture in the C3 estimation loop), one per thread and device: grown on
// demand, reused across calls, kept for the thread's lifetime (no per-call hipMalloc / stream
// creation; released with the process).  The entry points are synchronous, so a thread never has
// two calls in flight on its workspace.
struct Workspace {
    uint8_t *buf = nullptr;
    size_t cap = 0;
    hipStream_t s = nullptr;
    hipEvent_t ev = nullptr;   // blocking-sync event: ws_sync's wait point
};
thread_local Workspace tl_ws[mcs::kMaxDevices];

// Waits for the work queued on workspace stream `s`: hipStreamSynchronize, or with
// MCS_FEATURE_SYNC=block through an event created with hipEventBlockingSync (the thread sleeps
// instead of spinning; measured slower for the C3 loop on the 16-CPU box, so not the default).
hipError_t ws_sync(const Api *A, hipStream_t s)
{
    static const bool spin =
        !getenv("MCS_FEATURE_SYNC") || strcmp(getenv("MCS_FEATURE_SYNC"), "block");
    if (!spin)
        for (Workspace &w : tl_ws)
            if (w.s == s) {
                if (!w.ev) {
                    // hipEventBlockingSync | hipEventDisableTiming
                    hipError_t e = A->hipEventCreateWithFlags(&w.ev, 0x1u | 0x2u);
                    if (e != hipSuccess) return e;
                }
                hipError_t e = A->hipEventRecord(w.ev, s);
                return e == hipSuccess ? A->hipEventSynchronize(w.ev) : e;
            }
    return A->hipStreamSynchronize(s);
}

int workspace(const Api *A, int device, size_t bytes, uint8_t **buf, hipStream_t *s)
{
    if (device < 0 || device >= mcs::kMaxDevices)
        return mcs::fail(MCS_E_INVALID, "device %d", device);
    Workspace &w = tl_ws[device];
    if (!w.s) HIP_TRY(A->hipStreamCreateWithFlags(&w.s, hipStreamNonBlocking));
    if (w.cap < bytes) {
        if (w.buf) HIP_TRY(A->hipFree(w.buf));
        w.buf = nullptr;
        w.cap = 0;
        const size_t want = std::max(bytes, (size_t)1 << 20);
        HIP_TRY(A->hipMalloc((void **)&w.buf, want));
        w.cap = want;
    }
    *buf = w.buf;
    *s = w.s;
    return MCS_OK;
}

}  // namespace

int mcs::features_stream_wait(int device, void *event)
{
    const mcs::Entry A(device);
    if (A.status) return A.status;
    uint8_t *buf = nullptr;
    hipStream_t s = nullptr;
    int rc = workspace(A, device, 0, &buf, &s);
    if (rc) return rc;
    HIP_TRY(A->hipStreamWaitEvent(s, (hipEvent_t)event, 0));
    return MCS_OK;
}

int mcs::feat::feature_kernels(const Api *A, int device, const FeatureKernels **out)
{
    if (device < 0 || device >= mcs::kMaxDevices)
        return mcs::fail(MCS_E_INVALID, "device %d", device);
    std::lock_guard<std::mutex> lk(g_fk_mu);
    FeatureKernels &k = g_fk[device];
    if (!k.loaded) {
        int rc = mcs::module_function(A, device, mcs::kModFeatures, "mcs_hamming_knn2", &k.knn2);
        if (rc == MCS_OK)
            rc = mcs::module_function(A, device, mcs::kModFeatures, "mcs_hamming_knn2_finalize",
                                      &k.knn2_finalize);
        if (rc == MCS_OK)
            rc = mcs::module_function(A, device, mcs::kModFeatures, "mcs_ransac_score",
                                      &k.ransac_score);
        if (rc == MCS_OK)
            rc = mcs::module_function(A, device, mcs::kModFeatures, "mcs_ransac_mask",
                                      &k.ransac_mask);
        const struct {
            const char *name;
            hipFunction_t *f;
        } orb[] = {{"mcs_orb_gray", &k.orb_gray},     {"mcs_orb_level", &k.orb_level},
                   {"mcs_orb_pyramid", &k.orb_pyramid},
                   {"mcs_orb_describe", &k.orb_describe},
                   {"mcs_orb_select", &k.orb_select},
                   {"mcs_l2_prep", &k.l2_prep},       {"mcs_l2_knn2_i8", &k.l2_i8},
                   {"mcs_l2_knn2_f32", &k.l2_f32},    {"mcs_l2_knn2_finalize", &k.l2_finalize},
                   {"mcs_rig_knn2", &k.rig_knn2},     {"mcs_rig_match", &k.rig_match},
                   {"mcs_rig_ransac", &k.rig_ransac}, {"mcs_rig_best", &k.rig_best},
                   {"mcs_rig_hyp", &k.rig_hyp},       {"mcs_rig_unlens", &k.rig_unlens},
                   {"mcs_seam_flow_init", &k.seam_init}, {"mcs_seam_flow_hinit", &k.seam_hinit},
                   {"mcs_seam_flow_push", &k.seam_push},
                   {"mcs_seam_flow_active", &k.seam_active},
                   {"mcs_seam_flow_label", &k.seam_label},
                   {"mcs_seam_flow_relabel_lds", &k.seam_relabel_lds}};
        for (const auto &o : orb)
            if (rc == MCS_OK) rc = mcs::module_function(A, device, mcs::kModFeatures, o.name, o.f);
        if (rc) return rc;
        k.loaded = true;
    }
    *out = &k;
    return MCS_OK;
}

int mcs::feat::launch(const Api *A, hipFunction_t f, unsigned gx, unsigned gy, unsigned bx,
                      void *args, size_t sz, hipStream_t s, unsigned gz, unsigned lds)
{
    void *cfg[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, args, HIP_LAUNCH_PARAM_BUFFER_SIZE, &sz,
                   HIP_LAUNCH_PARAM_END};
    HIP_TRY(A->hipModuleLaunchKernel(f, gx, gy, gz, bx, 1, 1, lds, s, nullptr, cfg));
    return MCS_OK;
}

mcs::feat::KnnShape mcs::feat::knn_shape(int queries, int pairs, int train)
{
    KnnShape k = {};
    k.qblocks = (unsigned)((queries + kKnnQueriesPerBlock - 1) / kKnnQueriesPerBlock);
    const int blocks = (int)k.qblocks * pairs;
    int chunks = (kKnnTargetBlocks + blocks - 1) / blocks;
    chunks = std::max(1, std::min(chunks, (train + 63) / 64));
    k.per_chunk = (train + chunks - 1) / chunks;
    k.chunks = train > 0 ? (unsigned)((train + k.per_chunk - 1) / k.per_chunk) : 0u;
    return k;
}

namespace {

int knn2(const Api *A, const FeatureKernels *k, const uint8_t *q, int nq, const uint8_t *t, int nt,
         int32_t *idx2, int32_t *dist2, hipStream_t s)
{
    HIP_TRY(A->hipMemsetAsync(idx2, 0xff, (size_t)nq * 2 * sizeof(int32_t), s));
    mcs::KHammingArgs a;
    a.query = reinterpret_cast<const uint32_t *>(q);
    a.train = reinterpret_cast<const uint32_t *>(t);
    a.keys = reinterpret_cast<uint32_t *>(idx2);
    a.dist = dist2;
    a.nq = nq;
    a.nt = nt;
    a.pad_ = 0;
    const mcs::feat::KnnShape ks = mcs::feat::knn_shape(nq, 1, nt);
    a.per_chunk = ks.per_chunk;
    if (ks.chunks > 0) {
        const int rc = launch(A, k->knn2, ks.qblocks, ks.chunks, mcs::kKnnLanes, &a, sizeof(a), s);
        if (rc) return rc;
    }
    return launch(A, k->knn2_finalize, (2 * nq + 255) / 256, 1, 256, &a, sizeof(a), s);
}

// L2 kNN-2 on device buffers (float descriptors); scratch allocated here; synchronises.
int l2_knn2(const Api *A, const FeatureKernels *k, const float *dq, int nq, const float *dt, int nt,
            int dim, int32_t *idx2, float *dist2, int *exact, hipStream_t s)
{
    const int dimp = (dim + 63) / 64 * 64;
    const size_t n = (size_t)nq + nt;
    const size_t b8 = n * dimp, bi = n * 4, bk = (size_t)nq * 2 * 8;
    static const char what[] = "l2 knn2";
    uint32_t hflag = 0;
    mcs::Scratch sc(A, s);
    uint8_t *buf = nullptr;
    HIP_TRY(sc.dev(&buf, b8 + 5 * bi + bk + 256));
    int8_t *d8 = reinterpret_cast<int8_t *>(buf);
    uint8_t *p = buf + ((b8 + 15) & ~(size_t)15);
    int32_t *norm_i = reinterpret_cast<int32_t *>(p);
    int32_t *sum_i = norm_i + n;
    float *norm_f = reinterpret_cast<float *>(sum_i + n);
    uint32_t *flag = reinterpret_cast<uint32_t *>(norm_f + n);
    unsigned long long *keys =
        reinterpret_cast<unsigned long long *>(((uintptr_t)(flag + 4) + 15) & ~(uintptr_t)15);
    int rc = MCS_OK;
    HIP_TRY_AS(what, A->hipMemsetAsync(flag, 0, 4, s));
    HIP_TRY_AS(what, A->hipMemsetAsync(keys, 0xff, bk, s));
    for (int side = 0; side < 2; side++) {
        mcs::KL2PrepArgs pa;
        pa.desc = side ? dt : dq;
        pa.n = side ? nt : nq;
        const size_t o = side ? (size_t)nq : 0;
        pa.i8 = d8 + o * dimp;
        pa.norm_i = norm_i + o;
        pa.sum_i = sum_i + o;
        pa.norm_f = norm_f + o;
        pa.flag = flag;
        pa.dim = dim;
        pa.dimp = dimp;
        pa.pad_ = 0;
        if (pa.n > 0) rc = launch(A, k->l2_prep, (pa.n + 3) / 4, 1, 256, &pa, sizeof(pa), s);
        if (rc) return rc;
    }
    mcs::KL2Args a;
    a.q8 = d8;
    a.t8 = d8 + (size_t)nq * dimp;
    a.qf = dq;
    a.tf = dt;
    a.qn = norm_i, a.tn = norm_i + nq, a.qs = sum_i, a.ts = sum_i + nq;
    a.qnf = norm_f, a.tnf = norm_f + nq;
    a.flag = flag;
    a.keys = keys;
    a.idx = idx2;
    a.dist = dist2;
    a.nq = nq, a.nt = nt, a.dim = dim, a.dimp = dimp, a.pad_ = 0;
    const int qblocks = (nq + mcs::kL2QueriesPerBlock - 1) / mcs::kL2QueriesPerBlock;
    int chunks = (2048 + qblocks - 1) / qblocks;
    chunks = std::max(1, std::min(chunks, (nt + 255) / 256));
    a.per_chunk = ((nt + chunks - 1) / chunks + 15) / 16 * 16;
    chunks = nt > 0 ? (nt + a.per_chunk - 1) / a.per_chunk : 0;
    if (chunks > 0) {
        rc = launch(A, k->l2_i8, qblocks, chunks, 256, &a, sizeof(a), s);
        if (rc == MCS_OK) rc = launch(A, k->l2_f32, qblocks, chunks, 256, &a, sizeof(a), s);
        if (rc) return rc;
    }
    rc = launch(A, k->l2_finalize, (2 * nq + 255) / 256, 1, 256, &a, sizeof(a), s);
    if (rc) return rc;
    HIP_TRY_AS(what, A->hipMemcpyAsync(&hflag, flag, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY_AS(what, sc.synced(ws_sync(A, s)));
    if (exact) *exact = hflag ? 0 : 1;
    return MCS_OK;
}

// mcs_match_l2_knn2_host on its stream s, after the checks: upload, match, copy back.
int l2_host_on_stream(const Api *A, const FeatureKernels *k, hipStream_t s, const float *query,
                      int n_query, const float *train, int n_train, int dim, int32_t *idx2,
                      float *dist2, int *exact)
{
    static const char what[] = "l2 host path";
    const size_t qb = (size_t)n_query * dim * 4, tb = (size_t)n_train * dim * 4;
    const size_t ob = (size_t)n_query * 2 * 4;
    mcs::Scratch sc(A, s);
    uint8_t *buf = nullptr;
    HIP_TRY(sc.dev(&buf, qb + tb + 2 * ob + 64));
    float *dq = reinterpret_cast<float *>(buf);
    float *dt = reinterpret_cast<float *>(buf + qb);
    int32_t *di = reinterpret_cast<int32_t *>(buf + ((qb + tb + 15) & ~(size_t)15));
    float *dd = reinterpret_cast<float *>(di + (size_t)n_query * 2);
    HIP_TRY_AS(what, A->hipMemcpyAsync(dq, query, qb, hipMemcpyHostToDevice, s));
    if (tb) HIP_TRY_AS(what, A->hipMemcpyAsync(dt, train, tb, hipMemcpyHostToDevice, s));
    const int rc = l2_knn2(A, k, dq, n_query, dt, n_train, dim, di, dd, exact, s);
    if (rc) return rc;
    HIP_TRY_AS(what, A->hipMemcpyAsync(idx2, di, ob, hipMemcpyDeviceToHost, s));
    HIP_TRY_AS(what, A->hipMemcpyAsync(dist2, dd, ob, hipMemcpyDeviceToHost, s));
    HIP_TRY_AS(what, sc.synced(ws_sync(A, s)));
    return MCS_OK;
}

int check_l2(int nq, int nt, int dim)
{
    if (nq < 0 || nt < 0 || nq > (1 << 26) || nt > (1 << 30) || dim < 1 || dim > mcs::kL2MaxDim)
        return mcs::fail(MCS_E_INVALID, "n_query=%d n_train=%d dim=%d (1..%d)", nq, nt, dim,
                         mcs::kL2MaxDim);
    return MCS_OK;
}

int check_sizes(int nq, int nt)
{
    if (nq < 0 || nt < 0 || nt >= mcs::kKnnMaxTrain || nq > (1 << 26))
        return mcs::fail(MCS_E_INVALID, "n_query=%d n_train=%d (train < %d)", nq, nt,
                         mcs::kKnnMaxTrain);
    return MCS_OK;
}

// The status of a per-call entry point's body on workspace stream s.  A failed body first drains
// the stream: it may have queued copies from or towards host memory that the entry point, or its
// caller on seeing the status, is about to release.
int drained(const Api *A, hipStream_t s, int rc)
{
    if (rc) (void)ws_sync(A, s);
    return rc;
}

// mcs_match_hamming_knn2_host on its workspace (buf, s), after the checks.
int knn2_host(const Api *A, const FeatureKernels *k, uint8_t *buf, hipStream_t s,
              const uint8_t *query, int n_query, const uint8_t *train, int n_train, int32_t *idx2,
              int32_t *dist2)
{
    static const char what[] = "knn2 host path";
    const size_t qb = (size_t)n_query * mcs::kDescBytes, tb = (size_t)n_train * mcs::kDescBytes;
    const size_t ob = (size_t)n_query * 2 * sizeof(int32_t);
    uint8_t *dq = buf, *dt = buf + qb;
    int32_t *di = reinterpret_cast<int32_t *>(buf + ((qb + tb + 15) & ~(size_t)15));
    int32_t *dd = di + (size_t)n_query * 2;
    HIP_TRY_AS(what, A->hipMemcpyAsync(dq, query, qb, hipMemcpyHostToDevice, s));
    if (tb) HIP_TRY_AS(what, A->hipMemcpyAsync(dt, train, tb, hipMemcpyHostToDevice, s));
    const int rc = knn2(A, k, dq, n_query, dt, n_train, di, dd, s);
    if (rc) return rc;
    HIP_TRY_AS(what, A->hipMemcpyAsync(idx2, di, ob, hipMemcpyDeviceToHost, s));
    HIP_TRY_AS(what, A->hipMemcpyAsync(dist2, dd, ob, hipMemcpyDeviceToHost, s));
    HIP_TRY_AS(what, ws_sync(A, s));
    return MCS_OK;
}

// mcs_ransac_homography_host's host temporaries (they outlive the body: see drained).
struct RansacHost {
    std::vector<double> pts;        // n x (x, y, u, v)
    std::vector<int32_t> scores;    // per hypothesis
    std::vector<uint8_t> mask;      // the best model's inliers
    double h8[8] = {0};             // the best model
    int best_score = -1;
};

// mcs_ransac_homography_host on its workspace, after the checks: the best hypothesis (the first
// of the maximum score) and, when it has the 4 inliers a model needs, its mask and model into `t`.
int ransac_host(const Api *A, const FeatureKernels *k, uint8_t *buf, hipStream_t s, int n,
                double thresh, int iters, uint32_t seed, RansacHost &t)
{
    static const char what[] = "ransac";
    const size_t pb = t.pts.size() * sizeof(double), hb = (size_t)iters * 8 * sizeof(double);
    const size_t sb = (size_t)iters * sizeof(int32_t);
    mcs::KRansacArgs a;
    a.pts = reinterpret_cast<double *>(buf);
    a.hyps = reinterpret_cast<double *>(buf + pb);
    a.scores = reinterpret_cast<int32_t *>(buf + pb + hb);
    a.mask = buf + pb + hb + sb;
    a.t2 = thresh * thresh;
    a.n = n;
    a.iters = iters;
    a.best = 0;
    a.seed = seed;
    HIP_TRY_AS(what, A->hipMemcpyAsync((void *)a.pts, t.pts.data(), pb, hipMemcpyHostToDevice, s));
    int rc = launch(A, k->ransac_score, iters, 1, mcs::kRansacBlock, &a, sizeof(a), s);
    if (rc) return rc;
    HIP_TRY_AS(what, A->hipMemcpyAsync(t.scores.data(), a.scores, sb, hipMemcpyDeviceToHost, s));
    HIP_TRY_AS(what, ws_sync(A, s));
    int best = -1;
    for (int i = 0; i < iters; i++)
        if (t.scores[i] > t.best_score) t.best_score = t.scores[i], best = i;
    if (t.best_score < 4) return MCS_OK;
    a.best = best;
    rc = launch(A, k->ransac_mask, (n + 255) / 256, 1, 256, &a, sizeof(a), s);
    if (rc) return rc;
    HIP_TRY_AS(what, A->hipMemcpyAsync(t.mask.data(), a.mask, (size_t)n, hipMemcpyDeviceToHost, s));
    HIP_TRY_AS(what, A->hipMemcpyAsync(t.h8, a.hyps + (size_t)best * 8, sizeof(t.h8),
                                       hipMemcpyDeviceToHost, s));
    HIP_TRY_AS(what, ws_sync(A, s));
    return MCS_OK;
}

}  // namespace

extern "C" {

int mcs_match_hamming_knn2(const uint8_t *d_query, int n_query, const uint8_t *d_train,
                           int n_train, int32_t *d_idx2, int32_t *d_dist2, int device,
                           void *stream)
{
    mcs::clear_error();
    int rc = check_sizes(n_query, n_train);
    if (rc) return rc;
    if (n_query == 0) return MCS_OK;
    if (!d_query || (!d_train && n_train) || !d_idx2 || !d_dist2)
        return mcs::fail(MCS_E_INVALID, "NULL buffer");
    const mcs::Entry A(device);
    if (A.status) return A.status;
    const FeatureKernels *k = nullptr;
    rc = feature_kernels(A, device, &k);
    if (rc) return rc;
    return knn2(A, k, d_query, n_query, d_train, n_train, d_idx2, d_dist2, (hipStream_t)stream);
}

int mcs_match_hamming_knn2_host(const uint8_t *query, int n_query, const uint8_t *train,
                                int n_train, int32_t *idx2, int32_t *dist2, int device)
{
    mcs::clear_error();
    int rc = check_sizes(n_query, n_train);
    if (rc) return rc;
    if (n_query == 0) return MCS_OK;
    if (!query || (!train && n_train) || !idx2 || !dist2)
        return mcs::fail(MCS_E_INVALID, "NULL buffer");
    const mcs::Entry A(device);
    if (A.status) return A.status;
    const FeatureKernels *k = nullptr;
    rc = feature_kernels(A, device, &k);
    if (rc) return rc;
    uint8_t *buf = nullptr;
    hipStream_t s = nullptr;
    // (both descriptor sets, then idx2 and dist2: knn2_host)
    rc = workspace(A, device, ((size_t)n_query + n_train) * mcs::kDescBytes +
                                  (size_t)n_query * 4 * sizeof(int32_t) + 64, &buf, &s);
    if (rc) return rc;
    return drained(A, s, knn2_host(A, k, buf, s, query, n_query, train, n_train, idx2, dist2));
}

int mcs_match_l2_knn2(const float *d_query, int n_query, const float *d_train, int n_train,
                      int dim, int32_t *d_idx2, float *d_dist2, int *exact, int device,
                      void *stream)
{
    mcs::clear_error();
    int rc = check_l2(n_query, n_train, dim);
    if (rc) return rc;
    if (n_query == 0) return MCS_OK;
    if (!d_query || (!d_train && n_train) || !d_idx2 || !d_dist2)
        return mcs::fail(MCS_E_INVALID, "NULL buffer");
    const mcs::Entry A(device);
    if (A.status) return A.status;
    const FeatureKernels *k = nullptr;
    rc = feature_kernels(A, device, &k);
    if (rc) return rc;
    return l2_knn2(A, k, d_query, n_query, d_train, n_train, dim, d_idx2, d_dist2, exact,
                   (hipStream_t)stream);
}

int mcs_match_l2_knn2_host(const float *query, int n_query, const float *train, int n_train,
                           int dim, int32_t *idx2, float *dist2, int *exact, int device)
{
    mcs::clear_error();
    int rc = check_l2(n_query, n_train, dim);
    if (rc) return rc;
    if (n_query == 0) return MCS_OK;
    if (!query || (!train && n_train) || !idx2 || !dist2)
        return mcs::fail(MCS_E_INVALID, "NULL buffer");
    const mcs::Entry A(device);
    if (A.status) return A.status;
    const FeatureKernels *k = nullptr;
    rc = feature_kernels(A, device, &k);
    if (rc) return rc;
    hipStream_t s = nullptr;
    HIP_TRY_AS("l2 host path", A->hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    rc = l2_host_on_stream(A, k, s, query, n_query, train, n_train, dim, idx2, dist2, exact);
    (void)A->hipStreamDestroy(s);
    return rc;
}

int mcs_ransac_homography_host(const float *src_xy, const float *dst_xy, int n, double thresh,
                               int iters, uint32_t seed, double *H, uint8_t *mask,
                               int *n_inliers, int device)
{
    mcs::clear_error();
    if (!src_xy || !dst_xy || !H || !n_inliers) return mcs::fail(MCS_E_INVALID, "NULL buffer");
    if (n < 0 || iters <= 0 || iters > (1 << 20) || !(thresh >= 0.0))
        return mcs::fail(MCS_E_INVALID, "n=%d iters=%d thresh=%g", n, iters, thresh);
    *n_inliers = 0;
    for (int i = 0; i < 9; i++) H[i] = 0.0;
    if (mask)
        for (int i = 0; i < n; i++) mask[i] = 0;
    if (n < 4) return MCS_OK;   // no model (the reference needs > 4 matches to try)
    const mcs::Entry A(device);
    if (A.status) return A.status;
    const FeatureKernels *k = nullptr;
    int rc = feature_kernels(A, device, &k);
    if (rc) return rc;
    RansacHost t;
    t.pts.resize((size_t)n * 4);
    for (int i = 0; i < n; i++) {
        t.pts[4 * i] = src_xy[2 * i], t.pts[4 * i + 1] = src_xy[2 * i + 1];
        t.pts[4 * i + 2] = dst_xy[2 * i], t.pts[4 * i + 3] = dst_xy[2 * i + 1];
    }
    t.scores.resize((size_t)iters);
    t.mask.resize((size_t)n);
    uint8_t *buf = nullptr;
    hipStream_t s = nullptr;
    rc = workspace(A, device, t.pts.size() * sizeof(double) + (size_t)iters * 8 * sizeof(double) +
                                  (size_t)iters * sizeof(int32_t) + (size_t)n + 64, &buf, &s);
    if (rc) return rc;
    rc = drained(A, s, ransac_host(A, k, buf, s, n, thresh, iters, seed, t));
    if (rc || t.best_score < 4) return rc;
    // findHomography's refinement of the chosen model on its inliers (mcs_refine.cpp:
    // normalised DLT re-estimate + Levenberg-Marquardt, StitcherClass.py:443-444)
    for (int i = 0; i < 8; i++) H[i] = t.h8[i];
    H[8] = 1.0;
    mcs::homography_refine(src_xy, dst_xy, n, t.mask.data(), H);
    *n_inliers = t.best_score;
    if (mask)
        for (int i = 0; i < n; i++) mask[i] = t.mask[i];
    return MCS_OK;
}

}  // extern "C"

// Source index of destination index d in OpenCV's resize(INTER_LINEAR) (mcs_orb_pyramid's
// pyr_axis, the same float arithmetic).
static int pyr_src(int d, double scale, int ssize, bool is_x)
{
    float f = (float)((d + 0.5) * scale - 0.5);
    int si = (int)std::floor(f);
    if (is_x) {
        if (si < 0) si = 0;
        if (si >= ssize - 1) si = ssize - 1;
    }
    return si;
}

// mcs_orb_pyramid's arguments: last-level tiles of 32 x 16 (8 x 8 for small levels), the LDS
// buffer size from every block's dependency regions (the kernel's top-down walk, on the host).
// Returns the block count, 0 when the fused launch does not apply (a >= 2x level step, or
// regions too large for LDS).
unsigned mcs::feat::pyramid_args(const OrbGeom &g, uint8_t *lvl, KOrbBuildArgs &a)
{
    const int *lw = g.lw, *lh = g.lh, nlevels = g.nlevels;
    const size_t *off = g.off;
    std::memset(&a, 0, sizeof(a));
    const int L = nlevels - 1;
    for (int l = 1; l <= L; l++) {
        if (2 * lw[l] <= lw[l - 1] || 2 * lh[l] <= lh[l - 1]) return 0;
        a.sx[l] = 1. / ((double)lw[l] / lw[l - 1]);
        a.sy[l] = 1. / ((double)lh[l] / lh[l - 1]);
    }
    for (int l = 0; l <= L; l++) {
        a.off[l] = (int64_t)off[l];
        a.w[l] = lw[l];
        a.h[l] = lh[l];
    }
    a.lvl = lvl;
    a.nlevels = nlevels;
    a.tw = lw[L] >= 256 ? 32 : 8;
    a.th = lw[L] >= 256 ? 16 : 8;
    a.gx = (lw[L] + a.tw - 1) / a.tw;
    const int gy = (lh[L] + a.th - 1) / a.th;
    int mw = 1, mh = 1;
    for (int t = 0; t < a.gx * gy; t++) {
        int x0 = (t % a.gx) * a.tw, y0 = (t / a.gx) * a.th;
        int x1 = std::min(x0 + a.tw, lw[L]), y1 = std::min(y0 + a.th, lh[L]);
        for (int l = L; l >= 2; l--) {
            const int sw = lw[l - 1], sh = lh[l - 1];
            const int nx0 = pyr_src(x0, a.sx[l], sw, true), sxl = pyr_src(x1 - 1, a.sx[l], sw, true);
            const int nx1 = sxl >= sw - 1 ? sw : sxl + 2;
            const int ny0 = std::min(std::max(pyr_src(y0, a.sy[l], sh, false), 0), sh - 1);
            const int ny1 = std::min(std::max(pyr_src(y1 - 1, a.sy[l], sh, false) + 1, 0), sh - 1) + 1;
            x0 = nx0, x1 = nx1, y0 = ny0, y1 = ny1;
            if (l - 1 >= 1 && l - 1 < L) mw = std::max(mw, x1 - x0), mh = std::max(mh, y1 - y0);
        }
    }
    a.lds_w = mw;
    a.lds_h = mh;
    if (2 * (size_t)mw * mh + 16 > 64 * 1024) return 0;   // (+16: mcs_orb_pyramid reads 8 bytes past a row)
    return (unsigned)(a.gx * gy);
}

int mcs::feat::orb_geom(int w, int h, int nfeatures, int nlevels, float scale_factor,
                        OrbGeom *g)
{
    g->nlevels = nlevels;
    for (int l = 0; l < nlevels; l++) {
        g->lscale[l] = (float)std::pow((double)scale_factor, (double)l);
        g->lw[l] = (int)std::lrint((float)w / g->lscale[l]);
        g->lh[l] = (int)std::lrint((float)h / g->lscale[l]);
        if (g->lw[l] < 1 || g->lh[l] < 1) return mcs::fail(MCS_E_INVALID, "level %d is empty", l);
        g->off[l + 1] = g->off[l] + (((size_t)g->lw[l] * g->lh[l] + 255) & ~(size_t)255);
    }
    const float factor = (float)(1.0 / scale_factor);
    float per = nfeatures * (1 - factor) / (1 - (float)std::pow((double)factor, (double)nlevels));
    int sum = 0;
    // (each level's rounded share capped by what is left: the roundings can add up to more than
    // nfeatures -- 15 for 14 features on 11 levels --, and the callers' arrays hold nfeatures)
    for (int l = 0; l < nlevels - 1; l++) {
        g->quota[l] = std::min((int)std::lrint(per), nfeatures - sum);
        sum += g->quota[l];
        per *= factor;
    }
    g->quota[nlevels - 1] = nfeatures - sum;
    g->n_bound = 0;
    g->cap_total = 0;
    for (int l = 0; l < nlevels; l++) {
        g->n_bound += g->quota[l];
        g->cap[l] = std::max((size_t)4096, (size_t)g->lw[l] * g->lh[l] / 8);
        g->coff[l + 1] = g->coff[l] + g->cap[l];
        g->cap_total += g->cap[l];
    }
    return MCS_OK;
}

void mcs::feat::orb_chain(OrbChain *c, int w, int h, int fast_threshold, int n_frames,
                          const OrbBuffers &b)
{
    const OrbGeom &g = c->geo;
    const int L = g.nlevels;
    const int64_t pix = (int64_t)g.off[L];
    c->w = w, c->h = h, c->n_frames = n_frames;
    const int K = c->K = std::max(g.n_bound, 1);
    std::memset(&c->ga, 0, sizeof(c->ga));
    c->ga.gray = b.lvl, c->ga.stride = pix, c->ga.n = w * h;
    // levels 1 .. nlevels-1: one launch (mcs_orb_pyramid) when every level is a < 2x downscale of
    // the one before (its blocks' dependency regions then tile every level), else a resize each
    c->pyr_blocks = pyramid_args(g, b.lvl, c->ba);
    c->ba.stride = pix;
    // blur, FAST, NMS and Harris of every level: one launch (kOrbTileW x kOrbTileH tiles); then
    // the ranking on the device: a level with more than kOrbSelMax candidates sets the frame's
    // overflow flag instead (sel[1]; the per-call entry point then ranks on the host)
    KOrbPyrArgs &pa = c->pa;
    KOrbSelArgs &sa = c->sa;
    std::memset(&pa, 0, sizeof(pa));
    std::memset(&sa, 0, sizeof(sa));
    pa.img = b.lvl, pa.blur = b.blur;
    pa.cand = b.cand, sa.cand = b.cand;
    pa.ncand = b.ncand, sa.ncand = b.ncand;
    pa.nlevels = sa.nlevels = L;
    pa.threshold = fast_threshold;
    pa.stride = pix;
    pa.cstride = sa.cstride = (int)g.cap_total;
    sa.kp = b.kp, sa.resp = b.resp, sa.sel = b.sel, sa.kstride = K;
    for (int l = 0; l < L; l++) {
        pa.off[l] = (int64_t)g.off[l];
        pa.coff[l] = sa.coff[l] = (int)g.coff[l];
        pa.w[l] = g.lw[l];
        pa.h[l] = g.lh[l];
        pa.cap[l] = sa.cap[l] = (int)g.cap[l];
        pa.bstart[l + 1] = pa.bstart[l] + (g.lw[l] + kOrbTileW - 1) / kOrbTileW *
                                              ((g.lh[l] + kOrbTileH - 1) / kOrbTileH);
        sa.quota[l] = g.quota[l];
    }
    KOrbDescArgs &da = c->da;
    std::memset(&da, 0, sizeof(da));
    for (int l = 0; l < kOrbMaxLevels; l++) {
        const int ll = l < L ? l : 0;
        da.img[l] = b.lvl + g.off[ll];
        da.blur[l] = b.blur + g.off[ll];
        da.w[l] = g.lw[ll];
    }
    da.kp = b.kp, da.desc = b.desc, da.orient = b.orient, da.sel = b.sel;
    da.n = g.n_bound, da.kstride = K, da.stride = pix;
}

int mcs::feat::orb_enqueue(const Api *A, const FeatureKernels *k, OrbChain &c,
                           const uint8_t *const *frames, int channels, int device, hipStream_t s)
{
    const OrbGeom &g = c.geo;
    const int C = c.n_frames, L = g.nlevels;
    const int64_t pix = (int64_t)g.off[L];
    int rc = MCS_OK;
    if (channels == 3) {
        for (int f = 0; f < C; f++) c.ga.bgr[f] = frames[f];
        rc = launch(A, k->orb_gray, (unsigned)((c.w * c.h + 1023) / 1024), C, 256, &c.ga,
                    sizeof(c.ga), s);
        if (rc) return rc;
    } else {
        for (int f = 0; f < C; f++)
            HIP_TRY_AS("orb", A->hipMemcpyAsync(c.ga.gray + f * pix, frames[f],
                                                (size_t)c.w * c.h, hipMemcpyDeviceToDevice, s));
    }
    if (L > 1 && c.pyr_blocks > 0) {
        rc = launch(A, k->orb_pyramid, c.pyr_blocks, C, 256, &c.ba, sizeof(c.ba), s, 1,
                    (unsigned)(2 * c.ba.lds_w * c.ba.lds_h + 16));
        if (rc) return rc;
    } else {
        for (int l = 1; l < L; l++) {
            rc = mcs_resize_linear_device(c.ga.gray + g.off[l - 1], g.lw[l - 1], g.lh[l - 1],
                                          g.lw[l - 1], pix, c.ga.gray + g.off[l], g.lw[l], g.lh[l],
                                          g.lw[l], pix, 1, C, device, s);
            if (rc) return rc;
        }
    }
    rc = launch(A, k->orb_level, (unsigned)c.pa.bstart[L], C, kOrbLevelThreads, &c.pa,
                sizeof(c.pa), s);
    if (rc) return rc;
    rc = launch(A, k->orb_select, (unsigned)L, C, kOrbSelThreads, &c.sa, sizeof(c.sa), s);
    if (rc) return rc;
    if (g.n_bound > 0)
        rc = launch(A, k->orb_describe, (unsigned)g.n_bound, C, 64, &c.da, sizeof(c.da), s);
    return rc;
}

namespace {

// orb_detect's host results (they outlive the body: see drained).
struct OrbHost {
    std::vector<int> kp;             // n x (level, x, y)
    std::vector<double> orient;      // n x (cos, sin)
    std::vector<double> resp;
    int n = 0;
};

// orb_detect on its workspace stream s, after the checks: the frame (uploaded to `upload` unless
// that is NULL: it lies on the device), the chain, then ONE copy back of [b.ncand, + back_bytes):
// counts, keypoints, descriptors, orientations, responses and the ranking's [n, overflow].  On
// overflow the host ranks and the chain's describe launch runs again on its keypoints.
int orb_host(const Api *A, const FeatureKernels *k, mcs::feat::OrbChain &ch,
             const mcs::feat::OrbBuffers &b, uint8_t *upload, size_t back_bytes,
             const uint8_t *image, int channels, int device, hipStream_t s, OrbHost &t,
             uint8_t *desc)
{
    static const char what[] = "orb";
    const mcs::feat::OrbGeom &g = ch.geo;
    const int nlevels = g.nlevels;
    const uint8_t *in = image;
    if (upload) {
        HIP_TRY_AS(what, A->hipMemcpyAsync(upload, image, (size_t)ch.w * ch.h * channels,
                                           hipMemcpyHostToDevice, s));
        in = upload;
    }
    HIP_TRY_AS(what, A->hipMemsetAsync(b.ncand, 0, mcs::kOrbMaxLevels * sizeof(int), s));
    int rc = mcs::feat::orb_enqueue(A, k, ch, &in, channels, device, s);
    if (rc) return rc;
    static thread_local std::vector<uint8_t> blob;
    if (blob.size() < back_bytes) blob.resize(back_bytes);
    const uint8_t *dev0 = reinterpret_cast<const uint8_t *>(b.ncand);
    auto at = [&](const void *d) { return blob.data() + (static_cast<const uint8_t *>(d) - dev0); };
    HIP_TRY_AS(what, A->hipMemcpyAsync(blob.data(), dev0, back_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY_AS(what, ws_sync(A, s));
    const int *sel = reinterpret_cast<const int *>(at(b.sel));
    if (!sel[1]) {
        const size_t n = t.n = sel[0];
        const int *kpd = reinterpret_cast<const int *>(at(b.kp));
        const double *respd = reinterpret_cast<const double *>(at(b.resp));
        const double *ord = reinterpret_cast<const double *>(at(b.orient));
        t.kp.assign(kpd, kpd + 3 * n);
        t.resp.assign(respd, respd + n);
        t.orient.assign(ord, ord + 2 * n);
        std::memcpy(desc, at(b.desc), n * 32);
        return MCS_OK;
    }
    // host ranking: only the candidates each level found come back (the host copy: per thread,
    // grown on demand, never cleared -- only the entries the counts cover are copied and read)
    static thread_local std::vector<mcs::OrbCand> cand;
    if (cand.size() < g.cap_total) cand.resize(g.cap_total);
    int counts[mcs::kOrbMaxLevels];
    for (int l = 0; l < nlevels; l++) {
        counts[l] = std::min(std::max(reinterpret_cast<const int *>(blob.data())[l], 0),
                             (int)g.cap[l]);
        if (counts[l] > 0)
            HIP_TRY_AS(what, A->hipMemcpyAsync(cand.data() + g.coff[l], b.cand + g.coff[l],
                                               (size_t)counts[l] * sizeof(mcs::OrbCand),
                                               hipMemcpyDeviceToHost, s));
    }
    HIP_TRY_AS(what, ws_sync(A, s));
    // per level: rank by response (desc), then y, then x; keep the level's quota (a strict total
    // order -- positions are unique -- so selecting the quota first and sorting only it gives the
    // full sort's prefix)
    for (int l = 0; l < nlevels; l++) {
        const int c = counts[l];
        mcs::OrbCand *lc = cand.data() + g.coff[l];
        auto rank = [](const mcs::OrbCand &p, const mcs::OrbCand &q) {
            if (p.response != q.response) return p.response > q.response;
            return p.y != q.y ? p.y < q.y : p.x < q.x;
        };
        const int keep = std::min(c, g.quota[l]);
        if (keep < c) std::nth_element(lc, lc + keep, lc + c, rank);
        std::sort(lc, lc + keep, rank);
        for (int i = 0; i < keep; i++) {
            t.kp.push_back(l);
            t.kp.push_back(lc[i].x);
            t.kp.push_back(lc[i].y);
            t.resp.push_back(lc[i].response);
        }
    }
    const int n = t.n = (int)t.kp.size() / 3;
    t.orient.resize(2 * (size_t)std::max(n, 1));
    if (n == 0) return MCS_OK;
    HIP_TRY_AS(what, A->hipMemcpyAsync(b.kp, t.kp.data(), t.kp.size() * sizeof(int),
                                       hipMemcpyHostToDevice, s));
    ch.da.sel = nullptr;
    ch.da.n = n;
    rc = launch(A, k->orb_describe, n, 1, 64, &ch.da, sizeof(ch.da), s);
    if (rc) return rc;
    HIP_TRY_AS(what, A->hipMemcpyAsync(desc, b.desc, (size_t)n * 32, hipMemcpyDeviceToHost, s));
    HIP_TRY_AS(what, A->hipMemcpyAsync(t.orient.data(), b.orient, (size_t)n * 2 * sizeof(double),
                                       hipMemcpyDeviceToHost, s));
    HIP_TRY_AS(what, ws_sync(A, s));
    return MCS_OK;
}

// ORB of one image (host memory, or device memory when on_device); mcs_orb_detect_host /
// mcs_orb_detect_device below.
int orb_detect(const uint8_t *image, bool on_device, int w, int h, int channels, int nfeatures,
               int nlevels, float scale_factor, int fast_threshold, float *kp_xy,
               float *kp_response, float *kp_angle, int *kp_level, uint8_t *desc, int *n_out,
               int device)
{
    mcs::clear_error();
    if (!image || !kp_xy || !desc || !n_out) return mcs::fail(MCS_E_INVALID, "NULL buffer");
    // (w, h < 2^16: the device ranking packs a keypoint's position as y << 16 | x)
    if (w <= 0 || h <= 0 || w > 65535 || h > 65535 || (channels != 1 && channels != 3) ||
        nfeatures < 0 ||
        nlevels < 1 || nlevels > mcs::kOrbMaxLevels || !(scale_factor > 1.0f) ||
        fast_threshold < 0 || fast_threshold > 255)
        return mcs::fail(MCS_E_INVALID, "w=%d h=%d channels=%d nfeatures=%d nlevels=%d "
                         "scale=%g threshold=%d", w, h, channels, nfeatures, nlevels,
                         (double)scale_factor, fast_threshold);
    *n_out = 0;
    const mcs::Entry A(device);
    if (A.status) return A.status;
    const FeatureKernels *k = nullptr;
    int rc = feature_kernels(A, device, &k);
    if (rc) return rc;
    // level sizes and quotas, as OpenCV's ORB computes them (float arithmetic)
    mcs::feat::OrbChain ch;
    rc = mcs::feat::orb_geom(w, h, nfeatures, nlevels, scale_factor, &ch.geo);
    if (rc) return rc;
    const size_t pix = ch.geo.off[nlevels];
    // one allocation: input, levels, blur (u16 pass + u8), scores, candidates, counts, keypoints,
    // descriptors, orientations
    size_t o = 0;
    auto take = [&](size_t bytes) {
        const size_t at = o;
        o += (bytes + 255) & ~(size_t)255;
        return at;
    };
    const size_t o_in = take((size_t)w * h * channels), o_lvl = take(pix), o_blur = take(pix);
    const size_t o_cand = take(ch.geo.cap_total * sizeof(mcs::OrbCand));
    const size_t o_cnt = take(mcs::kOrbMaxLevels * sizeof(int));
    const size_t o_kp = take((size_t)std::max(nfeatures, 1) * 3 * sizeof(int));
    const size_t o_desc = take((size_t)std::max(nfeatures, 1) * 32);
    const size_t o_or = take((size_t)std::max(nfeatures, 1) * 2 * sizeof(double));
    const size_t o_resp = take((size_t)std::max(nfeatures, 1) * sizeof(double));
    const size_t o_sel = take(2 * sizeof(int));
    const size_t o_end = o;   // [o_cnt, o_end): everything the device ranking path copies back
    uint8_t *buf = nullptr;
    hipStream_t s = nullptr;
    rc = workspace(A, device, o, &buf, &s);
    if (rc) return rc;
    const mcs::feat::OrbBuffers b = {
        buf + o_lvl, buf + o_blur, reinterpret_cast<mcs::OrbCand *>(buf + o_cand),
        reinterpret_cast<int *>(buf + o_cnt), reinterpret_cast<int *>(buf + o_kp),
        reinterpret_cast<double *>(buf + o_resp), buf + o_desc,
        reinterpret_cast<double *>(buf + o_or), reinterpret_cast<int *>(buf + o_sel)};
    mcs::feat::orb_chain(&ch, w, h, fast_threshold, 1, b);
    OrbHost t;
    rc = drained(A, s, orb_host(A, k, ch, b, on_device ? nullptr : buf + o_in, o_end - o_cnt,
                                image, channels, device, s, t, desc));
    if (rc) return rc;
    for (int i = 0; i < t.n; i++) {
        const int l = t.kp[3 * i];
        kp_xy[2 * i] = (float)t.kp[3 * i + 1] * ch.geo.lscale[l];
        kp_xy[2 * i + 1] = (float)t.kp[3 * i + 2] * ch.geo.lscale[l];
        if (kp_level) kp_level[i] = l;
        if (kp_response) kp_response[i] = (float)t.resp[i];
        if (kp_angle) {
            double a = std::atan2(t.orient[2 * i + 1], t.orient[2 * i]) * (180.0 / M_PI);
            if (a < 0) a += 360.0;
            kp_angle[i] = (float)a;
        }
    }
    *n_out = t.n;
    return MCS_OK;
}
}  // namespace

extern "C" {

int mcs_orb_detect_host(const uint8_t *image, int w, int h, int channels, int nfeatures,
                        int nlevels, float scale_factor, int fast_threshold, float *kp_xy,
                        float *kp_response, float *kp_angle, int *kp_level, uint8_t *desc,
                        int *n_out, int device)
{
    return orb_detect(image, false, w, h, channels, nfeatures, nlevels, scale_factor,
                      fast_threshold, kp_xy, kp_response, kp_angle, kp_level, desc, n_out, device);
}

int mcs_orb_detect_device(const uint8_t *d_image, int w, int h, int channels, int nfeatures,
                          int nlevels, float scale_factor, int fast_threshold, float *kp_xy,
                          float *kp_response, float *kp_angle, int *kp_level, uint8_t *desc,
                          int *n_out, int device)
{
    return orb_detect(d_image, true, w, h, channels, nfeatures, nlevels, scale_factor,
                      fast_threshold, kp_xy, kp_response, kp_angle, kp_level, desc, n_out, device);
}

}  // extern "C"
