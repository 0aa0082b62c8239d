// mcs_rig.cpp -- config 3 estimation of a whole rig capture in libmcs:
// ORB of every camera frame, then per adjacent pair (camera k+1 -> camera k, k = 0 .. n-2)
// BF Hamming kNN-2, Lowe's ratio (strict, StitcherClass.py:432), more than 4 matches
// (:437), findHomography's RANSAC + LM (:440-441, mcs_ransac_homography_host).  The reference
// runs detectAndDescribe + matchKeypoints once at calibration (:356-448); config 3 runs them per
// capture.
//
// Device path (default): the whole capture is ONE launch chain on the job's own stream, with
// one host round trip -- the ORB kernels batched over the cameras (grid.y = camera), the pairs'
// kNN-2, ratio test + compaction, RANSAC hypotheses and best-model selection batched over the
// pairs (mcs_rig_* kernels, every count read on the device), then one copy back of the counts,
// best models, inlier masks and matched positions; the host only runs findHomography's LM
// refinement (mcs_refine.cpp) per pair.  The same kernels and arithmetic as the per-call entry
// points, so the same homographies, bit for bit.  The chain is captured once as a hipGraph and
// replayed while the job is fed the same frame pointers (one graph launch per capture; a new
// frame set re-captures it).
//
// Per-call path (a capture whose ORB ranking overflowed on the device -- more than kOrbSelMax
// candidates on a level --, or MCS_RIG_PATH=calls): the C-ABI's own steps
// (mcs_orb_detect_device, mcs_match_hamming_knn2_host, mcs_ransac_homography_host -- each with
// its thread's device workspace and stream) issued from libmcs's worker threads: a job's camera
// ORBs side by side, a pair queued as soon as both of its cameras' ORBs are done, the last pair
// marks the job done.
//
// Lenses (mcs_rig_job_set_lens): the job is fed raw frames.  ORB runs on them as they are; the
// positions of the ratio-passing matches go through the inverse lens of their cameras
// (mcs_lens_core.h lens_invert: mcs_rig_unlens in the chain, unlens() on the per-call path), a
// match without a valid inverse is dropped, and the capture's plan gets the same lenses.
//
// Either way a job runs on libmcs's worker threads and mcs_rig_job_submit returns at once, so a
// caller that keeps several jobs in flight overlaps one capture's estimation with another's.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <memory>
#include <functional>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "hip_rt.h"
#include "mcs_common.h"
#include "mcs_feat_int.h"
#include "mcs_orb_core.h"

namespace {

// Worker threads of libmcs (created on first use, never joined: they sleep on the queue).
class Pool {
public:
    static Pool &get()
    {
        // (sized for three captures in flight: one job's pairs beside two jobs' camera ORBs)
        static Pool *p = new Pool(12);
        return *p;
    }
    void run(std::function<void()> f)
    {
        {
            std::lock_guard<std::mutex> lk(mu_);
            q_.push_back(std::move(f));
        }
        cv_.notify_one();
    }

private:
    explicit Pool(int n)
    {
        for (int i = 0; i < n; i++) std::thread([this] { loop(); }).detach();
    }
    void loop()
    {
        for (;;) {
            std::function<void()> f;
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [this] { return !q_.empty(); });
                f = std::move(q_.front());
                q_.pop_front();
            }
            f();
        }
    }
    std::mutex mu_;
    std::condition_variable cv_;
    std::deque<std::function<void()>> q_;
};

struct Feat {
    std::vector<float> xy;
    std::vector<uint8_t> desc;
    int n = 0;
    int rc = MCS_OK;
    char err[256] = {0};
};

// Device state of the one-launch-chain path (allocated on the job's first capture).
struct RigDevice {
    bool ready = false;
    hipStream_t s = nullptr;
    uint8_t *buf = nullptr;      // device: every per-capture buffer
    uint8_t *host = nullptr;     // pinned: the copy-back blob
    size_t blob_bytes = 0;
    mcs::feat::OrbChain orb;     // the cameras' ORB (orb.K: keypoints per camera at most)
    mcs::feat::KnnShape knn;
    size_t o_cnt = 0, cnt_bytes = 0, o_keys = 0, keys_bytes = 0, o_blob = 0;
    size_t o_sel = 0, o_info = 0, o_hbest = 0, o_mask = 0, o_pts = 0;   // within the blob
    size_t o_lens = 0, o_lpts = 0;   // the lens table (n_cams rows) and mcs_rig_unlens's positions
    mcs::KRigArgs ra;
    // the chain captured as a hipGraph for the frame pointers it was captured with (a job is
    // usually fed the same frame set every time: one per capture slot in flight)
    hipGraphExec_t exec = nullptr;
    std::vector<const uint8_t *> graph_frames;
};

}  // namespace

struct mcs_rig_job {
    int n_cams, w, h, channels;
    // captures per job (mcs_rig_job_create_batch): the chain runs over ci = n_cams x n_caps
    // cameras, capture q's at q n_cams ..; the pairs across a capture boundary are computed with
    // the others and never reported
    int n_caps = 1, ci = 0;
    int nfeatures, nlevels, fast_threshold, iters;
    float scale_factor, ratio;
    double thresh;
    uint32_t seed;
    int device;
    // per submitted capture
    std::vector<const uint8_t *> frames;
    void *wait_event = nullptr;
    std::vector<Feat> feat;
    std::vector<double> H;            // (ci - 1) x 9
    std::vector<int> ok, n_matches, n_inliers;
    std::vector<int> prc;             // per pair status
    std::vector<std::string> perr;
    std::atomic<int> left{0};             // pairs not finished
    std::unique_ptr<std::atomic<int>[]> need;   // per pair: cameras whose ORB is still running
    std::mutex mu;
    std::condition_variable cv;
    bool busy = false, done = true;
    RigDevice dev;
    int captures_device = 0, captures_calls = 0;   // captures finished by each path
    // blend mode of the per-capture plan of wait_stitch (mcs_rig_job_set_blend)
    int blend = MCS_BLEND_NONE;
    // mcs_rig_job_set_multiband: the per-capture plan is a MULTIBAND plan rendered by
    // mcs_stitch_direct_multiband (blend above is kept for when it is switched off); the work area
    // between that call's two launches, the job's, only ever grown
    bool multiband = false;
    void *d_mbwork = nullptr;
    int64_t mbwork_bytes = 0;
    // per-capture exposure gains of wait_stitch (mcs_rig_job_set_exposure): the grid step (< 0:
    // off), the solver's constants, the last call's gains and their q (n_caps x n_cams), and the
    // statistics' buffers (n_caps x (N, S): device and pinned host; allocated on first use)
    int exp_step = -1;
    double exp_alpha = 0.01, exp_beta = 100.0;
    std::vector<double> gains;
    std::vector<uint16_t> gain_q;
    int64_t *d_stats = nullptr, *h_stats = nullptr;
    // per-camera lenses (mcs_rig_job_set_lens): bit c of lens_mask: camera c has one; lens[c] is
    // its row of the device table (uploaded into the job's buffer before the next capture's chain
    // when lens_stale), lens_K / lens_dist / lens_nd / lens_model what the capture's plan is given
    uint32_t lens_mask = 0;
    bool lens_stale = false;
    mcs::Lens lens[MCS_MAX_CAMS];
    double lens_K[MCS_MAX_CAMS][9], lens_dist[MCS_MAX_CAMS][14];
    int lens_nd[MCS_MAX_CAMS], lens_model[MCS_MAX_CAMS];
};

namespace {

// MCS_RIG_PATH=calls: every capture takes the per-call path (read per capture).
bool calls_forced()
{
    const char *e = getenv("MCS_RIG_PATH");
    return e && !strcmp(e, "calls");
}

// A matched position of camera c (a float) through the camera's inverse lens, rounded to float
// again -- what mcs_rig_unlens does on the device; false: no valid inverse, the match is dropped.
bool unlens(const mcs_rig_job *j, int c, float &x, float &y)
{
    c %= j->n_cams;
    if (!((j->lens_mask >> c) & 1u)) return true;
    double u, v;
    if (!mcs::lens_invert(j->lens[c], (double)x, (double)y, u, v)) return false;
    x = (float)u;
    y = (float)v;
    return true;
}

void finish(mcs_rig_job *j)
{
    std::lock_guard<std::mutex> lk(j->mu);
    j->done = true;
    j->cv.notify_all();
}

// Pair k: camera k+1 (query, matchKeypoints' A) against camera k (train, B).
void pair_task(mcs_rig_job *j, int k)
{
    const Feat &fa = j->feat[k + 1], &fb = j->feat[k];
    double *H = j->H.data() + 9 * k;
    for (int i = 0; i < 9; i++) H[i] = 0.0;
    j->ok[k] = 0;
    j->n_matches[k] = j->n_inliers[k] = 0;
    int rc = fa.rc ? fa.rc : fb.rc;
    if (rc == MCS_OK && fa.n > 0 && fb.n > 0) {
        std::vector<int32_t> idx((size_t)fa.n * 2), dist((size_t)fa.n * 2);
        rc = mcs_match_hamming_knn2_host(fa.desc.data(), fa.n, fb.desc.data(), fb.n, idx.data(),
                                         dist.data(), j->device);
        std::vector<float> src, dst;
        if (rc == MCS_OK) {
            // Lowe's ratio, m0.distance < ratio * m1.distance (strict), in double as the
            // reference's Python float compare
            for (int q = 0; q < fa.n; q++) {
                if (idx[2 * q + 1] < 0) continue;
                if (!((double)dist[2 * q] < (double)dist[2 * q + 1] * (double)j->ratio)) continue;
                const int t = idx[2 * q];
                float x = fa.xy[2 * q], y = fa.xy[2 * q + 1], u = fb.xy[2 * t], v = fb.xy[2 * t + 1];
                if (j->lens_mask && !(unlens(j, k + 1, x, y) && unlens(j, k, u, v))) continue;
                src.push_back(x);
                src.push_back(y);
                dst.push_back(u);
                dst.push_back(v);
            }
            j->n_matches[k] = (int)src.size() / 2;
        }
        if (rc == MCS_OK && j->n_matches[k] > 4) {
            int ninl = 0;
            rc = mcs_ransac_homography_host(src.data(), dst.data(), j->n_matches[k], j->thresh,
                                            j->iters, j->seed, H, nullptr, &ninl, j->device);
            if (rc == MCS_OK) {
                j->n_inliers[k] = ninl;
                j->ok[k] = ninl > 0;
            }
        }
    }
    j->prc[k] = rc;
    if (rc != MCS_OK) {
        const char *m = mcs_last_error();
        j->perr[k] = m ? m : "";
    }
    if (j->left.fetch_sub(1) == 1) finish(j);
}

void orb_task(mcs_rig_job *j, int c)
{
    Feat &f = j->feat[c];
    f.rc = MCS_OK;
    f.err[0] = 0;
    const int cap = std::max(j->nfeatures, 1);
    f.xy.resize((size_t)cap * 2);
    f.desc.resize((size_t)cap * 32);
    // the frames' producer (e.g. an upload on the caller's stream): ordered before this
    // thread's ORB stream on the GPU
    if (j->wait_event) f.rc = mcs::features_stream_wait(j->device, j->wait_event);
    if (f.rc == MCS_OK)
        f.rc = mcs_orb_detect_device(j->frames[c], j->w, j->h, j->channels, j->nfeatures,
                                     j->nlevels, j->scale_factor, j->fast_threshold, f.xy.data(),
                                     nullptr, nullptr, nullptr, f.desc.data(), &f.n, j->device);
    if (f.rc != MCS_OK) {
        const char *m = mcs_last_error();
        snprintf(f.err, sizeof(f.err), "%s", m ? m : "");
        f.n = 0;
    }
    // a pair starts as soon as both of its cameras' features are in (pair c - 1 and pair c use
    // camera c)
    for (int k = c - 1; k <= c; k++)
        if (k >= 0 && k < j->ci - 1 && j->need[k].fetch_sub(1) == 1)
            Pool::get().run([j, k] { pair_task(j, k); });
}

// Sizes, offsets, stream and buffers of the device path; the argument blocks that do not change
// between captures (the ORB chain's: mcs::feat::orb_chain).
int device_setup(mcs_rig_job *j, const mcs::rt::Api *A)
{
    RigDevice &d = j->dev;
    mcs::feat::OrbGeom &g = d.orb.geo;
    const int rc = mcs::feat::orb_geom(j->w, j->h, j->nfeatures, j->nlevels, j->scale_factor, &g);
    if (rc) return rc;
    const int C = j->ci, P = j->ci - 1, L = j->nlevels;
    const int K = std::max(g.n_bound, 1);
    const size_t pix = g.off[L];
    size_t o = 0;
    auto take = [&](size_t bytes) {
        const size_t at = o;
        o += (bytes + 255) & ~(size_t)255;
        return at;
    };
    const size_t o_lvl = take(C * pix), o_blur = take(C * pix);
    const size_t o_cand = take(C * g.cap_total * sizeof(mcs::OrbCand));
    d.cnt_bytes = (size_t)C * mcs::kOrbMaxLevels * sizeof(int);
    d.o_cnt = take(d.cnt_bytes);
    const size_t o_kp = take((size_t)C * K * 3 * sizeof(int));
    const size_t o_resp = take((size_t)C * K * sizeof(double));
    const size_t o_desc = take((size_t)C * K * 32);
    const size_t o_or = take((size_t)C * K * 2 * sizeof(double));
    d.keys_bytes = (size_t)P * K * 2 * sizeof(uint32_t);
    d.o_keys = take(d.keys_bytes);
    const size_t o_hyps = take((size_t)P * j->iters * 8 * sizeof(double));
    const size_t o_scores = take((size_t)P * j->iters * sizeof(int32_t));
    d.o_lens = take(sizeof(j->lens));
    d.o_lpts = take((size_t)P * K * 4 * sizeof(double));
    // the copy-back blob, contiguous
    d.o_blob = o;
    size_t b = 0;
    auto btake = [&](size_t bytes) {
        const size_t at = b;
        b += (bytes + 255) & ~(size_t)255;
        return at;
    };
    d.o_sel = btake((size_t)C * 2 * sizeof(int));
    d.o_info = btake((size_t)P * 4 * sizeof(int));
    d.o_hbest = btake((size_t)P * 8 * sizeof(double));
    d.o_mask = btake((size_t)P * K);
    d.o_pts = btake((size_t)P * K * 4 * sizeof(double));
    d.blob_bytes = b;
    o += b;
    HIP_TRY(A->hipStreamCreateWithFlags(&d.s, hipStreamNonBlocking));
    HIP_TRY(A->hipMalloc((void **)&d.buf, o));
    HIP_TRY(A->hipHostMalloc((void **)&d.host, d.blob_bytes, 0));
    uint8_t *B = d.buf, *blob = d.buf + d.o_blob;

    const mcs::feat::OrbBuffers ob = {
        B + o_lvl, B + o_blur, reinterpret_cast<mcs::OrbCand *>(B + o_cand),
        reinterpret_cast<int *>(B + d.o_cnt), reinterpret_cast<int *>(B + o_kp),
        reinterpret_cast<double *>(B + o_resp), B + o_desc,
        reinterpret_cast<double *>(B + o_or), reinterpret_cast<int *>(blob + d.o_sel)};
    mcs::feat::orb_chain(&d.orb, j->w, j->h, j->fast_threshold, C, ob);

    std::memset(&d.ra, 0, sizeof(d.ra));
    d.ra.kp = ob.kp;
    d.ra.desc = ob.desc;
    d.ra.sel = ob.sel;
    d.ra.keys = reinterpret_cast<uint32_t *>(B + d.o_keys);
    d.ra.pts = reinterpret_cast<double *>(blob + d.o_pts);
    d.ra.info = reinterpret_cast<int *>(blob + d.o_info);
    d.ra.hyps = reinterpret_cast<double *>(B + o_hyps);
    d.ra.scores = reinterpret_cast<int32_t *>(B + o_scores);
    d.ra.mask = blob + d.o_mask;
    d.ra.hbest = reinterpret_cast<double *>(blob + d.o_hbest);
    for (int l = 0; l < L; l++) d.ra.lscale[l] = g.lscale[l];
    d.ra.ratio = (double)j->ratio;
    d.ra.t2 = j->thresh * j->thresh;
    d.ra.kstride = K;
    d.ra.iters = j->iters;
    d.ra.seed = j->seed;
    d.ra.lpts = reinterpret_cast<double *>(B + d.o_lpts);
    d.ra.n_cams = j->n_cams;
    j->lens_stale = true;   // (a fresh buffer: the table, if any, is uploaded before the chain)
    // kNN-2 blocks: query waves x train chunks x pairs (as the per-call matcher sizes them)
    d.knn = mcs::feat::knn_shape(K, P, K);
    d.ra.per_chunk = d.knn.per_chunk;
    d.ready = true;
    return MCS_OK;
}

void device_release(mcs_rig_job *j)
{
    RigDevice &d = j->dev;
    const mcs::rt::Api *A = mcs::rt::api();
    if (!A) return;
    mcs::DeviceGuard dg(A, j->device);
    if (d.s) (void)A->hipStreamSynchronize(d.s);
    if (d.exec) (void)A->hipGraphExecDestroy(d.exec);
    if (d.buf) (void)A->hipFree(d.buf);
    if (d.host) (void)A->hipHostFree(d.host);
    if (d.s) (void)A->hipStreamDestroy(d.s);
    d = RigDevice();
    if (j->d_stats) (void)A->hipFree(j->d_stats);
    if (j->h_stats) (void)A->hipHostFree(j->h_stats);
    j->d_stats = j->h_stats = nullptr;
    if (j->d_mbwork) (void)A->hipFree(j->d_mbwork);
    j->d_mbwork = nullptr;
    j->mbwork_bytes = 0;
}

// The job's direct multi-band work area, at least `bytes` (a mosaic larger than any before grows
// it: the one time a capture's stitch allocates).
int multiband_work(mcs_rig_job *j, int64_t bytes)
{
    if (j->d_mbwork && j->mbwork_bytes >= bytes) return MCS_OK;
    const mcs::Entry A(j->device);
    if (A.status) return A.status;
    if (j->d_mbwork) (void)A->hipFree(j->d_mbwork);
    j->d_mbwork = nullptr;
    j->mbwork_bytes = 0;
    HIP_TRY(A->hipMalloc(&j->d_mbwork, (size_t)(bytes > 0 ? bytes : 1)));
    j->mbwork_bytes = bytes;
    return MCS_OK;
}

// The statistics' buffers of a job with exposure enabled: n_caps x (N, S of one frame).
int exposure_buffers(mcs_rig_job *j)
{
    if (j->d_stats && j->h_stats) return MCS_OK;
    const mcs::Entry A(j->device);
    if (A.status) return A.status;
    const size_t bytes = (size_t)j->n_caps * 2 * j->n_cams * j->n_cams * sizeof(int64_t);
    if (!j->d_stats) HIP_TRY(A->hipMalloc((void **)&j->d_stats, bytes));
    if (!j->h_stats) HIP_TRY(A->hipHostMalloc((void **)&j->h_stats, bytes, 0));
    return MCS_OK;
}

// The per-capture resets (candidate counts, kNN-2 keys): stream-ordered memsets issued before
// the chain or its graph (measured: memset nodes captured into the graph did not reset the counts
// on replay -- the ranking then overflowed and every capture fell back to the per-call path).
int enqueue_resets(mcs_rig_job *j, const mcs::rt::Api *A, hipStream_t s)
{
    RigDevice &d = j->dev;
    HIP_TRY(A->hipMemsetAsync(d.buf + d.o_cnt, 0, d.cnt_bytes, s));
    HIP_TRY(A->hipMemsetAsync(d.buf + d.o_keys, 0xff, d.keys_bytes, s));
    return MCS_OK;
}

// The capture's launch chain on stream s (its one copy back included; after enqueue_resets):
// issued directly or recorded into the job's graph.  Every argument block lives in the job (a
// graph's kernel nodes keep their arguments for replays).
int enqueue_chain(mcs_rig_job *j, const mcs::rt::Api *A, const mcs::feat::FeatureKernels *k,
                  hipStream_t s)
{
    RigDevice &d = j->dev;
    using mcs::feat::launch;
    const unsigned P = (unsigned)(j->ci - 1), iters = (unsigned)j->iters;
    int rc = mcs::feat::orb_enqueue(A, k, d.orb, j->frames.data(), j->channels, j->device, s);
    if (rc == MCS_OK)
        rc = launch(A, k->rig_knn2, d.knn.qblocks, d.knn.chunks, mcs::kKnnLanes, &d.ra,
                    sizeof(d.ra), s, P);
    if (rc == MCS_OK && d.ra.lens)
        rc = launch(A, k->rig_unlens, (unsigned)((d.orb.K + 255) / 256), P, 256, &d.ra,
                    sizeof(d.ra), s);
    if (rc == MCS_OK) rc = launch(A, k->rig_match, P, 1, 1024, &d.ra, sizeof(d.ra), s);
    if (rc == MCS_OK)
        rc = launch(A, k->rig_hyp, (iters + 63) / 64, P, 64, &d.ra, sizeof(d.ra), s);
    if (rc == MCS_OK)
        rc = launch(A, k->rig_ransac, iters, P, mcs::kRansacBlock, &d.ra, sizeof(d.ra), s);
    if (rc == MCS_OK) rc = launch(A, k->rig_best, P, 1, 1024, &d.ra, sizeof(d.ra), s);
    if (rc == MCS_OK)
        HIP_TRY(A->hipMemcpyAsync(d.host, d.buf + d.o_blob, d.blob_bytes, hipMemcpyDeviceToHost,
                                  s));
    return rc;
}

// The capture's launch chain and its one copy back (see the file comment).  Returns MCS_OK
// with *overflow set when a camera's device ranking overflowed (nothing else is valid then).
int device_capture(mcs_rig_job *j, bool *overflow)
{
    *overflow = false;
    const mcs::Entry A(j->device);
    if (A.status) return A.status;
    int rc = MCS_OK;
    if (!j->dev.ready && (rc = device_setup(j, A)) != MCS_OK) {
        device_release(j);   // (a partial setup: the next capture starts from clean state)
        return rc;
    }
    RigDevice &d = j->dev;
    const mcs::feat::FeatureKernels *k = nullptr;
    if ((rc = mcs::feat::feature_kernels(A, j->device, &k)) != MCS_OK) return rc;
    const int C = j->ci, P = j->ci - 1;
    hipStream_t s = d.s;
    if (j->wait_event) HIP_TRY(A->hipStreamWaitEvent(s, (hipEvent_t)j->wait_event, 0));
    hipError_t e = hipSuccess;
    if (j->lens_stale) {
        // the lenses changed: the table into the job's buffer (stream-ordered before the chain;
        // the job is not submitted again before this capture ends, so the host rows stay), the
        // kernels' arguments, and the graph that recorded the old ones dropped
        if (j->lens_mask)
            HIP_TRY(A->hipMemcpyAsync(d.buf + d.o_lens, j->lens, sizeof(j->lens),
                                      hipMemcpyHostToDevice, s));
        d.ra.lens = j->lens_mask ? reinterpret_cast<const double *>(d.buf + d.o_lens) : nullptr;
        d.ra.lens_mask = j->lens_mask;
        if (d.exec) (void)A->hipGraphExecDestroy(d.exec);
        d.exec = nullptr;
        j->lens_stale = false;
    }
    if ((rc = enqueue_resets(j, A, s)) != MCS_OK) return rc;
    if (d.orb.pyr_blocks > 0) {
        if (!d.exec || d.graph_frames != j->frames) {
            if (d.exec) (void)A->hipGraphExecDestroy(d.exec);
            d.exec = nullptr;
            hipGraph_t graph = nullptr;
            HIP_TRY(A->hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
            rc = enqueue_chain(j, A, k, s);
            const hipError_t ec = A->hipStreamEndCapture(s, &graph);
            if (rc == MCS_OK && ec != hipSuccess)
                rc = mcs::fail(MCS_E_HIP, "rig capture graph: %s", A->hipGetErrorString(ec));
            if (rc == MCS_OK) {
                const hipError_t ei =
                    A->hipGraphInstantiate(&d.exec, graph, nullptr, nullptr, 0);
                if (ei != hipSuccess) {
                    d.exec = nullptr;
                    rc = mcs::fail(MCS_E_HIP, "rig graph instantiate: %s",
                                   A->hipGetErrorString(ei));
                }
            }
            if (graph) (void)A->hipGraphDestroy(graph);
            if (rc) return rc;
            d.graph_frames = j->frames;
        }
        e = A->hipGraphLaunch(d.exec, s);
    } else {
        rc = enqueue_chain(j, A, k, s);
    }
    const hipError_t e2 = A->hipStreamSynchronize(s);   // (drains the queued work on error too)
    if (rc) return rc;
    if (e != hipSuccess || e2 != hipSuccess)
        return mcs::fail(MCS_E_HIP, "rig capture: %s",
                         A->hipGetErrorString(e != hipSuccess ? e : e2));
    const int *sel = reinterpret_cast<const int *>(d.host + d.o_sel);
    for (int c = 0; c < C; c++)
        if (sel[2 * c + 1]) {
            *overflow = true;
            return MCS_OK;
        }
    const int *info = reinterpret_cast<const int *>(d.host + d.o_info);
    const size_t K = (size_t)d.orb.K;
    const double *hbest = reinterpret_cast<const double *>(d.host + d.o_hbest);
    for (int c = 0; c < C; c++) j->feat[c].n = sel[2 * c], j->feat[c].rc = MCS_OK;
    std::vector<float> src, dst;
    for (int p = 0; p < P; p++) {
        double *H = j->H.data() + 9 * p;
        for (int i = 0; i < 9; i++) H[i] = 0.0;
        const int nm = info[4 * p], score = info[4 * p + 2];
        j->n_matches[p] = nm;
        j->n_inliers[p] = 0;
        j->ok[p] = 0;
        j->prc[p] = MCS_OK;
        if (nm <= 4 || score < 4) continue;
        // findHomography's refinement of the chosen model on its inliers (as
        // mcs_ransac_homography_host): the positions are floats carried as doubles
        const double *pts = reinterpret_cast<const double *>(d.host + d.o_pts) + 4 * p * K;
        src.resize(2 * (size_t)nm);
        dst.resize(2 * (size_t)nm);
        for (int i = 0; i < nm; i++) {
            src[2 * i] = (float)pts[4 * i], src[2 * i + 1] = (float)pts[4 * i + 1];
            dst[2 * i] = (float)pts[4 * i + 2], dst[2 * i + 1] = (float)pts[4 * i + 3];
        }
        for (int i = 0; i < 8; i++) H[i] = hbest[8 * p + i];
        H[8] = 1.0;
        mcs::homography_refine(src.data(), dst.data(), nm, d.host + d.o_mask + p * K, H);
        j->n_inliers[p] = score;
        j->ok[p] = 1;
    }
    return MCS_OK;
}

void start_calls(mcs_rig_job *j)
{
    j->left.store(j->ci - 1);
    for (int k = 0; k < j->ci - 1; k++) j->need[k].store(2);
    for (int c = 0; c < j->ci; c++) Pool::get().run([j, c] { orb_task(j, c); });
}

void capture_task(mcs_rig_job *j)
{
    bool overflow = calls_forced();
    const int rc = overflow ? MCS_OK : device_capture(j, &overflow);
    if (rc == MCS_OK && !overflow) {
        j->captures_device++;
        finish(j);
        return;
    }
    if (rc != MCS_OK) {
        // report through the pairs' status, as the per-call path does
        const char *m = mcs_last_error();
        for (int p = 0; p < j->ci - 1; p++) {
            j->prc[p] = rc;
            j->perr[p] = m ? m : "";
            j->ok[p] = 0;
        }
        for (auto &f : j->feat) f.rc = MCS_OK, f.n = 0;
        finish(j);
        return;
    }
    j->captures_calls++;
    start_calls(j);   // a ranking overflowed: the per-call path (host ranking) for this capture
}

}  // namespace

extern "C" {

int mcs_rig_job_create_batch(int n_cams, int n_captures, int w, int h, int channels,
                             int nfeatures, int nlevels, float scale_factor, int fast_threshold,
                             float ratio, double reproj_thresh, int iters, uint32_t seed,
                             int device, mcs_rig_job **out)
{
    mcs::clear_error();
    if (!out) return mcs::fail(MCS_E_INVALID, "NULL out");
    *out = nullptr;
    if (n_cams < 2 || n_cams > MCS_MAX_CAMS || n_captures < 1 ||
        n_cams * n_captures > MCS_MAX_CAMS || w < 1 || h < 1 ||
        (channels != 1 && channels != 3) || nfeatures < 1 || nlevels < 1 ||
        nlevels > mcs::kOrbMaxLevels || iters < 1 || iters > (1 << 20) ||
        !(ratio > 0.f) || !(reproj_thresh >= 0.0))
        return mcs::fail(MCS_E_INVALID, "n_cams %d x %d captures, %dx%dx%d, nfeatures %d, iters %d",
                         n_cams, n_captures, w, h, channels, nfeatures, iters);
    mcs_rig_job *j = new (std::nothrow) mcs_rig_job();
    if (!j) return mcs::fail(MCS_E_NOMEM, "rig job");
    const int ci = n_cams * n_captures;
    j->n_cams = n_cams, j->n_caps = n_captures, j->ci = ci;
    j->w = w, j->h = h, j->channels = channels;
    j->nfeatures = nfeatures, j->nlevels = nlevels, j->fast_threshold = fast_threshold;
    j->iters = iters, j->scale_factor = scale_factor, j->ratio = ratio;
    j->thresh = reproj_thresh, j->seed = seed, j->device = device;
    j->feat.resize(ci);
    j->H.assign(9 * (size_t)(ci - 1), 0.0);
    j->ok.assign(ci - 1, 0);
    j->n_matches.assign(ci - 1, 0);
    j->n_inliers.assign(ci - 1, 0);
    j->prc.assign(ci - 1, MCS_OK);
    j->perr.assign(ci - 1, std::string());
    j->gains.assign(ci, 1.0);
    j->gain_q.assign(ci, 256);
    j->need.reset(new (std::nothrow) std::atomic<int>[ci - 1]);
    if (!j->need) {
        delete j;
        return mcs::fail(MCS_E_NOMEM, "rig job");
    }
    *out = j;
    return MCS_OK;
}

int mcs_rig_job_create(int n_cams, int w, int h, int channels, int nfeatures, int nlevels,
                       float scale_factor, int fast_threshold, float ratio, double reproj_thresh,
                       int iters, uint32_t seed, int device, mcs_rig_job **out)
{
    return mcs_rig_job_create_batch(n_cams, 1, w, h, channels, nfeatures, nlevels, scale_factor,
                                    fast_threshold, ratio, reproj_thresh, iters, seed, device, out);
}

int mcs_rig_job_submit(mcs_rig_job *j, const uint8_t *const *d_frames, void *wait_event)
{
    mcs::clear_error();
    if (!j || !d_frames) return mcs::fail(MCS_E_INVALID, "NULL job/frames");
    {
        std::lock_guard<std::mutex> lk(j->mu);
        if (j->busy && !j->done) return mcs::fail(MCS_E_INVALID, "job still running");
        j->busy = true;
        j->done = false;
    }
    j->frames.assign(d_frames, d_frames + j->ci);
    j->wait_event = wait_event;
    Pool::get().run([j] { capture_task(j); });
    return MCS_OK;
}

int mcs_rig_job_wait(mcs_rig_job *j, double *H, int *ok, int *n_keypoints, int *n_matches,
                     int *n_inliers)
{
    mcs::clear_error();
    if (!j) return mcs::fail(MCS_E_INVALID, "NULL job");
    {
        std::unique_lock<std::mutex> lk(j->mu);
        if (!j->busy) return mcs::fail(MCS_E_INVALID, "no capture submitted");
        j->cv.wait(lk, [j] { return j->done; });
        j->busy = false;
    }
    // capture q's pair k is chain pair q n_cams + k (the pair across the boundary is skipped)
    const int N = j->n_cams, np = N - 1;
    for (int q = 0; q < j->n_caps; q++)
        for (int k = 0; k < np; k++) {
            const int p = q * N + k, o = q * np + k;
            if (H) std::memcpy(H + 9 * o, j->H.data() + 9 * p, sizeof(double) * 9);
            if (ok) ok[o] = j->ok[p];
            if (n_matches) n_matches[o] = j->n_matches[p];
            if (n_inliers) n_inliers[o] = j->n_inliers[p];
        }
    for (int c = 0; c < j->ci; c++) {
        if (n_keypoints) n_keypoints[c] = j->feat[c].n;
        if (j->feat[c].rc) return mcs::fail(j->feat[c].rc, "camera %d ORB: %s", c, j->feat[c].err);
    }
    for (int q = 0; q < j->n_caps; q++)
        for (int k = 0; k < np; k++) {
            const int p = q * N + k;
            if (j->prc[p]) return mcs::fail(j->prc[p], "pair %d: %s", p, j->perr[p].c_str());
        }
    return MCS_OK;
}

int mcs_rig_job_wait_stitch_batch(mcs_rig_job *j, double *H_io, int *ok_io, int super_mode,
                                  int interp, uint8_t *const *d_out, int64_t out_pitch,
                                  int64_t out_capacity, void *stream, int *out_w, int *out_h,
                                  int *n_keypoints, int *n_matches, int *n_inliers)
{
    mcs::clear_error();
    if (!j || !H_io || !ok_io || !d_out || !out_w || !out_h)
        return mcs::fail(MCS_E_INVALID, "mcs_rig_job_wait_stitch: NULL argument");
    const int N = j->n_cams, np = N - 1;
    std::vector<double> H(9 * (size_t)np * j->n_caps);
    std::vector<int> ok((size_t)np * j->n_caps);
    int rc = mcs_rig_job_wait(j, H.data(), ok.data(), n_keypoints, n_matches, n_inliers);
    if (rc) return rc;
    for (int q = 0; q < j->n_caps; q++)
        if (!d_out[q]) return mcs::fail(MCS_E_INVALID, "mcs_rig_job_wait_stitch: NULL output %d", q);
    int64_t fs[MCS_MAX_CAMS];
    for (int i = 0; i < N; i++) fs[i] = (int64_t)j->w * j->h * j->channels;
    // Capture q's plan: the pairs the job estimated into H_io / ok_io, the chain, the blend mode;
    // the mosaic must fit the output.
    const auto make_plan = [&](int q, mcs_plan **out) -> int {
        // a pair whose estimate failed keeps the caller's -- the previous capture's -- homography
        for (int k = 0; k < np; k++)
            if (ok[q * np + k]) {
                std::memcpy(H_io + 9 * k, H.data() + 9 * ((size_t)q * np + k), sizeof(double) * 9);
                ok_io[k] = 1;
            }
        mcs_stage_desc st[MCS_MAX_CAMS];
        int cw[MCS_MAX_CAMS], ch[MCS_MAX_CAMS];
        for (int c = 0; c < N; c++) cw[c] = j->w, ch[c] = j->h;
        int r = mcs_chain_stages(N, cw, ch, H_io, ok_io, super_mode, st);
        if (r) return r;
        mcs_plan *plan = nullptr;
        r = mcs_plan_create(st, np, j->w, j->h, j->channels, interp, j->device, &plan);
        if (r) return r;
        int w = 0, h = 0, c = 0;
        for (int cam = 0; cam < N && r == MCS_OK; cam++)
            if ((j->lens_mask >> cam) & 1u)
                r = mcs_plan_set_lens_model(plan, cam, j->lens_model[cam], j->lens_K[cam],
                                            j->lens_dist[cam], j->lens_nd[cam]);
        const int blend = j->multiband ? (int)MCS_BLEND_MULTIBAND : j->blend;
        if (r == MCS_OK && blend != MCS_BLEND_NONE) r = mcs_plan_set_blend(plan, blend);
        if (r == MCS_OK) r = mcs_plan_out_shape(plan, &w, &h, &c);
        if (r == MCS_OK && ((int64_t)w * c > out_pitch || (int64_t)h * out_pitch > out_capacity))
            r = mcs::fail(MCS_E_SHAPE, "mosaic %d x %d does not fit the output (pitch %lld, "
                          "%lld bytes)", w, h, (long long)out_pitch, (long long)out_capacity);
        out_w[q] = w;
        out_h[q] = h;
        if (r) {
            mcs_plan_destroy(plan);
            return r;
        }
        *out = plan;
        return MCS_OK;
    };
    // Capture q's stitch: mcs_stitch_direct[_gained], or with set_multiband its multi-band form
    // with the job's work area (the captures of a call run on one stream and share it).
    const auto stitch = [&](int q, mcs_plan *plan, bool gained) -> int {
        const uint8_t *const *cams = j->frames.data() + (size_t)q * N;
        const int64_t ofs = out_pitch * out_h[q];
        if (!j->multiband)
            return (gained ? mcs_stitch_direct_gained : mcs_stitch_direct)(
                plan, cams, fs, d_out[q], out_pitch, ofs, 1, stream);
        int64_t bytes = 0;
        int r = mcs_direct_multiband_work_size(plan, &bytes);
        if (r == MCS_OK) r = multiband_work(j, bytes);
        if (r) return r;
        return (gained ? mcs_stitch_direct_multiband_gained : mcs_stitch_direct_multiband)(
            plan, cams, fs, d_out[q], out_pitch, ofs, 1, j->d_mbwork, j->mbwork_bytes, stream);
    };
    if (j->exp_step < 0) {
        for (int q = 0; q < j->n_caps; q++) {
            mcs_plan *plan = nullptr;
            rc = make_plan(q, &plan);
            if (rc) return rc;
            // (the plan's geometry travels in the kernel arguments: it may go right after the
            // launch)
            rc = stitch(q, plan, false);
            mcs_plan_destroy(plan);
            if (rc) return rc;
        }
        return MCS_OK;
    }
    // Exposure: carrying H_io from capture to capture is host work, so the captures' statistics
    // are all enqueued first (sweep 1), read back with one copy and one synchronise of `stream`,
    // and only then solved and stitched (sweep 2).
    rc = exposure_buffers(j);
    if (rc) return rc;
    const size_t per = 2 * (size_t)N * N;   // N, then S of the capture's one frame
    std::vector<mcs_plan *> plans(j->n_caps, nullptr);
    for (int q = 0; q < j->n_caps && rc == MCS_OK; q++) {
        rc = make_plan(q, &plans[q]);
        if (rc == MCS_OK)
            rc = mcs_plan_overlap_stats_direct_async(plans[q], j->frames.data() + (size_t)q * N, fs,
                                                     1, j->exp_step, j->d_stats + q * per, stream);
    }
    const mcs::rt::Api *A = mcs::rt::api();
    if (rc == MCS_OK) {
        mcs::DeviceGuard dg(A, j->device);
        hipError_t e = dg.err;
        if (e == hipSuccess)
            e = A->hipMemcpyAsync(j->h_stats, j->d_stats, j->n_caps * per * sizeof(int64_t),
                                  hipMemcpyDeviceToHost, (hipStream_t)stream);
        const hipError_t e2 = A->hipStreamSynchronize((hipStream_t)stream);
        if (e != hipSuccess || e2 != hipSuccess)
            rc = mcs::fail(MCS_E_HIP, "rig exposure statistics: %s",
                           A->hipGetErrorString(e != hipSuccess ? e : e2));
    }
    for (int q = 0; q < j->n_caps && rc == MCS_OK; q++) {
        double *g = j->gains.data() + (size_t)q * N;
        const int64_t *st = j->h_stats + q * per;
        rc = mcs_gain_solve_host(N, st, st + (size_t)N * N, j->channels, j->exp_alpha, j->exp_beta, g);
        if (rc == MCS_OK) rc = mcs_plan_set_gains(plans[q], g);
        if (rc == MCS_OK) rc = mcs_plan_gains(plans[q], j->gain_q.data() + (size_t)q * N, nullptr);
        if (rc == MCS_OK) rc = stitch(q, plans[q], true);
    }
    for (mcs_plan *plan : plans) mcs_plan_destroy(plan);
    return rc;
}

int mcs_rig_job_wait_stitch(mcs_rig_job *j, double *H_io, int *ok_io, int super_mode, int interp,
                            uint8_t *d_out, int64_t out_pitch, int64_t out_capacity, void *stream,
                            int *out_w, int *out_h, int *n_keypoints, int *n_matches,
                            int *n_inliers)
{
    if (j && j->n_caps != 1)
        return mcs::fail(MCS_E_INVALID, "mcs_rig_job_wait_stitch: a %d-capture job needs "
                         "mcs_rig_job_wait_stitch_batch", j->n_caps);
    return mcs_rig_job_wait_stitch_batch(j, H_io, ok_io, super_mode, interp, &d_out, out_pitch,
                                         out_capacity, stream, out_w, out_h, n_keypoints,
                                         n_matches, n_inliers);
}

int mcs_rig_job_set_blend(mcs_rig_job *j, int mode)
{
    mcs::clear_error();
    if (!j) return mcs::fail(MCS_E_INVALID, "NULL job");
    if (mode != MCS_BLEND_NONE && mode != MCS_BLEND_SEAM && mode != MCS_BLEND_FEATHER)
        return mcs::fail(MCS_E_INVALID, "blend mode %d: a rig job stitches with the direct path "
                         "(NONE, SEAM or FEATHER)", mode);
    j->blend = mode;
    return MCS_OK;
}

int mcs_rig_job_set_multiband(mcs_rig_job *j, int on)
{
    mcs::clear_error();
    if (!j) return mcs::fail(MCS_E_INVALID, "NULL job");
    j->multiband = on != 0;
    return MCS_OK;
}

int mcs_rig_job_set_exposure(mcs_rig_job *j, int step_log2, double alpha, double beta)
{
    mcs::clear_error();
    if (!j) return mcs::fail(MCS_E_INVALID, "NULL job");
    if (step_log2 > 4) return mcs::fail(MCS_E_INVALID, "step_log2 %d (0..4, or < 0: off)", step_log2);
    if (!std::isfinite(alpha) || !std::isfinite(beta))
        return mcs::fail(MCS_E_INVALID, "alpha / beta");
    j->exp_step = step_log2 < 0 ? -1 : step_log2;
    j->exp_alpha = alpha > 0.0 ? alpha : 0.01;
    j->exp_beta = beta > 0.0 ? beta : 100.0;
    if (j->exp_step < 0) {
        j->gains.assign(j->ci, 1.0);
        j->gain_q.assign(j->ci, 256);
    }
    return MCS_OK;
}

int mcs_rig_job_set_lens(mcs_rig_job *j, int cam, const double *K, const double *dist, int n_dist)
{
    return mcs_rig_job_set_lens_model(j, cam, MCS_LENS_PINHOLE, K, dist, n_dist);
}

int mcs_rig_job_set_lens_model(mcs_rig_job *j, int cam, int model, const double *K,
                               const double *dist, int n_dist)
{
    mcs::clear_error();
    if (!j) return mcs::fail(MCS_E_INVALID, "NULL job");
    if (cam < 0 || cam >= j->n_cams)
        return mcs::fail(MCS_E_INVALID, "camera %d (0..%d)", cam, j->n_cams - 1);
    mcs::Lens L;
    if (K) {
        if (n_dist < 0 || (n_dist > 0 && !dist)) return mcs::fail(MCS_E_INVALID, "NULL dist");
        const int rc = mcs::lens_from(K, dist, n_dist, &L, model);
        if (rc) return rc;
    }
    std::lock_guard<std::mutex> lk(j->mu);
    if (j->busy && !j->done) return mcs::fail(MCS_E_INVALID, "job still running");
    if (K) {
        j->lens[cam] = L;
        std::memcpy(j->lens_K[cam], K, sizeof(j->lens_K[cam]));
        for (int i = 0; i < 14; i++) j->lens_dist[cam][i] = i < n_dist ? dist[i] : 0.0;
        j->lens_nd[cam] = n_dist;
        j->lens_model[cam] = model;
        j->lens_mask |= 1u << cam;
    } else {
        if (!((j->lens_mask >> cam) & 1u)) return MCS_OK;   // none to remove
        j->lens[cam] = mcs::Lens();
        j->lens_mask &= ~(1u << cam);
    }
    j->lens_stale = true;
    return MCS_OK;
}

int mcs_rig_job_gains(const mcs_rig_job *j, double *gains, uint16_t *q, int *enabled)
{
    mcs::clear_error();
    if (!j) return mcs::fail(MCS_E_INVALID, "NULL job");
    if (enabled) *enabled = j->exp_step >= 0 ? 1 : 0;
    for (int i = 0; i < j->ci; i++) {
        if (gains) gains[i] = j->gains[i];
        if (q) q[i] = j->gain_q[i];
    }
    return MCS_OK;
}

int mcs_rig_job_counts(const mcs_rig_job *j, int *device_captures, int *call_captures)
{
    mcs::clear_error();
    if (!j) return mcs::fail(MCS_E_INVALID, "NULL job");
    if (device_captures) *device_captures = j->captures_device;
    if (call_captures) *call_captures = j->captures_calls;
    return MCS_OK;
}

int mcs_rig_job_destroy(mcs_rig_job *j)
{
    if (!j) return MCS_OK;
    {
        std::unique_lock<std::mutex> lk(j->mu);
        j->cv.wait(lk, [j] { return j->done; });   // never free a job the workers still use
    }
    device_release(j);
    delete j;
    return MCS_OK;
}

}  // extern "C"
