// Host check of the entry points that allocate device memory for the length of one call (built
// and run by tests/test_host_calls_native_cpu.py, also with -fsanitize=address,undefined):
// libmcs's host sources on the stub HIP runtime (stub_hip.h), driven through the C ABI only.
// Five scenarios -- mcs_plan_find_seams, mcs_plan_footprint, mcs_seam_graphcut_device,
// mcs_plan_overlap_stats with a table that is built, replaced and rebuilt after
// mcs_plan_set_lens, and the L2 / Hamming host matchers with mcs_ransac_homography_host -- on a
// 2-camera chain (64 x 48 x 3), a 3-camera cylinder (96 x 32 x 1) and a plan with a 1 x 1 mosaic.
// Two more on the ORB launch chain (mcs_feat_int.h): `orb`, the per-call entry points on a
// 64 x 48 frame (the one-launch pyramid, the resize chain, one level, and a device ranking
// "overflow" that sends the call through host ranking); `rig`, rig jobs on the device path -- a
// 3-camera job captured as a graph, replayed, and re-captured after mcs_rig_job_set_lens, then a
// 2-capture batch job whose 2x pyramid takes plain launches.  One on the entry points that render
// a mosaic: `stitch`, the host-array stitch and the six device forms (prepared, direct and direct
// multi-band, each with its _gained twin) over 3 captures, on every plan in its blend modes, with
// frames back to back and with a stride of its own per camera, without gains and with a gain on
// a used camera (the forms without _gained must refuse such a plan).  The rig job's overflow
// fallback is left out of the injection: it runs the per-call steps on pool threads, whose
// thread-lifetime workspaces make the allocation snapshots depend on which thread ran what.  Per
// scenario:
//   (a) a clean run, its log printed one event a line;
//   (b) for k = 1 .. the clean run's runtime calls: call k fails.  The scenario returns a non-zero
//       status; once the plans are destroyed, the device allocations, streams and pinned
//       allocations are back where they were, nothing freed twice or unknown; a retry without a
//       failure returns MCS_OK with the log of (a).
// A synchronise whose status libmcs discards on purpose -- the drain at the head of a plan-lifetime
// release (release_tables) -- cannot make the call fail: such a k must leave MCS_OK and every
// other event of (a)'s log, and their number per scenario is pinned below.
// Prints "scenario <name>: calls <n>, failed <f>, discarded <d>" per scenario, then "ok" or the
// failed checks.  With the argument --args it prints (a) alone, every launch's argument block in
// hex behind its line: the launch record two builds of libmcs are compared by.  Links every host
// source but hip_rt.cpp and mcs_runtime.cpp.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "mcs.h"
#include "mcs_fparams.h"
#include "stub_hip.h"

static int g_bad = 0;
#define CHECK(cond)                                                                            \
    do {                                                                                       \
        if (!(cond)) {                                                                         \
            printf("line %d: %s\n", __LINE__, #cond);                                          \
            g_bad++;                                                                           \
        }                                                                                      \
    } while (0)

static hipStream_t g_stream = nullptr;     // the caller's stream of the overlap scenario
static int g_armed_calls = 0;              // runtime calls of a run up to its disarm()
static int g_hook_cams = 0;                // copy hook: cameras of the plan at work
static size_t g_hook_cover_bytes = 0;      // copy hook: size of the seam grid's cover copy
static size_t g_hook_orb_bytes = 0;        // copy hook: size of the ORB copy back to "overflow"
static size_t g_hook_scores_bytes = 0;     // copy hook: size of the RANSAC scores' copy
static bool g_print_args = false;          // --args

// Ends the part of a run that failures are injected into (what follows releases the plans).
static void disarm()
{
    g_armed_calls = stub::g.calls;
    stub::fail_at(0);
}

// What the device "computed": overlap counts of every camera pair (so that a table is built) and
// a seam grid that cameras 0 and 1 both cover (so that a pair has a graph to cut).
static void copy_hook(void *dst, size_t bytes, hipStream_t)
{
    if (g_hook_cams > 0 && bytes == mcs::kOvSegs * sizeof(uint32_t)) {
        uint32_t *cnt = (uint32_t *)dst;
        for (int i = 0; i < g_hook_cams; i++)
            for (int j = i; j < g_hook_cams; j++) cnt[i * MCS_MAX_CAMS + j] = i == j ? 70 : 9;
    }
    if (g_hook_cover_bytes && bytes == g_hook_cover_bytes) {
        uint16_t *cov = (uint16_t *)dst;
        for (size_t i = 0; i < bytes / 2; i++) cov[i] = 3;
    }
    if (g_hook_orb_bytes && bytes == g_hook_orb_bytes) {
        // orb_detect's copy back, [counts .. sel]: one candidate on level 0, the overflow flag set
        int *blob = (int *)dst;
        blob[0] = 1;
        blob[(bytes - 256) / sizeof(int) + 1] = 1;
    }
    if (g_hook_scores_bytes && bytes == g_hook_scores_bytes) ((int32_t *)dst)[3] = 5;
}

struct Plans {
    mcs_plan *p[3] = {nullptr, nullptr, nullptr};
    int n_cams[3] = {2, 3, 2};
};

static void make_plans(Plans &P)
{
    {   // a 2-camera chain, 64 x 48 x 3
        const int cw[2] = {64, 64}, ch[2] = {48, 48}, ok[1] = {1};
        const double H[9] = {1, 0, 0.7 * 64, 0, 1, 2, 0, 0, 1};
        mcs_stage_desc st[MCS_MAX_CAMS];
        CHECK(mcs_chain_stages(2, cw, ch, H, ok, 0, st) == MCS_OK);
        CHECK(mcs_plan_create(st, 1, 64, 48, 3, 1, 0, &P.p[0]) == MCS_OK && P.p[0]);
    }
    const auto cylinder = [](int n, int w, int h, int out_w, int out_h, mcs_plan **out) {
        mcs_cyl_camera cams[3];
        for (int c = 0; c < n; c++) {
            const double t = 0.4 * (c - 1), co = std::cos(t), si = std::sin(t);
            const double R[9] = {co, 0, si, 0, 1, 0, -si, 0, co};
            memcpy(cams[c].R, R, sizeof(R));
            cams[c].f = 80, cams[c].cx = w / 2.0, cams[c].cy = h / 2.0;
            cams[c].w = w, cams[c].h = h;
        }
        return mcs_plan_create_cylindrical(cams, n, out_w, out_h, 80.0, out_w / 2.0, out_h / 2.0,
                                           1, 1, 0, out);
    };
    CHECK(cylinder(3, 96, 32, 200, 32, &P.p[1]) == MCS_OK && P.p[1]);   // 3 cameras, 96 x 32 x 1
    CHECK(cylinder(2, 8, 8, 1, 1, &P.p[2]) == MCS_OK && P.p[2]);        // a 1 x 1 mosaic
}

static void destroy_plans(Plans &P)
{
    disarm();
    for (mcs_plan *&p : P.p) {
        CHECK(mcs_plan_destroy(p) == MCS_OK);
        p = nullptr;
    }
}

static std::vector<uint8_t> g_frame(96 * 64 * 3, 17);      // a host frame (larger than any camera)
static const uint8_t *const HOST_CAMS[3] = {g_frame.data(), g_frame.data(), g_frame.data()};
static const uint8_t *const DEV_CAMS[3] = {(const uint8_t *)(uintptr_t)0x1000000,
                                           (const uint8_t *)(uintptr_t)0x2000000,
                                           (const uint8_t *)(uintptr_t)0x3000000};

// ---- the scenarios: each returns the first status that is not MCS_OK
static int run_seams()
{
    Plans P;
    make_plans(P);
    int rc = MCS_OK;
    for (int i = 0; i < 3 && rc == MCS_OK; i++) {
        int w = 0, h = 0, c = 0;
        mcs_plan_out_shape(P.p[i], &w, &h, &c);
        for (int k = 0; k <= 2 && rc == MCS_OK; k += 2) {
            g_hook_cover_bytes = (size_t)((w + (1 << k) - 1) >> k) * ((h + (1 << k) - 1) >> k) * 2;
            rc = mcs_plan_find_seams(P.p[i], HOST_CAMS, MCS_SEAM_GRAPHCUT, k);
        }
        g_hook_cover_bytes = 0;
        if (rc == MCS_OK) rc = mcs_plan_find_seams(P.p[i], nullptr, MCS_SEAM_DISTANCE, 0);
    }
    g_hook_cover_bytes = 0;
    destroy_plans(P);
    return rc;
}

static int run_footprint()
{
    Plans P;
    make_plans(P);
    int rc = MCS_OK;
    for (int i = 0; i < 3 && rc == MCS_OK; i++) {
        int64_t touched[MCS_MAX_CAMS];
        rc = mcs_plan_footprint(P.p[i], touched, MCS_MAX_CAMS);
    }
    destroy_plans(P);
    return rc;
}

static int run_graphcut()
{
    const int gw = 8, gh = 8, n = 2, cn = 3;
    uint8_t lab[gw * gh];
    uint16_t cov[gw * gh];
    std::vector<uint8_t> smp((size_t)gw * gh * n * cn, 100);
    for (int q = 0; q < gw * gh; q++) lab[q] = q % gw < gw / 2 ? 0 : 1, cov[q] = 3;
    int64_t stats[5];
    const int rc = mcs_seam_graphcut_device(n, gw, gh, lab, cov, smp.data(), cn, 0, stats);
    disarm();
    return rc;
}

static int run_overlap()
{
    Plans P;
    make_plans(P);
    int rc = MCS_OK;
    for (int i = 0; i < 3 && rc == MCS_OK; i++) {
        mcs_plan *p = P.p[i];
        g_hook_cams = P.n_cams[i];
        int64_t N[9], S[9];
        const double K[9] = {60, 0, 30, 0, 60, 20, 0, 0, 1}, dist[4] = {0.01, 0, 0, 0};
        rc = mcs_plan_overlap_stats(p, DEV_CAMS, nullptr, 1, 2, N, S, g_stream);
        if (rc == MCS_OK) CHECK(N[0] == 70 && N[1] == 9);       // (the table was built)
        // another step: the table is replaced; a lens: it is dropped and built again
        if (rc == MCS_OK) rc = mcs_plan_overlap_stats(p, DEV_CAMS, nullptr, 1, 1, N, S, g_stream);
        if (rc == MCS_OK) rc = mcs_plan_set_lens(p, 0, K, dist, 4);
        if (rc == MCS_OK) rc = mcs_plan_overlap_stats(p, DEV_CAMS, nullptr, 1, 1, N, S, g_stream);
    }
    g_hook_cams = 0;
    destroy_plans(P);
    return rc;
}

static int run_match()
{
    const int sizes[2][2] = {{1, 1}, {65, 257}};
    int rc = MCS_OK;
    for (int i = 0; i < 2 && rc == MCS_OK; i++) {
        const int nq = sizes[i][0], nt = sizes[i][1], dim = 32;
        std::vector<float> q((size_t)nq * dim, 0.5f), t((size_t)nt * dim, 0.25f);
        std::vector<uint8_t> qb((size_t)nq * 32, 0x5a), tb((size_t)nt * 32, 0xa5);
        std::vector<int32_t> idx((size_t)nq * 2), di((size_t)nq * 2);
        std::vector<float> df((size_t)nq * 2);
        int exact = -1;
        rc = mcs_match_l2_knn2_host(q.data(), nq, t.data(), nt, dim, idx.data(), df.data(),
                                    &exact, 0);
        if (rc == MCS_OK)
            rc = mcs_match_hamming_knn2_host(qb.data(), nq, tb.data(), nt, idx.data(), di.data(), 0);
    }
    // RANSAC: no hypothesis scores 4 (the stub's zeros), then hypothesis 3 scores 5 (mask and model
    // are fetched; the refinement of the all-zero model on no inliers is host arithmetic)
    for (int i = 0; i < 2 && rc == MCS_OK; i++) {
        const int n = 8, iters = 16;
        float src[2 * n], dst[2 * n];
        for (int q = 0; q < 2 * n; q++) src[q] = (float)(7 * q % 13), dst[q] = src[q] + 1.f;
        double H[9];
        uint8_t mask[n];
        int ninl = -1;
        g_hook_scores_bytes = i ? iters * sizeof(int32_t) : 0;
        rc = mcs_ransac_homography_host(src, dst, n, 3.0, iters, 0, H, mask, &ninl, 0);
        if (rc == MCS_OK) CHECK(ninl == (i ? 5 : 0));
    }
    g_hook_scores_bytes = 0;
    disarm();
    return rc;
}

static int run_orb()
{
    const int w = 64, h = 48, cap = 100;
    float xy[2 * cap], resp[cap], ang[cap];
    int lvl[cap], n = -1;
    uint8_t desc[32 * cap];
    // a host BGR frame, 3 levels at 1.2: the one-launch pyramid
    int rc = mcs_orb_detect_host(g_frame.data(), w, h, 3, cap, 3, 1.2f, 20, xy, resp, ang, lvl,
                                 desc, &n, 0);
    // a device gray frame, 3 levels at 2.0: the per-level resize chain
    if (rc == MCS_OK)
        rc = mcs_orb_detect_device(DEV_CAMS[0], w, h, 1, cap, 3, 2.0f, 20, xy, resp, ang, lvl,
                                   desc, &n, 0);
    // one level: no pyramid
    if (rc == MCS_OK)
        rc = mcs_orb_detect_device(DEV_CAMS[1], w, h, 3, cap, 1, 1.2f, 20, xy, resp, ang, lvl,
                                   desc, &n, 0);
    if (rc == MCS_OK) CHECK(n == 0);
    // 8 keypoints asked for, and a copy back that reports an overflowed ranking (copy_hook): the
    // host ranks the one candidate and mcs_orb_describe runs again without the device's count.
    // The copy back: counts, keypoints, descriptors, orientations, responses, [n, overflow],
    // each rounded up to 256 bytes.
    if (rc == MCS_OK) {
        const auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
        g_hook_orb_bytes = up(12 * 4) + up(8 * 12) + up(8 * 32) + up(8 * 16) + up(8 * 8) + up(8);
        rc = mcs_orb_detect_host(g_frame.data(), w, h, 3, 8, 3, 1.2f, 20, xy, resp, ang, lvl, desc,
                                 &n, 0);
        g_hook_orb_bytes = 0;
        if (rc == MCS_OK) {
            CHECK(n == 1 && lvl[0] == 0);
            mcs::KOrbDescArgs da;
            bool seen = false;
            for (const stub::Event &e : stub::g.log)
                if (e.name == "mcs_orb_describe" && e.args_as(&da) && !da.sel)
                    seen = e.gx == 1 && da.n == 1;
            CHECK(seen);
        }
    }
    disarm();
    return rc;
}

static int rig_capture(mcs_rig_job *j, const uint8_t *const *frames)
{
    double H[9 * MCS_MAX_CAMS];
    int ok[MCS_MAX_CAMS], nk[MCS_MAX_CAMS], nm[MCS_MAX_CAMS], ni[MCS_MAX_CAMS];
    const int rc = mcs_rig_job_submit(j, frames, nullptr);
    // (the worker thread makes the capture's runtime calls while this thread waits here: their
    // order, and so the injection's count, is that of one thread)
    return rc ? rc : mcs_rig_job_wait(j, H, ok, nk, nm, ni);
}

static int run_rig()
{
    const uint8_t *six[6];
    for (int c = 0; c < 6; c++) six[c] = DEV_CAMS[c % 3] + 0x100000 * (c / 3);
    mcs_rig_job *a = nullptr, *b = nullptr;
    int rc = mcs_rig_job_create(3, 64, 48, 3, 100, 3, 1.2f, 20, 0.75f, 3.0, 64, 0, 0, &a);
    if (rc == MCS_OK)   // 2 captures of 3 gray cameras, 2x levels: no one-launch pyramid, no graph
        rc = mcs_rig_job_create_batch(3, 2, 64, 48, 1, 100, 3, 2.0f, 20, 0.75f, 3.0, 64, 0, 0, &b);
    // the graph's capture, then its replay; a lens: the graph is dropped and captured again
    for (int i = 0; i < 2 && rc == MCS_OK; i++) rc = rig_capture(a, DEV_CAMS);
    const double K[9] = {60, 0, 32, 0, 60, 24, 0, 0, 1}, dist[4] = {0.01, 0, 0, 0};
    if (rc == MCS_OK) rc = mcs_rig_job_set_lens(a, 1, K, dist, 4);
    if (rc == MCS_OK) rc = rig_capture(a, DEV_CAMS);
    if (rc == MCS_OK) rc = rig_capture(b, six);
    if (rc == MCS_OK) {
        // every capture stayed on the device path (the stub's copy back reports no overflow)
        int dev = -1, calls = -1;
        CHECK(mcs_rig_job_counts(a, &dev, &calls) == MCS_OK && dev == 3 && calls == 0);
        CHECK(mcs_rig_job_counts(b, &dev, &calls) == MCS_OK && dev == 1 && calls == 0);
        int graphs = 0, plain = 0;
        for (const stub::Event &e : stub::g.log) {
            graphs += e.name == "mcs_orb_pyramid" && e.gy == 3 && e.lds > 0;
            plain += e.name == "mcs_resize_c1" && e.gz == 6;
        }
        CHECK(graphs == 2 && plain == 2);   // two captures of the graph; levels 1 and 2 resized
    }
    disarm();
    CHECK(mcs_rig_job_destroy(a) == MCS_OK);
    CHECK(mcs_rig_job_destroy(b) == MCS_OK);
    return rc;
}

// Three captures through the device entry points that take the plan's blend mode: the prepared
// path and the table-free one (mcs_stitch_direct, or the multi-band form with a work area of the
// size it asks for: a fake pointer, as the frames and the mosaic are).  strides: NULL (frames
// back to back, one launch chain per batch) or one stride per camera, no two alike (a chain per
// capture: the only case in which the walk's pointer arithmetic reaches the argument blocks).
// gains: the plan has gains on a used camera -- the forms without _gained must refuse it.
static int stitch_batch(mcs_plan *p, int mode, const int64_t *strides, bool gains)
{
    int w = 0, h = 0, c = 0;
    mcs_plan_out_shape(p, &w, &h, &c);
    uint8_t *const out = (uint8_t *)(uintptr_t)0x8000000;
    void *const work = (void *)(uintptr_t)0x5000000;
    const int64_t pitch = (int64_t)w * c, ofs = strides ? pitch * h + 64 : 0;
    int64_t wb = -1;
    CHECK(mcs_direct_multiband_work_size(p, &wb) == MCS_OK && wb >= 4);
    const bool mb = mode == MCS_BLEND_MULTIBAND;
    int rc = MCS_OK;
    if (gains) {
        CHECK(mcs_stitch_device(p, DEV_CAMS, strides, out, pitch, ofs, 3, g_stream) ==
              MCS_E_UNSUPPORTED);
        CHECK((mb ? mcs_stitch_direct_multiband(p, DEV_CAMS, strides, out, pitch, ofs, 3, work, wb,
                                                g_stream)
                  : mcs_stitch_direct(p, DEV_CAMS, strides, out, pitch, ofs, 3, g_stream)) ==
              MCS_E_UNSUPPORTED);
    } else {
        rc = mcs_stitch_device(p, DEV_CAMS, strides, out, pitch, ofs, 3, g_stream);
        if (rc == MCS_OK)
            rc = mb ? mcs_stitch_direct_multiband(p, DEV_CAMS, strides, out, pitch, ofs, 3, work,
                                                  wb, g_stream)
                    : mcs_stitch_direct(p, DEV_CAMS, strides, out, pitch, ofs, 3, g_stream);
    }
    if (rc == MCS_OK)
        rc = mcs_stitch_device_gained(p, DEV_CAMS, strides, out, pitch, ofs, 3, g_stream);
    if (rc == MCS_OK)
        rc = mb ? mcs_stitch_direct_multiband_gained(p, DEV_CAMS, strides, out, pitch, ofs, 3, work,
                                                     wb, g_stream)
                : mcs_stitch_direct_gained(p, DEV_CAMS, strides, out, pitch, ofs, 3, g_stream);
    return rc;
}

// The chain in its four blend modes, the cylinder and the 1 x 1 mosaic in two of theirs (a
// cylinder has no paste order).  Per mode: the host-array stitch, then stitch_batch with both
// kinds of strides, all of it once without gains and once with a gain on camera 1.
static int run_stitch()
{
    Plans P;
    make_plans(P);
    static const int modes[3][4] = {
        {MCS_BLEND_NONE, MCS_BLEND_SEAM, MCS_BLEND_FEATHER, MCS_BLEND_MULTIBAND},
        {MCS_BLEND_FEATHER, MCS_BLEND_MULTIBAND, -1, -1},
        {MCS_BLEND_SEAM, MCS_BLEND_MULTIBAND, -1, -1}};
    const int64_t strides[3] = {0x10000, 0x10100, 0x10200};
    const double gains[3] = {1.0, 1.5, 1.0};
    std::vector<uint8_t> mosaic(256 * 64 * 3);    // (larger than any mosaic)
    int rc = MCS_OK;
    for (int i = 0; i < 3 && rc == MCS_OK; i++)
        for (int m = 0; m < 4 && modes[i][m] >= 0 && rc == MCS_OK; m++) {
            mcs_plan *p = P.p[i];
            rc = mcs_plan_set_blend(p, modes[i][m]);
            for (int g = 0; g < 2 && rc == MCS_OK; g++) {
                CHECK(mcs_plan_set_gains(p, g ? gains : nullptr) == MCS_OK);
                rc = mcs_stitch_host(p, HOST_CAMS, mosaic.data());
                if (rc == MCS_OK) rc = stitch_batch(p, modes[i][m], nullptr, g);
                if (rc == MCS_OK) rc = stitch_batch(p, modes[i][m], strides, g);
            }
            CHECK(mcs_plan_set_gains(p, nullptr) == MCS_OK);
        }
    destroy_plans(P);
    return rc;
}

struct Snapshot {
    size_t live, pinned, streams, events, graphs, execs;
    int bad_free;
    bool operator==(const Snapshot &o) const
    {
        return live == o.live && pinned == o.pinned && streams == o.streams &&
               events == o.events && graphs == o.graphs && execs == o.execs &&
               bad_free == o.bad_free;
    }
};
static Snapshot snapshot()
{
    const stub::State &g = stub::g;
    return {g.live.size(),   g.pinned.size(), g.streams.size(), g.events.size(),
            g.graphs.size(), g.execs.size(),  g.bad_free};
}

// One run with call k failing (0: none); the log is that run's alone.
static int run_with(int (*run)(), int k)
{
    stub::g.log.clear();
    stub::fail_at(k);
    const int rc = run();
    stub::fail_at(0);
    return rc;
}

static void scenario(const char *name, int (*run)(), int want_discarded)
{
    // first use: the kernel handles, the calling thread's feature workspace (kept by design)
    CHECK(run_with(run, 0) == MCS_OK);
    const Snapshot base = snapshot();
    CHECK(base.bad_free == 0);
    // (a)
    CHECK(run_with(run, 0) == MCS_OK && snapshot() == base);
    const int calls = g_armed_calls;
    const std::vector<std::string> clean = stub::log_lines();
    // the clean run's call k: its kind and its line of the log (-1: a call that is not logged)
    std::vector<char> kind(calls + 1, 0);
    std::vector<int> line(calls + 1, -1);
    for (size_t i = 0; i < stub::g.log.size(); i++) {
        const stub::Event &e = stub::g.log[i];
        if (e.call >= 1 && e.call <= calls) kind[e.call] = e.kind, line[e.call] = (int)i;
    }
    printf("== %s: %d runtime calls, %zu events\n", name, calls, clean.size());
    for (size_t i = 0; i < clean.size(); i++) {
        printf("%s", clean[i].c_str());
        if (g_print_args && !stub::g.log[i].args.empty()) {
            printf(" : ");
            for (const uint8_t byte : stub::g.log[i].args) printf("%02x", byte);
        }
        printf("\n");
    }
    if (g_print_args) return;
    // (b)
    int failed = 0, discarded = 0;
    for (int k = 1; k <= calls; k++) {
        const int rc = run_with(run, k);
        const bool cleaned = snapshot() == base;
        bool as_clean = true;
        if (rc == MCS_OK) {
            discarded++;
            printf("%s, call %d fails: MCS_OK (discarded)\n", name, k);
            std::vector<std::string> rest = clean;      // (the failed call itself is not logged)
            if (line[k] >= 0) rest.erase(rest.begin() + line[k]);
            as_clean = kind[k] == 'S' && stub::log_lines() == rest;
        } else {
            failed++;
        }
        const bool retry = run_with(run, 0) == MCS_OK && stub::log_lines() == clean &&
                           snapshot() == base;
        if (!cleaned || !as_clean || !retry) {
            printf("%s, call %d fails: status %d%s%s%s\n", name, k, rc,
                   cleaned ? "" : ", something left allocated or freed twice",
                   as_clean ? "" : ", MCS_OK although the call's result was needed",
                   retry ? "" : ", the retry differs from the clean run");
            g_bad++;
        }
    }
    printf("scenario %s: calls %d, failed %d, discarded %d\n", name, calls, failed, discarded);
    CHECK(discarded == want_discarded);
}

int main(int argc, char **argv)
{
    g_print_args = argc > 1 && !strcmp(argv[1], "--args");
    CHECK(stub::hipStreamCreateWithFlags(&g_stream, 0) == hipSuccess);
    stub::g.copy_hook = copy_hook;
    // mcs_plan_find_seams begins with release_tables, which drains the plan's stream once the
    // plan has one: the second graph cut and the return to distance seams of each of the 3 plans
    scenario("seams", run_seams, 6);
    scenario("footprint", run_footprint, 0);
    scenario("graphcut", run_graphcut, 0);
    scenario("overlap", run_overlap, 0);
    scenario("match", run_match, 0);
    scenario("orb", run_orb, 0);
    // (the jobs are released after the injected part, as the plans are)
    scenario("rig", run_rig, 0);
    // mcs_plan_set_blend on a prepared plan begins with release_tables, which drains the plan's own
    // stream (the host-array stitch made it; on the stub no plan comes to side streams): the
    // chain's three changes of mode, and the second mode of the cylinder and of the 1 x 1 mosaic
    // (their first is set before anything was prepared)
    scenario("stitch", run_stitch, 5);
    if (g_bad == 0) printf("ok\n");
    return g_bad ? 1 : 0;
}
