// Host check of the table-free overlap statistics and the rig job's exposure step (built and run
// by tests/test_direct_gain_native_cpu.py): libmcs's host sources on the stub HIP runtime
// (stub_hip.h), which records, in order, every kernel launch (name, grid, block, stream, argument block), every
// stream synchronise, memset and copy.  Checked: mcs_plan_overlap_stats_direct is one memset, one
// mcs_direct_overlap_c<C>_i<I> launch, one copy back and one synchronise, builds no table and
// leaves the plan's own alone; the _async form neither allocates nor synchronises; the grid keeps
// the 32-bit partials of a block from wrapping, up to a 16-camera plan at step 0 on a 65535-wide
// mosaic; a rig job with exposure runs, per wait_stitch_batch of 2 captures, two statistics
// launches, one synchronise of the caller's stream, then two _g stitch launches; with exposure
// off (never set, or set and disabled again) the launch list is the parent's: two mcs_direct_*
// launches and no synchronise of the caller's stream.  Links every host source but hip_rt.cpp and
// mcs_runtime.cpp.  Prints "ok" or the failed checks.
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "mcs_common.h"
#include "mcs_plan_state.h"
#include "stub_hip.h"

using mcs::host::Api;

struct Event {
    char kind;                     // 'L'aunch, 'S'ynchronise, 'M'emset, 'C'opy
    std::string name;
    unsigned gx = 0, gy = 0, gz = 0, bx = 0, by = 0, bz = 0;
    hipStream_t stream = nullptr;
    size_t bytes = 0;
    void *dst = nullptr;
    bool has_ov = false, has_direct = false;
    mcs::KDirectOverlapArgs ov;
    mcs::KDirectArgs da;
};
static int g_bad = 0;
static int &g_mallocs = stub::g.mallocs;
// the rig job's statistics buffers (2 captures x (N, S) of 3 cameras), by their size
static const size_t kJobStatsBytes = 2 * 2 * 3 * 3 * sizeof(int64_t);
static void *job_dstats() { return stub::device_alloc_of(kJobStatsBytes); }
static void *job_hstats() { return stub::pinned_alloc_of(kJobStatsBytes); }

// The stub's log since clear_log(), with the argument blocks this program reads.
static std::vector<Event> g_events;
static void clear_log()
{
    std::lock_guard<std::mutex> lk(stub::g.mu);
    stub::g.log.clear();
    g_events.clear();
}
static const std::vector<Event> &log()
{
    std::lock_guard<std::mutex> lk(stub::g.mu);
    for (size_t i = g_events.size(); i < stub::g.log.size(); i++) {
        const stub::Event &e = stub::g.log[i];
        Event o;
        o.kind = e.kind, o.name = e.name, o.stream = e.stream, o.bytes = e.bytes, o.dst = e.dst;
        o.gx = e.gx, o.gy = e.gy, o.gz = e.gz, o.bx = e.bx, o.by = e.by, o.bz = e.bz;
        if (e.kind == 'L') {
            const bool ov = e.name.rfind("mcs_direct_overlap_", 0) == 0;
            o.has_ov = ov && e.args_as(&o.ov);
            o.has_direct = !ov && e.args_as(&o.da);
        }
        g_events.push_back(o);
    }
    return g_events;
}

// Statistics a capture of the 3-camera job "measured": camera i's mean 80, 100, 125.
static const int kJobCams = 3;
static void fake_stats(int64_t *st)
{
    const int n = kJobCams;
    const int64_t mean[kJobCams] = {80, 100, 125};
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) {
            const int64_t c = i == j ? 1000 : (i - j == 1 || j - i == 1) ? 300 : 0;
            st[i * n + j] = c;
            st[n * n + i * n + j] = c * 3 * mean[i];
        }
}
// the rig job's statistics copy (2 captures x (N, S) of 3 cameras): give the solver overlaps
static void copy_hook(void *dst, size_t n, hipStream_t)
{
    if (n == kJobStatsBytes && dst == job_hstats()) {
        fake_stats((int64_t *)dst);
        fake_stats((int64_t *)dst + 2 * kJobCams * kJobCams);
    }
}

#define CHECK(cond)                                                                            \
    do {                                                                                       \
        if (!(cond)) {                                                                         \
            printf("line %d: %s\n", __LINE__, #cond);                                          \
            g_bad++;                                                                           \
        }                                                                                      \
    } while (0)

static const uint8_t *const CAM[MCS_MAX_CAMS] = {
    (const uint8_t *)(uintptr_t)0x1000000, (const uint8_t *)(uintptr_t)0x1100000,
    (const uint8_t *)(uintptr_t)0x1200000, (const uint8_t *)(uintptr_t)0x1300000,
    (const uint8_t *)(uintptr_t)0x1400000, (const uint8_t *)(uintptr_t)0x1500000,
    (const uint8_t *)(uintptr_t)0x1600000, (const uint8_t *)(uintptr_t)0x1700000,
    (const uint8_t *)(uintptr_t)0x1800000, (const uint8_t *)(uintptr_t)0x1900000,
    (const uint8_t *)(uintptr_t)0x1a00000, (const uint8_t *)(uintptr_t)0x1b00000,
    (const uint8_t *)(uintptr_t)0x1c00000, (const uint8_t *)(uintptr_t)0x1d00000,
    (const uint8_t *)(uintptr_t)0x1e00000, (const uint8_t *)(uintptr_t)0x1f00000};
static hipStream_t const STREAM = (hipStream_t)(uintptr_t)0x5000;

// n cameras of w x h, camera k+1 `shift` pixels to the right of camera k.
static mcs_plan *make_plan(int n, int w, int h, double shift, int channels, int interp)
{
    int cw[MCS_MAX_CAMS], ch[MCS_MAX_CAMS], ok[MCS_MAX_CAMS];
    double Hp[9 * MCS_MAX_CAMS];
    for (int c = 0; c < n; c++) cw[c] = w, ch[c] = h;
    for (int k = 0; k < n - 1; k++) {
        const double t[9] = {1, 0, shift, 0, 1, 0, 0, 0, 1};
        memcpy(Hp + 9 * k, t, sizeof(t));
        ok[k] = 1;
    }
    mcs_stage_desc st[MCS_MAX_CAMS];
    mcs_plan *p = nullptr;
    CHECK(mcs_chain_stages(n, cw, ch, Hp, ok, 0, st) == MCS_OK);
    CHECK(mcs_plan_create(st, n - 1, w, h, channels, interp, 0, &p) == MCS_OK && p);
    return p;
}

// Points the block with the most of them gets in a launch of gx blocks over `points`.
static int64_t block_points(int64_t points, unsigned gx)
{
    const int64_t step = (int64_t)gx * mcs::kDovThreads;
    const int64_t rounds = (points + step - 1) / step;   // (block 0's)
    return rounds * mcs::kDovThreads;
}

static size_t count(char kind, hipStream_t s)
{
    size_t n = 0;
    for (const Event &e : log()) n += e.kind == kind && e.stream == s;
    return n;
}

// The events on the caller's stream STREAM, as a string: L:<kernel> S M C, in order.
static std::string stream_trace()
{
    std::string t;
    for (const Event &e : log()) {
        if (e.stream != STREAM) continue;
        if (e.kind == 'L') t += "L:" + e.name + " ";
        else t += std::string(1, e.kind) + " ";
    }
    return t;
}

int main()
{
    stub::g.copy_hook = copy_hook;

    CHECK(mcs::kDovThreads == 256 && mcs::kOvFrames == 4 && mcs::kDovBlocks == 1024);
    // ---- the grid: enough blocks to fill the chip, more where the partials ask for them
    {
        const int64_t pts[] = {1, 255, 256, 257, 262144, 262145, 1ll << 22, (1ll << 32) - 1,
                               1ll << 32, (1ll << 32) + 1, 65535ll * 65535ll};
        for (int64_t np : pts) {
            const unsigned gx = mcs::dov_blocks(np);
            CHECK(gx >= 1 && (int64_t)gx * mcs::kDovThreads < np + mcs::kDovThreads * 1024ll);
            CHECK(gx >= 1024 || (int64_t)gx * mcs::kDovThreads < np + mcs::kDovThreads);
            CHECK(block_points(np, gx) <= mcs::kDovMaxBlockPoints);
            CHECK(block_points(np, gx) * 4 * 255 < (1ll << 32));
        }
        CHECK(mcs::dov_blocks(65535ll * 65535ll) == 1024);        // (4.29e9 points: 2^22 a block)
        CHECK(mcs::dov_blocks((1ll << 32) + 1) == 1025);
    }

    // ---- the synchronous entry point: memset, one launch, copy, synchronise; no table
    for (int channels = 1; channels <= 3; channels += 2)
        for (int interp = 0; interp < 2; interp++) {
            mcs_plan *p = make_plan(3, 320, 180, 0.7 * 320, channels, interp);
            if (!p) continue;
            int w = 0, h = 0, c = 0;
            CHECK(mcs_plan_out_shape(p, &w, &h, &c) == MCS_OK && w > 2 * 320);
            char name[64];
            snprintf(name, sizeof(name), "mcs_direct_overlap_c%d_i%d", channels, interp);
            const int64_t fs = (int64_t)320 * 180 * channels;
            const int64_t strides[3] = {fs, fs + 5, fs + 48};
            int64_t N[9], S[5 * 9];
            const int ks[3] = {0, 2, 4}, nfs[3] = {1, 4, 5};
            for (int i = 0; i < 3; i++) {
                const int k = ks[i], nf = nfs[i];
                clear_log();
                const int m0 = g_mallocs;
                for (int64_t &v : N) v = -1;
                for (int64_t &v : S) v = -1;
                CHECK(mcs_plan_overlap_stats_direct(p, CAM, strides, nf, k, N, S, STREAM) == MCS_OK);
                CHECK(g_mallocs - m0 <= 1);          // (the thread's accumulators, first call)
                CHECK(stream_trace() == std::string("M L:") + name + " C S ");
                CHECK(log().size() == 4 && p->ov.step == -1 && !p->ov.d_table);
                if (log().size() != 4) continue;
                const Event &ms = log()[0], &l = log()[1], &cp = log()[2];
                const int gw = (w + (1 << k) - 1) >> k, gh = (h + (1 << k) - 1) >> k;
                CHECK(ms.bytes == (size_t)(1 + nf) * 9 * 8 && cp.bytes == ms.bytes);
                CHECK(l.has_ov && l.gx == mcs::dov_blocks((int64_t)gw * gh) &&
                      l.gy == (unsigned)((nf + 3) / 4) && l.gz == 1);
                CHECK(l.bx == 256 && l.by == 1 && l.bz == 1);
                CHECK(l.ov.gw == gw && l.ov.gh == gh && l.ov.k == k && l.ov.n_frames == nf &&
                      l.ov.n_cams == 3 && (void *)l.ov.stats == ms.dst);
                CHECK(l.ov.P.n_stages == 2 && l.ov.P.out_w == w && l.ov.P.out_h == h);
                for (int cam = 0; cam < 3; cam++)
                    CHECK(l.ov.P.cams[cam] == CAM[cam] && l.ov.P.cam_fstride[cam] == strides[cam]);
                CHECK(N[0] == 0 && S[0] == 0 && S[nf * 9 - 1] == 0);   // (the stub copies nothing)
            }
            // NULL strides: dense frames; NULL stream: the plan's own
            clear_log();
            CHECK(mcs_plan_overlap_stats_direct(p, CAM, nullptr, 1, 2, N, S, nullptr) == MCS_OK);
            CHECK(log().size() == 4 && log()[1].has_ov && log()[1].ov.P.cam_fstride[2] == fs &&
                  log()[1].stream == p->stream && p->stream != nullptr);

            // ---- a table the plan has survives the direct call and is not used
            CHECK(mcs_plan_overlap_stats(p, CAM, strides, 1, 2, N, S, STREAM) == MCS_OK);
            // (the stub's counts are zero: the table is empty, its step stands)
            CHECK(p->ov.step == 2);
            clear_log();
            CHECK(mcs_plan_overlap_stats_direct(p, CAM, strides, 1, 1, N, S, STREAM) == MCS_OK);
            CHECK(p->ov.step == 2 && stream_trace() == std::string("M L:") + name + " C S ");

            // ---- the enqueue-only form: memset + launch, no allocation, no synchronise
            clear_log();
            const int m0 = g_mallocs;
            int64_t *const d_stats = (int64_t *)(uintptr_t)0x8000000;
            CHECK(mcs_plan_overlap_stats_direct_async(p, CAM, strides, 5, 2, d_stats, STREAM) ==
                  MCS_OK);
            CHECK(g_mallocs == m0 && stream_trace() == std::string("M L:") + name + " ");
            CHECK(log().size() == 2 && log()[0].dst == (void *)d_stats &&
                  log()[0].bytes == 6 * 9 * 8 && log()[1].gy == 2 &&
                  (void *)log()[1].ov.stats == (void *)d_stats);
            // refused arguments launch nothing
            clear_log();
            CHECK(mcs_plan_overlap_stats_direct_async(p, CAM, strides, 1, 5, d_stats, STREAM) ==
                  MCS_E_INVALID);
            CHECK(mcs_plan_overlap_stats_direct_async(p, CAM, strides, 0, 2, d_stats, STREAM) ==
                  MCS_E_INVALID);
            CHECK(mcs_plan_overlap_stats_direct(p, CAM, strides, 1, -1, N, S, STREAM) ==
                  MCS_E_INVALID);
            CHECK(log().empty());
            CHECK(mcs_plan_destroy(p) == MCS_OK);
        }

    // ---- 16 cameras at step 0 on a 65535-wide mosaic: the partials of a block cannot wrap
    {
        mcs_plan *p = make_plan(16, 4500, 600, 4069.0, 3, 1);
        if (p) {
            int w = 0, h = 0, c = 0;
            CHECK(mcs_plan_out_shape(p, &w, &h, &c) == MCS_OK && w == 65535 && h == 600);
            const size_t count = 2 * 16 * 16;
            std::vector<int64_t> st(count);
            clear_log();
            CHECK(mcs_plan_overlap_stats_direct(p, CAM, nullptr, 1, 0, st.data(), st.data() + 256,
                                                STREAM) == MCS_OK);
            CHECK(log().size() == 4 && log()[1].has_ov);
            if (log().size() == 4 && log()[1].has_ov) {
                const Event &l = log()[1];
                const int64_t np = (int64_t)l.ov.gw * l.ov.gh;
                CHECK(l.ov.gw == 65535 && l.ov.gh == 600 && l.ov.n_cams == 16 && l.ov.k == 0);
                CHECK(l.gx == 1024 && l.gy == 1);
                CHECK(block_points(np, l.gx) * 4 * 255 < (1ll << 32));
                CHECK(log()[0].bytes == count * 8);
            }
            CHECK(mcs_plan_destroy(p) == MCS_OK);
        }
    }

    // ---- the rig job: 3 cameras, 2 captures per job, feather
    {
        const int n = kJobCams, W = 320, H = 180;
        mcs_rig_job *j = nullptr;
        CHECK(mcs_rig_job_create_batch(n, 2, W, H, 3, 500, 4, 1.2f, 20, 0.75f, 3.0, 100, 0, 0,
                                       &j) == MCS_OK && j);
        CHECK(mcs_rig_job_set_exposure(nullptr, 2, 0, 0) == MCS_E_INVALID);
        if (j) {
            CHECK(mcs_rig_job_set_blend(j, MCS_BLEND_FEATHER) == MCS_OK);
            uint8_t *outs[2] = {(uint8_t *)(uintptr_t)0x9000000, (uint8_t *)(uintptr_t)0xa000000};
            const int64_t pitch = 4096, cap = pitch * 1024;
            // one wait_stitch_batch with the caller's homographies (the stub's estimate finds no
            // pair: every pair keeps H_io); returns the caller's stream's events
            const auto capture = [&]() -> std::string {
                double Hio[18] = {1, 0, 0.7 * W, 0, 1, 2, 0, 0, 1, 1, 0, 0.7 * W, 0, 1, -1, 0, 0, 1};
                int okio[2] = {1, 1}, ow[2] = {0, 0}, oh[2] = {0, 0};
                CHECK(mcs_rig_job_submit(j, CAM, nullptr) == MCS_OK);
                const int rc = mcs_rig_job_wait_stitch_batch(j, Hio, okio, 0, 1, outs, pitch, cap,
                                                             STREAM, ow, oh, nullptr, nullptr,
                                                             nullptr);
                CHECK(rc == MCS_OK && ow[0] > 2 * W && ow[1] == ow[0] && oh[0] >= H);
                return stream_trace();
            };
            double g[6];
            uint16_t q[6];
            int on = -1;
            CHECK(mcs_rig_job_gains(j, g, q, &on) == MCS_OK && on == 0 && g[5] == 1.0 && q[0] == 256);

            // exposure never set: the parent's launches, no synchronise of the caller's stream
            clear_log();
            const std::string off = capture();
            CHECK(off == "L:mcs_direct_feather_c3_i1 L:mcs_direct_feather_c3_i1 ");
            CHECK(count('S', STREAM) == 0 && count('M', STREAM) == 0 && count('C', STREAM) == 0);
            CHECK(!job_dstats() && !job_hstats());   // (no statistics buffers without exposure)

            // exposure on
            CHECK(mcs_rig_job_set_exposure(j, 5, 0, 0) == MCS_E_INVALID);
            CHECK(mcs_rig_job_set_exposure(j, 2, 0, 0) == MCS_OK);
            clear_log();
            const std::string want_on =
                "M L:mcs_direct_overlap_c3_i1 M L:mcs_direct_overlap_c3_i1 C S "
                "L:mcs_direct_feather_c3_i1_g L:mcs_direct_feather_c3_i1_g ";
            CHECK(capture() == want_on);
            std::vector<Event> ev;
            for (const Event &e : log())
                if (e.stream == STREAM) ev.push_back(e);
            if (ev.size() == 8) {
                const size_t per = 2 * n * n * sizeof(int64_t);
                CHECK(job_dstats() && ev[0].dst == job_dstats() && ev[0].bytes == per);
                CHECK(ev[2].dst == (void *)((uint8_t *)job_dstats() + per) && ev[2].bytes == per);
                CHECK(ev[1].has_ov && ev[1].ov.k == 2 && ev[1].ov.n_frames == 1 && ev[1].gy == 1 &&
                      ev[1].ov.P.cams[0] == CAM[0] && ev[3].ov.P.cams[0] == CAM[3]);
                CHECK(job_hstats() && ev[4].dst == job_hstats() && ev[4].bytes == 2 * per);
                // the solver's gains of the stub's statistics: brighter cameras come down
                CHECK(mcs_rig_job_gains(j, g, q, &on) == MCS_OK && on == 1);
                CHECK(g[0] > g[1] && g[1] > g[2] && g[3] == g[0] && g[5] == g[2]);
                CHECK(q[0] > 256 && q[2] < 256 && q[3] == q[0]);
                for (int cam = 0; cam < n; cam++) {
                    CHECK(ev[6].has_direct && ev[6].da.P.gain_q[cam] == q[cam]);
                    CHECK(ev[7].has_direct && ev[7].da.P.gain_q[cam] == q[n + cam]);
                }
                CHECK(ev[6].da.P.out == outs[0] && ev[7].da.P.out == outs[1]);
            } else {
                CHECK(ev.size() == 8);
            }
            // a second call reuses the job's buffers
            const int m0 = g_mallocs;
            clear_log();
            CHECK(capture() == want_on && g_mallocs == m0);

            // disabled again: the parent's launches, identity gains reported
            CHECK(mcs_rig_job_set_exposure(j, -1, 0, 0) == MCS_OK);
            clear_log();
            CHECK(capture() == off && count('S', STREAM) == 0);
            CHECK(mcs_rig_job_gains(j, g, q, &on) == MCS_OK && on == 0 && g[0] == 1.0 && q[5] == 256);
            CHECK(mcs_rig_job_destroy(j) == MCS_OK);
        }
    }

    if (g_bad == 0) printf("ok\n");
    return g_bad ? 1 : 0;
}
