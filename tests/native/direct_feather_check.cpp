// Host check of feather on the direct stitch path (built and run by
// tests/test_direct_feather_native_cpu.py): libmcs's host sources on the stub HIP runtime
// (stub_hip.h), which records every kernel launch -- name, grid, block and the KDirectArgs block.  A real chain plan
// (mcs_chain_stages + mcs_plan_create, host only) goes through mcs_stitch_direct and
// mcs_stitch_direct_gained.  Checked: a FEATHER plan launches mcs_direct_feather_c<C>_i<I> over
// every 128 x 16 tile with grid y = ceil(frames / kDirectFrames); the _g twin only when gains
// are active, with the plan's q in the arguments; non-uniform camera strides split the batch into
// per-frame launches with the frame pointers advanced; NONE / SEAM plans launch mcs_direct_* as
// before; a MULTIBAND plan is refused and launches nothing; mcs_rig_job_set_blend's argument
// checks.  Links every host source but hip_rt.cpp and mcs_runtime.cpp.  Prints "ok" or the
// failed checks.
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "mcs_common.h"
#include "mcs_plan_state.h"
#include "stub_hip.h"

using mcs::host::Api;

struct Launch {
    std::string name;
    unsigned gx, gy, gz, bx, by, bz;
    mcs::KDirectArgs a;
    bool has_args;
};
static std::vector<Launch> g_launches;
static int g_bad = 0;

// The launches the stub logged since the log was cleared, into g_launches.
static void collect_launches()
{
    g_launches.clear();
    for (const stub::Event &e : stub::g.log) {
        if (e.kind != 'L') continue;
        Launch l;
        l.name = e.name;
        l.gx = e.gx, l.gy = e.gy, l.gz = e.gz, l.bx = e.bx, l.by = e.by, l.bz = e.bz;
        l.has_args = e.args_as(&l.a);
        g_launches.push_back(l);
    }
}

#define CHECK(cond)                                                                            \
    do {                                                                                       \
        if (!(cond)) {                                                                         \
            printf("line %d: %s\n", __LINE__, #cond);                                          \
            g_bad++;                                                                           \
        }                                                                                      \
    } while (0)

static const int W = 320, H = 180, N = 3;
static const uint8_t *const CAM[3] = {(const uint8_t *)(uintptr_t)0x1000000,
                                      (const uint8_t *)(uintptr_t)0x2000000,
                                      (const uint8_t *)(uintptr_t)0x3000000};
static uint8_t *const OUT = (uint8_t *)(uintptr_t)0x9000000;

// A batch through mcs_stitch_direct[_gained]; the launches land in g_launches.
static int run(mcs_plan *p, int channels, int n_frames, bool gained, const int64_t *strides)
{
    stub::g.log.clear();
    int w = 0, h = 0, c = 0;
    mcs_plan_out_shape(p, &w, &h, &c);
    const int64_t pitch = (int64_t)w * channels;
    const int rc = (gained ? mcs_stitch_direct_gained : mcs_stitch_direct)(
        p, CAM, strides, OUT, pitch, 0, n_frames, nullptr);
    collect_launches();
    return rc;
}

static mcs_plan *make_plan(int channels, int interp)
{
    int cw[N], ch[N], ok[N - 1];
    double Hp[9 * (N - 1)];
    for (int c = 0; c < N; c++) cw[c] = W, ch[c] = H;
    for (int k = 0; k < N - 1; k++) {      // camera k+1 -> camera k: 70 % of a frame to the right
        const double t[9] = {1, 0, 0.7 * W, 0, 1, 3.0, 0, 0, 1};
        memcpy(Hp + 9 * k, t, sizeof(t));
        ok[k] = 1;
    }
    mcs_stage_desc st[MCS_MAX_CAMS];
    mcs_plan *p = nullptr;
    CHECK(mcs_chain_stages(N, cw, ch, Hp, ok, 0, st) == MCS_OK);
    CHECK(mcs_plan_create(st, N - 1, W, H, channels, interp, 0, &p) == MCS_OK && p);
    return p;
}

int main()
{
    for (int channels = 1; channels <= 4; channels += 2)        // 1 and 3
        for (int interp = 0; interp < 2; interp++) {
            mcs_plan *p = make_plan(channels, interp);
            if (!p) continue;
            int w = 0, h = 0, c = 0;
            CHECK(mcs_plan_out_shape(p, &w, &h, &c) == MCS_OK && w > 2 * W && c == channels);
            const unsigned tiles = (unsigned)(((w + mcs::kTileW - 1) / mcs::kTileW) *
                                              ((h + mcs::kTileH - 1) / mcs::kTileH));
            CHECK(mcs::kTileW == 128 && mcs::kTileH == 16 && mcs::kDirectFrames == 4);
            char paste[64], feather[64], feather_g[80];
            snprintf(feather, sizeof(feather), "mcs_direct_feather_c%d_i%d", channels, interp);
            snprintf(feather_g, sizeof(feather_g), "%s_g", feather);
            const int64_t fs = (int64_t)W * H * channels;
            const int64_t dense[N] = {fs, fs, fs}, padded[N] = {fs, fs + 5, fs};

            // ---- NONE and SEAM: the direct-gather kernel, as before
            for (int mode : {MCS_BLEND_NONE, MCS_BLEND_SEAM}) {
                CHECK(mcs_plan_set_blend(p, mode) == MCS_OK);
                CHECK(run(p, channels, 5, false, dense) == MCS_OK && g_launches.size() == 1);
                snprintf(paste, sizeof(paste), "mcs_direct_c%d_i%d_o32", channels, interp);
                if (g_launches.size() == 1) {
                    const Launch &l = g_launches[0];
                    CHECK(l.name == paste && l.gx == tiles && l.gy == 2 && l.a.P.blend == mode);
                }
            }

            // ---- FEATHER: the one-pass kernel over every tile, grid y over blocks of 4 captures
            CHECK(mcs_plan_set_blend(p, MCS_BLEND_FEATHER) == MCS_OK);
            const int nfs[4] = {1, 4, 5, 9};
            for (int nf : nfs) {
                CHECK(run(p, channels, nf, false, dense) == MCS_OK && g_launches.size() == 1);
                if (g_launches.size() != 1) continue;
                const Launch &l = g_launches[0];
                CHECK(l.name == feather);
                CHECK(l.gx == tiles && l.gy == (unsigned)((nf + 3) / 4) && l.gz == 1);
                CHECK(l.bx == 64 && l.by == 8 && l.bz == 1);
                CHECK(l.has_args && l.a.n_frames == nf && l.a.fallback == nullptr);
                CHECK(l.a.P.blend == MCS_BLEND_FEATHER && l.a.P.out == OUT &&
                      l.a.P.out_pitch == (int64_t)w * channels &&
                      l.a.P.out_fstride == (int64_t)w * channels * h);
                for (int i = 0; i < N; i++)
                    CHECK(l.a.P.cams[i] == CAM[i] && l.a.P.cam_fstride[i] == fs);
            }
            CHECK(run(p, channels, 0, false, dense) == MCS_OK && g_launches.empty());

            // ---- the _g twin only with active gains
            CHECK(run(p, channels, 5, true, dense) == MCS_OK && g_launches.size() == 1 &&
                  g_launches[0].name == feather);                         // gains disabled
            const double one[N] = {1.0, 1.0, 1.0}, ga[N] = {1.37, 1.0, 0.61};
            CHECK(mcs_plan_set_gains(p, one) == MCS_OK);
            CHECK(run(p, channels, 5, true, dense) == MCS_OK && g_launches.size() == 1 &&
                  g_launches[0].name == feather);                         // every q = 256
            CHECK(run(p, channels, 5, false, dense) == MCS_E_UNSUPPORTED && g_launches.empty());
            CHECK(mcs_plan_set_gains(p, ga) == MCS_OK);
            CHECK(run(p, channels, 5, true, dense) == MCS_OK && g_launches.size() == 1);
            if (g_launches.size() == 1) {
                const Launch &l = g_launches[0];
                CHECK(l.name == feather_g && l.gx == tiles && l.gy == 2);
                CHECK(l.a.P.gain_q[0] == 351 && l.a.P.gain_q[1] == 256 && l.a.P.gain_q[2] == 156);
            }
            // ... and through the per-frame split
            CHECK(run(p, channels, 3, true, padded) == MCS_OK && g_launches.size() == 3);
            for (const Launch &l : g_launches) CHECK(l.name == feather_g && l.a.P.gain_q[2] == 156);
            CHECK(mcs_plan_set_gains(p, nullptr) == MCS_OK);

            // ---- non-uniform strides: one launch per frame, pointers advanced, one capture each
            CHECK(run(p, channels, 3, false, padded) == MCS_OK && g_launches.size() == 3);
            for (size_t f = 0; f < g_launches.size(); f++) {
                const Launch &l = g_launches[f];
                CHECK(l.name == feather && l.gx == tiles && l.gy == 1 && l.a.n_frames == 1);
                for (int i = 0; i < N; i++) CHECK(l.a.P.cams[i] == CAM[i] + (int64_t)f * padded[i]);
                CHECK(l.a.P.out == OUT + (int64_t)f * w * channels * h);
            }

            // ---- MULTIBAND: refused, nothing launched; bad arguments come first
            CHECK(mcs_plan_set_blend(p, MCS_BLEND_MULTIBAND) == MCS_OK);
            CHECK(run(p, channels, 5, false, dense) == MCS_E_UNSUPPORTED && g_launches.empty());
            CHECK(strstr(mcs_last_error(), "mcs_stitch_device") != nullptr);
            CHECK(run(p, channels, 5, true, dense) == MCS_E_UNSUPPORTED && g_launches.empty());
            CHECK(mcs_plan_set_blend(p, MCS_BLEND_FEATHER) == MCS_OK);
            CHECK(run(p, channels, -1, false, dense) == MCS_E_INVALID && g_launches.empty());
            CHECK(mcs_stitch_direct(p, CAM, dense, OUT, (int64_t)w * channels - 1, 0, 1, nullptr) ==
                  MCS_E_INVALID);
            CHECK(mcs_plan_destroy(p) == MCS_OK);
        }

    // ---- the rig job's blend mode
    {
        mcs_rig_job *j = nullptr;
        CHECK(mcs_rig_job_create(3, 96, 64, 3, 500, 4, 1.2f, 20, 0.75f, 3.0, 100, 0, 0, &j) ==
                  MCS_OK && j);
        CHECK(mcs_rig_job_set_blend(nullptr, MCS_BLEND_FEATHER) == MCS_E_INVALID);
        if (j) {
            CHECK(mcs_rig_job_set_blend(j, MCS_BLEND_FEATHER) == MCS_OK);
            CHECK(mcs_rig_job_set_blend(j, MCS_BLEND_SEAM) == MCS_OK);
            CHECK(mcs_rig_job_set_blend(j, MCS_BLEND_NONE) == MCS_OK);
            CHECK(mcs_rig_job_set_blend(j, MCS_BLEND_MULTIBAND) == MCS_E_INVALID);
            CHECK(mcs_rig_job_set_blend(j, -1) == MCS_E_INVALID);
            CHECK(mcs_rig_job_set_blend(j, 4) == MCS_E_INVALID);
            CHECK(mcs_rig_job_destroy(j) == MCS_OK);
        }
    }

    if (g_bad == 0) printf("ok\n");
    return g_bad ? 1 : 0;
}
