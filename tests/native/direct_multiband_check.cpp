// Host check of the direct multi-band path (built and run by
// tests/test_direct_multiband_native_cpu.py): libmcs's host sources on the stub HIP runtime
// (stub_hip.h), which records every kernel launch -- name, grid, block, LDS bytes and the
// KDirectMbArgs block.  A real chain plan (mcs_chain_stages + mcs_plan_create, host only) goes
// through mcs_stitch_direct_multiband and its _gained twin.  Checked: a MULTIBAND plan launches
// mcs_direct_mb_own_c<C>_i<I> over every 128 x 16 tile with grid y = ceil(frames / kDirectFrames),
// then mcs_direct_mb_tile_c<C>_i<I> over (blend tiles, frames) with dmb_lds(C).bytes of LDS, both
// with the caller's work area and the grids in their arguments; the _g twins only when gains are
// active, with the plan's q in the arguments; non-uniform camera strides split the batch into
// per-frame launch pairs with the frame pointers advanced; the refusals launch nothing and the
// early returns make no runtime call; every runtime call failed in turn gives MCS_E_HIP;
// mcs_rig_job_set_multiband's argument checks.  Links every host source but hip_rt.cpp and
// mcs_runtime.cpp.  Prints "ok" or the failed checks.
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "mcs_common.h"
#include "mcs_plan_state.h"
#include "stub_hip.h"

struct Launch {
    std::string name;
    unsigned gx, gy, gz, bx, by, bz, lds;
    mcs::KDirectMbArgs a;
    bool has_args;
};
static std::vector<Launch> g_launches;
static int g_bad = 0;

static void collect_launches()
{
    g_launches.clear();
    for (const stub::Event &e : stub::g.log) {
        if (e.kind != 'L') continue;
        Launch l;
        l.name = e.name;
        l.gx = e.gx, l.gy = e.gy, l.gz = e.gz, l.bx = e.bx, l.by = e.by, l.bz = e.bz, l.lds = e.lds;
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
static void *const WORK = (void *)(uintptr_t)0xA000000;

// A batch through mcs_stitch_direct_multiband[_gained]; the launches land in g_launches.
static int run(mcs_plan *p, int channels, int n_frames, bool gained, const int64_t *strides,
               void *work = WORK, int64_t short_by = 0)
{
    stub::g.log.clear();
    int w = 0, h = 0, c = 0;
    mcs_plan_out_shape(p, &w, &h, &c);
    int64_t need = 0;
    mcs_direct_multiband_work_size(p, &need);
    const int64_t pitch = (int64_t)w * channels;
    const int rc = (gained ? mcs_stitch_direct_multiband_gained : mcs_stitch_direct_multiband)(
        p, CAM, strides, OUT, pitch, 0, n_frames, work, need - short_by, nullptr);
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
    CHECK(mcs::kTileW == 128 && mcs::kTileH == 16 && mcs::kDirectFrames == 4);
    CHECK(mcs::kBlendTileW == 32 && mcs::kBlendTileH == 64 && mcs::kDmbCell == 16);
    CHECK(mcs::direct_mb_work_bytes(1, 1) == 4 && mcs::direct_mb_work_bytes(16, 16) == 4 &&
          mcs::direct_mb_work_bytes(17, 17) == 16 && mcs::direct_mb_work_bytes(0, 5) == 0);
    CHECK(mcs::dmb_lds(4).bytes <= 160 * 1024 && mcs::dmb_lds(1).bytes < mcs::dmb_lds(2).bytes);
    for (int channels = 1; channels <= 4; channels += 2)        // 1 and 3
        for (int interp = 0; interp < 2; interp++) {
            mcs_plan *p = make_plan(channels, interp);
            if (!p) continue;
            int w = 0, h = 0, c = 0;
            CHECK(mcs_plan_out_shape(p, &w, &h, &c) == MCS_OK && w > 2 * W && c == channels);
            int64_t need = -1;
            CHECK(mcs_direct_multiband_work_size(p, &need) == MCS_OK &&
                  need == 4 * (int64_t)((w + 15) / 16) * ((h + 15) / 16));
            const unsigned tiles = (unsigned)(((w + 127) / 128) * ((h + 15) / 16));
            const int gxb = (w + 31) / 32, gyb = (h + 63) / 64;
            char own[64], tile[64], own_g[80], tile_g[80];
            snprintf(own, sizeof(own), "mcs_direct_mb_own_c%d_i%d", channels, interp);
            snprintf(tile, sizeof(tile), "mcs_direct_mb_tile_c%d_i%d", channels, interp);
            snprintf(own_g, sizeof(own_g), "%s_g", own);
            snprintf(tile_g, sizeof(tile_g), "%s_g", tile);
            const int64_t fs = (int64_t)W * H * channels;
            const int64_t dense[N] = {fs, fs, fs}, padded[N] = {fs, fs + 5, fs};

            // ---- any other blend mode: MCS_E_INVALID naming mcs_stitch_direct, nothing launched
            for (int mode : {MCS_BLEND_NONE, MCS_BLEND_SEAM, MCS_BLEND_FEATHER}) {
                CHECK(mcs_plan_set_blend(p, mode) == MCS_OK);
                for (int g = 0; g < 2; g++) {
                    CHECK(run(p, channels, 5, g != 0, dense) == MCS_E_INVALID && g_launches.empty());
                    CHECK(strstr(mcs_last_error(), "mcs_stitch_direct") != nullptr);
                }
                CHECK(run(p, channels, -1, false, dense) == MCS_E_INVALID &&
                      strstr(mcs_last_error(), "n_frames") != nullptr);   // device_kparams first
            }

            // ---- MULTIBAND, uniform strides: the owner pass, then the tile pass
            CHECK(mcs_plan_set_blend(p, MCS_BLEND_MULTIBAND) == MCS_OK);
            const int nfs[4] = {1, 4, 5, 9};
            for (int nf : nfs) {
                CHECK(run(p, channels, nf, false, dense) == MCS_OK && g_launches.size() == 2);
                if (g_launches.size() != 2) continue;
                const Launch &a = g_launches[0], &b = g_launches[1];
                CHECK(a.name == own && b.name == tile);
                CHECK(a.gx == tiles && a.gy == (unsigned)((nf + 3) / 4) && a.gz == 1);
                CHECK(a.bx == 64 && a.by == 8 && a.bz == 1 && a.lds == 0);
                CHECK(b.gx == (unsigned)(gxb * gyb) && b.gy == (unsigned)nf && b.gz == 1);
                CHECK(b.bx == (unsigned)mcs::kDmbTileThreads && b.by == 1 && b.bz == 1);
                CHECK(b.lds == (unsigned)mcs::dmb_lds(channels).bytes);
                for (const Launch &l : g_launches) {
                    CHECK(l.has_args && l.a.n_frames == nf && l.a.cells == (uint32_t *)WORK);
                    CHECK(l.a.gxb == gxb && l.a.gyb == gyb && l.a.cgx == (w + 15) / 16 &&
                          l.a.cgy == (h + 15) / 16);
                    CHECK(l.a.P.blend == MCS_BLEND_MULTIBAND && l.a.P.out == OUT &&
                          l.a.P.out_pitch == (int64_t)w * channels &&
                          l.a.P.out_fstride == (int64_t)w * channels * h);
                    for (int i = 0; i < N; i++)
                        CHECK(l.a.P.cams[i] == CAM[i] && l.a.P.cam_fstride[i] == fs);
                }
                CHECK(memcmp(&a.a, &b.a, sizeof(a.a)) == 0);   // one argument block for both
            }

            // ---- early returns: no runtime call at all
            {
                stub::fail_at(0);
                CHECK(run(p, channels, 0, false, dense) == MCS_OK && g_launches.empty());
                CHECK(run(p, channels, 0, false, dense, nullptr) == MCS_OK);   // nothing to render
                CHECK(run(p, channels, 1, false, dense, nullptr) == MCS_E_INVALID);
                CHECK(strstr(mcs_last_error(), std::to_string(need).c_str()) != nullptr);
                CHECK(run(p, channels, 1, false, dense, WORK, 1) == MCS_E_INVALID);
                CHECK(strstr(mcs_last_error(), std::to_string(need).c_str()) != nullptr);
                CHECK(run(p, channels, 65536, false, dense) == MCS_E_INVALID);
                CHECK(mcs_stitch_direct_multiband(p, CAM, dense, OUT, (int64_t)w * channels - 1, 0,
                                                  1, WORK, need, nullptr) == MCS_E_INVALID);
                CHECK(stub::g.calls == 0 && g_launches.empty());
            }

            // ---- the _g twins only with active gains
            CHECK(run(p, channels, 5, true, dense) == MCS_OK && g_launches.size() == 2 &&
                  g_launches[0].name == own && g_launches[1].name == tile);     // gains disabled
            const double one[N] = {1.0, 1.0, 1.0}, ga[N] = {1.37, 1.0, 0.61};
            CHECK(mcs_plan_set_gains(p, one) == MCS_OK);
            CHECK(run(p, channels, 5, true, dense) == MCS_OK && g_launches.size() == 2 &&
                  g_launches[0].name == own && g_launches[1].name == tile);     // every q = 256
            CHECK(run(p, channels, 5, false, dense) == MCS_E_UNSUPPORTED && g_launches.empty());
            CHECK(mcs_plan_set_gains(p, ga) == MCS_OK);
            CHECK(run(p, channels, 5, true, dense) == MCS_OK && g_launches.size() == 2);
            if (g_launches.size() == 2) {
                CHECK(g_launches[0].name == own_g && g_launches[1].name == tile_g);
                CHECK(g_launches[0].gx == tiles && g_launches[0].gy == 2 && g_launches[1].gy == 5);
                for (const Launch &l : g_launches)
                    CHECK(l.a.P.gain_q[0] == 351 && l.a.P.gain_q[1] == 256 &&
                          l.a.P.gain_q[2] == 156);
            }
            // ... and through the per-frame split
            CHECK(run(p, channels, 3, true, padded) == MCS_OK && g_launches.size() == 6);
            for (size_t i = 0; i < g_launches.size(); i++)
                CHECK(g_launches[i].name == (i % 2 ? tile_g : own_g) &&
                      g_launches[i].a.P.gain_q[2] == 156);
            CHECK(mcs_plan_set_gains(p, nullptr) == MCS_OK);

            // ---- non-uniform strides: a launch pair per frame, pointers advanced, one capture each
            CHECK(run(p, channels, 3, false, padded) == MCS_OK && g_launches.size() == 6);
            for (size_t i = 0; i < g_launches.size(); i++) {
                const Launch &l = g_launches[i];
                const int64_t f = (int64_t)(i / 2);
                CHECK(l.name == (i % 2 ? tile : own) && l.gy == 1 && l.a.n_frames == 1);
                CHECK(l.gx == (i % 2 ? (unsigned)(gxb * gyb) : tiles) && l.a.cells == (uint32_t *)WORK);
                for (int c2 = 0; c2 < N; c2++) CHECK(l.a.P.cams[c2] == CAM[c2] + f * padded[c2]);
                CHECK(l.a.P.out == OUT + f * w * channels * h);
            }

            // ---- every runtime call failed in turn: MCS_E_HIP, then the whole call
            {
                int k = 1, rc = MCS_E_HIP;
                for (; k < 64; k++) {
                    stub::fail_at(k);
                    rc = run(p, channels, 5, false, dense);
                    if (rc == MCS_OK) break;
                    CHECK(rc == MCS_E_HIP && g_launches.size() < 2);
                }
                stub::fail_at(0);
                CHECK(rc == MCS_OK && k >= 3 && g_launches.size() == 2);   // >= two launches fail
            }
            CHECK(mcs_plan_destroy(p) == MCS_OK);
        }

    // ---- a lensed plan uploads its lens table first: every call of that failed in turn, no leak
    {
        mcs_plan *p = make_plan(3, 1);
        const double K[9] = {300, 0, 159.5, 0, 300, 89.5, 0, 0, 1}, dist[5] = {0.05, -0.01, 0, 0, 0};
        CHECK(p && mcs_plan_set_lens(p, 1, K, dist, 5) == MCS_OK);
        CHECK(mcs_plan_set_blend(p, MCS_BLEND_MULTIBAND) == MCS_OK);
        const int64_t fs = (int64_t)W * H * 3, dense[N] = {fs, fs, fs};
        int k = 1, rc = MCS_E_HIP;
        for (; k < 64; k++) {
            stub::fail_at(k);
            rc = run(p, 3, 2, false, dense);
            if (rc == MCS_OK) break;
            CHECK(rc == MCS_E_HIP && g_launches.size() < 2);
        }
        stub::fail_at(0);
        CHECK(rc == MCS_OK && k >= 4 && g_launches.size() == 2);
        if (g_launches.size() == 2)
            CHECK(g_launches[0].a.P.lens_tab != nullptr && g_launches[0].a.P.lens_mask == 2u);
        CHECK(mcs_plan_destroy(p) == MCS_OK);
        CHECK(stub::live_set().empty() && stub::g.bad_free == 0);
    }

    // ---- the rig job's switch
    {
        mcs_rig_job *j = nullptr;
        CHECK(mcs_rig_job_create(3, 96, 64, 3, 500, 4, 1.2f, 20, 0.75f, 3.0, 100, 0, 0, &j) ==
                  MCS_OK && j);
        CHECK(mcs_rig_job_set_multiband(nullptr, 1) == MCS_E_INVALID);
        if (j) {
            CHECK(mcs_rig_job_set_multiband(j, 1) == MCS_OK);
            CHECK(mcs_rig_job_set_blend(j, MCS_BLEND_FEATHER) == MCS_OK);     // kept for later
            CHECK(mcs_rig_job_set_blend(j, MCS_BLEND_MULTIBAND) == MCS_E_INVALID);
            CHECK(mcs_rig_job_set_multiband(j, 0) == MCS_OK);
            CHECK(mcs_rig_job_set_multiband(j, 7) == MCS_OK);
            CHECK(mcs_rig_job_destroy(j) == MCS_OK);
        }
    }

    if (g_bad == 0) printf("ok\n");
    return g_bad ? 1 : 0;
}
