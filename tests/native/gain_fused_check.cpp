// Host check of the fused-gain launch path (built and run by tests/test_gain_fused_native_cpu.py):
// on the stub HIP runtime (stub_hip.h), which records every kernel launch -- the kernel's name and
// its argument block, the KParams at its head -- a hand-made prepared plan goes through launch_stitch
// (mcs_launch.cpp) ungained and gained, in paste, feather and multi-band (levels and band pass)
// form with both side lists.  Checked: the gained launch takes the _g twin of every kernel that
// reads source bytes (the multi-band blend has none) and the ungained launch none; the q in the
// arguments is the plan's q as of the launch; gains_active is the identity fast path's rule; a
// sweep plan is refused before anything is launched.  Links mcs_gain.cpp, mcs_prepare.cpp,
// mcs_sweep_host.cpp and mcs_launch.cpp.  Prints "ok" or the failed checks.
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "mcs_common.h"
#include "mcs_plan_state.h"
#define STUB_HIP_DEFINE_FAIL   // (mcs_runtime.cpp is not linked)
#include "stub_hip.h"

using mcs::host::Api;

struct Launch {
    std::string name;
    uint16_t q[MCS_MAX_CAMS];
};
static std::vector<Launch> g_launches;
static int g_bad = 0;

// The launches the stub logged since the log was cleared, into g_launches: every stitch kernel's
// argument block starts with its KParams.
static void collect_launches()
{
    g_launches.clear();
    for (const stub::Event &e : stub::g.log) {
        if (e.kind != 'L') continue;
        Launch l;
        l.name = e.name;
        if (e.args.size() >= sizeof(mcs::KParams))
            memcpy(l.q, e.args.data() + offsetof(mcs::KParams, gain_q), sizeof(l.q));
        else
            memset(l.q, 0, sizeof(l.q));
        g_launches.push_back(l);
    }
}

// what the linked sources need of mcs_capi.cpp: the plan's stream and host-path buffers (their
// other callers, mcs_stitch.cpp and mcs_seam.cpp, are not linked either)
int mcs::host::ensure_stream(const Api *, mcs_plan *) { return MCS_OK; }
int mcs::host::ensure_host_buffers(const Api *, mcs_plan *) { return MCS_OK; }

#define CHECK(cond)                                                                            \
    do {                                                                                       \
        if (!(cond)) {                                                                         \
            printf("line %d: %s\n", __LINE__, #cond);                                          \
            g_bad++;                                                                           \
        }                                                                                      \
    } while (0)

static bool ends_g(const std::string &n)
{
    return n.size() > 2 && n.compare(n.size() - 2, 2, "_g") == 0;
}
static bool has(const char *name)
{
    for (const Launch &l : g_launches)
        if (l.name == name) return true;
    return false;
}

// One batch of 3 captures through launch_stitch; the launches land in g_launches.
static int run(mcs_plan *p, bool gained)
{
    stub::g.log.clear();
    mcs::KParams kp = p->kp;
    for (int i = 0; i < p->fd.n_cams; i++) {
        kp.cams[i] = (const uint8_t *)(uintptr_t)(0x1000000 * (i + 1));
        kp.cam_fstride[i] = 16 * 12 * 3;
    }
    kp.out = (uint8_t *)(uintptr_t)0x9000000;
    kp.out_pitch = 40 * 3;
    kp.out_fstride = 40 * 3 * 30;
    const int rc = mcs::host::launch_stitch(stub::api(), p, kp, 3, nullptr, gained);
    collect_launches();
    return rc;
}

int main()
{
    // a prepared 3-camera plan (cameras 0 and 2 used, camera 1 bypassed) with one tile on each
    // side list; the tables are fake pointers no stub dereferences
    mcs_plan *p = new mcs_plan();
    p->fd.n_cams = 3, p->fd.n_stages = 1, p->fd.channels = 3, p->fd.interp = 1;
    p->fd.out_w = 40, p->fd.out_h = 30;
    for (int i = 0; i < 3; i++) p->fd.cam_w[i] = 16, p->fd.cam_h[i] = 12;
    p->fd.st[0].cam = 2;
    p->kp.out_w = 40, p->kp.out_h = 30, p->kp.n_stages = 1;
    p->gx = p->gy = 1;
    p->t.prepared = true;
    p->t.n_fallback = 1, p->t.n_big = 1;
    p->t.d_big = (int *)(uintptr_t)0x2000;

    // ---- gains_active: the identity fast path's rule
    {
        CHECK(!mcs::host::gains_active(p));                               // disabled
        const double one[3] = {1.0, 1.0, 1.0};
        CHECK(mcs_plan_set_gains(p, one) == MCS_OK && !mcs::host::gains_active(p));
        const double unused[3] = {1.0, 1.5, 1.0};                         // camera 1 is not sampled
        CHECK(mcs_plan_set_gains(p, unused) == MCS_OK && !mcs::host::gains_active(p));
        const double used[3] = {1.0, 1.0, 0.5};
        CHECK(mcs_plan_set_gains(p, used) == MCS_OK && mcs::host::gains_active(p));
        mcs::KParams kp = {};
        mcs::host::fill_gain_q(p, &kp);
        CHECK(kp.gain_q[0] == 256 && kp.gain_q[2] == 128 && kp.gain_q[3] == 256);
        CHECK(mcs_plan_set_gains(p, nullptr) == MCS_OK);
        mcs::host::fill_gain_q(p, &kp);
        CHECK(kp.gain_q[2] == 256);
    }

    // ---- paste with both side lists: stream, big, direct
    const double ga[3] = {1.37, 1.0, 0.61}, gb[3] = {0.5, 1.0, 2.0};
    {
        CHECK(run(p, false) == MCS_OK && g_launches.size() == 3);
        for (const Launch &l : g_launches) CHECK(!ends_g(l.name));
        CHECK(has("mcs_stream_c3_b32") && has("mcs_stream_big_c3_b32") &&
              has("mcs_direct_c3_i1_o32"));
        CHECK(mcs_plan_set_gains(p, ga) == MCS_OK);
        CHECK(run(p, true) == MCS_OK && g_launches.size() == 3);
        CHECK(has("mcs_stream_c3_b32_g") && has("mcs_stream_big_c3_b32_g") &&
              has("mcs_direct_c3_i1_o32_g"));
        for (const Launch &l : g_launches)
            CHECK(l.q[0] == 351 && l.q[1] == 256 && l.q[2] == 156 && l.q[3] == 256);
        // the gains as of the launch: changed on the plan, the next launch carries the new ones
        CHECK(mcs_plan_set_gains(p, gb) == MCS_OK);
        CHECK(run(p, true) == MCS_OK && g_launches.size() == 3);
        for (const Launch &l : g_launches) CHECK(l.q[0] == 128 && l.q[2] == 512);
        // an ungained launch of the same plan state keeps the ungained kernels
        CHECK(run(p, false) == MCS_OK);
        for (const Launch &l : g_launches) CHECK(!ends_g(l.name));
    }

    // ---- feather
    {
        p->blend = MCS_BLEND_FEATHER;
        p->t.n_blend = 2;
        CHECK(run(p, true) == MCS_OK && has("mcs_feather_c3_i1_g") && !has("mcs_feather_c3_i1"));
        CHECK(run(p, false) == MCS_OK && has("mcs_feather_c3_i1") && !has("mcs_feather_c3_i1_g"));
    }

    // ---- multi-band: levels kernel, then the band pass; degraded tiles take the feather kernel
    {
        p->blend = MCS_BLEND_MULTIBAND;
        p->t.mb_slots = 2, p->t.mb_chunk = 64, p->t.n_dense = 1;
        CHECK(run(p, true) == MCS_OK);
        CHECK(has("mcs_mb_levels_c3_g") && has("mcs_mb_blend_c3_s2") && has("mcs_feather_c3_i1_g"));
        for (const Launch &l : g_launches)
            CHECK(ends_g(l.name) || l.name == "mcs_mb_blend_c3_s2");
        p->t.n_bands = 4, p->t.n_bands_in = 2;
        CHECK(run(p, true) == MCS_OK && has("mcs_mb_bands_all_a_c3_g") &&
              !has("mcs_mb_levels_c3_g"));
        for (const Launch &l : g_launches)
            CHECK((ends_g(l.name) || l.name == "mcs_mb_blend_c3_s2") && l.q[2] == 512);
        CHECK(run(p, false) == MCS_OK && has("mcs_mb_bands_all_a_c3"));
        for (const Launch &l : g_launches) CHECK(!ends_g(l.name));
    }

    // ---- a sweep plan: refused before any launch when gained, launched as ever otherwise
    {
        p->t.n_strips = 1, p->t.sw_jb = 2;
        CHECK(run(p, true) == MCS_E_UNSUPPORTED && g_launches.empty());
        CHECK(run(p, false) == MCS_OK && has("mcs_mb_sweep_a_c3_j2"));
    }
    p->t = mcs_plan::Tables();
    delete p;

    if (g_bad == 0) printf("ok\n");
    return g_bad ? 1 : 0;
}
