// Host check of the exposure code (built and run by tests/test_gain_native_cpu.py, also with
// -fsanitize=address,undefined): mcs_gain_solve_host, the gain quantiser behind mcs_plan_set_gains,
// the argument checks of mcs_gain_apply_device and the overlap table's life on the stub HIP runtime
// (stub_hip.h: hipMalloc hands out fake pointers that are never dereferenced; read-backs keep
// their zeros, so a table has no entries).  Links mcs_gain.cpp, mcs_prepare.cpp, mcs_sweep_host.cpp and
// mcs_launch.cpp.  Prints "ok" or the failed checks.
#include <cmath>
#include <cstdio>
#include <set>

#include "mcs_common.h"
#include "mcs_plan_state.h"
#define STUB_HIP_DEFINE_FAIL   // (mcs_runtime.cpp is not linked)
#include "stub_hip.h"

using mcs::host::Api;

static int g_bad = 0;
static auto &g_live = stub::g.live;
static int &g_bad_free = stub::g.bad_free;

// Kernel launches so far.
static int launches()
{
    int n = 0;
    for (const stub::Event &e : stub::g.log) n += e.kind == 'L';
    return n;
}

// what the linked sources need of mcs_capi.cpp: the plan's stream and host-path buffers (their
// other callers, mcs_stitch.cpp and mcs_seam.cpp, are not linked either)
int mcs::host::ensure_stream(const Api *, mcs_plan *) { return MCS_OK; }
int mcs::host::ensure_host_buffers(const Api *, mcs_plan *p)
{
    for (int i = 0; i < p->fd.n_cams; i++) p->d_cams[i] = (uint8_t *)(uintptr_t)(0x900000 + i);
    return MCS_OK;
}

#define CHECK(cond)                                                                            \
    do {                                                                                       \
        if (!(cond)) {                                                                         \
            printf("line %d: %s\n", __LINE__, #cond);                                          \
            g_bad++;                                                                           \
        }                                                                                      \
    } while (0)

static bool near(double a, double b) { return std::fabs(a - b) <= 1e-12 * std::fabs(b); }

int main()
{
    // ---- the solver
    {
        // two cameras, 100 common points, means 100 and 200, alpha 0.01, beta 100:
        // A = [[b (n0 + n) + 2a 100^2 n, -2a 100 200 n], [.., b (n1 + n) + 2a 200^2 n]]
        const int64_t N[4] = {400, 100, 100, 300};
        const int64_t S[4] = {3 * 400 * 90, 3 * 100 * 100, 3 * 100 * 200, 3 * 300 * 210};
        double g[2] = {0, 0};
        CHECK(mcs_gain_solve_host(2, N, S, 3, 0.01, 100.0, g) == MCS_OK);
        const double a00 = 100.0 * 500 + 0.02 * 100 * 100 * 100, a01 = -0.02 * 100 * 200 * 100;
        const double a11 = 100.0 * 400 + 0.02 * 200 * 200 * 100, b0 = 100.0 * 500, b1 = 100.0 * 400;
        const double det = a00 * a11 - a01 * a01;
        CHECK(near(g[0], (b0 * a11 - a01 * b1) / det) && near(g[1], (a00 * b1 - a01 * b0) / det));
        CHECK(g[0] > 1.0 && g[1] < 1.0);
        // the full width, one camera without coverage in the middle, all-zero statistics
        int64_t N16[256] = {}, S16[256] = {};
        double g16[MCS_MAX_CAMS];
        CHECK(mcs_gain_solve_host(MCS_MAX_CAMS, N16, S16, 3, 0.01, 100.0, g16) == MCS_OK);
        for (double v : g16) CHECK(v == 1.0);
        for (int i = 0; i < MCS_MAX_CAMS; i++) {
            if (i == 7) continue;
            N16[i * 16 + i] = 1000 + i;
            S16[i * 16 + i] = 3 * (1000 + i) * (100 + i);
            const int j = (i + 1) % MCS_MAX_CAMS;
            if (j == 7 || i == 6) continue;
            N16[i * 16 + j] = N16[j * 16 + i] = 50;
            S16[i * 16 + j] = 3 * 50 * (100 + 5 * i);
            S16[j * 16 + i] = 3 * 50 * (140 - 3 * i);
        }
        CHECK(mcs_gain_solve_host(MCS_MAX_CAMS, N16, S16, 3, 0.01, 100.0, g16) == MCS_OK);
        CHECK(g16[7] == 1.0);
        for (double v : g16) CHECK(std::isfinite(v) && v > 0.5 && v < 2.0);
        CHECK(mcs_gain_solve_host(0, N, S, 3, 0.01, 100.0, g) == MCS_E_INVALID);
        CHECK(mcs_gain_solve_host(MCS_MAX_CAMS + 1, N16, S16, 3, 0.01, 100.0, g16) == MCS_E_INVALID);
        const int64_t Nd[4] = {5, 0, 0, 5};                                    // no prior, no data
        CHECK(mcs_gain_solve_host(2, Nd, Nd, 3, 0.01, 0.0, g) == MCS_E_INVALID);   // singular
    }

    // ---- the quantiser and the plan's gain state
    mcs_plan *p = new mcs_plan();
    p->fd.n_cams = 3, p->fd.n_stages = 2, p->fd.channels = 3, p->fd.interp = 1;
    p->fd.out_w = 40, p->fd.out_h = 30;
    for (int i = 0; i < 3; i++) p->fd.cam_w[i] = 16, p->fd.cam_h[i] = 12;
    p->fd.st[0].cam = 1, p->fd.st[1].cam = 2;
    {
        uint16_t q[MCS_MAX_CAMS] = {};
        int on = -1;
        CHECK(mcs_plan_gains(p, q, &on) == MCS_OK && on == 0 && q[0] == 256 && q[2] == 256);
        const double g0[3] = {0.001953125, 1.001953125, 1.005859375};    // 0.5, 256.5, 257.5
        CHECK(mcs_plan_set_gains(p, g0) == MCS_OK && mcs_plan_gains(p, q, &on) == MCS_OK);
        CHECK(on == 1 && q[0] == 1 && q[1] == 256 && q[2] == 258);
        const double g1[3] = {1e300, 255.998046875, 1e-300};
        CHECK(mcs_plan_set_gains(p, g1) == MCS_OK && mcs_plan_gains(p, q, nullptr) == MCS_OK);
        CHECK(q[0] == 65535 && q[1] == 65535 && q[2] == 1);
        const double bad[3] = {1.0, std::nan(""), 1.0};
        CHECK(mcs_plan_set_gains(p, bad) == MCS_E_INVALID && mcs_plan_gains(p, q, &on) == MCS_OK);
        CHECK(on == 1 && q[0] == 65535);                                  // unchanged
        CHECK(mcs_plan_set_gains(p, nullptr) == MCS_OK && mcs_plan_gains(p, q, &on) == MCS_OK);
        CHECK(on == 0 && q[0] == 256);
    }

    // ---- mcs_gain_apply_device: refused before the device, launched otherwise
    {
        uint8_t *a = (uint8_t *)0x100000;
        CHECK(mcs_gain_apply_device(a, a + 8, 16, 0, 0, 1, 256, 0, nullptr) == MCS_E_INVALID);
        CHECK(mcs_gain_apply_device(a, a, 16, 16, 32, 2, 256, 0, nullptr) == MCS_E_INVALID);
        CHECK(mcs_gain_apply_device(a, a + 30, 16, 21, 0, 2, 256, 0, nullptr) == MCS_E_INVALID);
        CHECK(launches() == 0);
        CHECK(mcs_gain_apply_device(a, a, 16, 21, 21, 3, 300, 0, nullptr) == MCS_OK);
        CHECK(mcs_gain_apply_device(a, a + 64, 16, 21, 0, 3, 300, 0, nullptr) == MCS_OK);
        CHECK(launches() == 2);
    }

    // ---- the overlap table on the stub device: built per step, dropped with the plan's lens
    {
        const uint8_t *cams[3] = {(uint8_t *)0x200000, (uint8_t *)0x300000, (uint8_t *)0x400000};
        int64_t N[9], S[2 * 9];
        const int before = (int)g_live.size();
        CHECK(mcs_plan_overlap_stats(p, cams, nullptr, 2, 2, N, S, nullptr) == MCS_OK);
        CHECK(p->ov.step == 2 && p->ov.n_units == 0 && N[0] == 0 && S[17] == 0);
        CHECK((int)g_live.size() == before);           // (no entries: nothing kept)
        const int before_table = launches();
        CHECK(mcs_plan_overlap_stats(p, cams, nullptr, 1, 2, N, S, nullptr) == MCS_OK);
        CHECK(launches() == before_table);                 // the same step: no second table
        CHECK(mcs_plan_overlap_stats(p, cams, nullptr, 1, 0, N, S, nullptr) == MCS_OK);
        CHECK(p->ov.step == 0 && launches() == before_table + 1);
        CHECK(mcs_plan_overlap_stats_host(p, cams, 3, N, S) == MCS_OK && p->ov.step == 3);
        CHECK(mcs_plan_overlap_stats(p, cams, nullptr, 0, 2, N, S, nullptr) == MCS_E_INVALID);
        CHECK(mcs_plan_overlap_stats(p, cams, nullptr, 1, 5, N, S, nullptr) == MCS_E_INVALID);
        p->single = true;
        CHECK(mcs_plan_overlap_stats(p, cams, nullptr, 1, 2, N, S, nullptr) == MCS_E_UNSUPPORTED);
        p->single = false;
        mcs::host::drop_overlap(stub::api(), p);
        CHECK(p->ov.step == -1 && (int)g_live.size() == before && g_bad_free == 0);
    }
    delete p;

    if (g_bad == 0) printf("ok\n");
    return g_bad ? 1 : 0;
}
