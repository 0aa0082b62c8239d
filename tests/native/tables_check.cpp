// CPU check of the plan's table ownership (built and run by tests/test_plan_tables_cpu.py):
// mcs_plan::Tables alloc / drop and release_tables / prepare of mcs_prepare.cpp, linked against
// the stub HIP runtime (stub_hip.h): hipMalloc hands out fake pointers (never dereferenced) and
// can fail on the k-th call, hipFree records what it is given.  Prints "ok" or the failed checks.
#include <cstdio>
#include <set>
#include <vector>

#include "mcs_common.h"
#include "mcs_plan_state.h"
#define STUB_HIP_DEFINE_FAIL   // (mcs_runtime.cpp is not linked)
#include "stub_hip.h"

using mcs::host::Api;
using Tables = mcs_plan::Tables;

static int g_bad = 0;

#define CHECK(cond)                                                                            \
    do {                                                                                       \
        if (!(cond)) {                                                                         \
            printf("line %d: %s\n", __LINE__, #cond);                                          \
            g_bad++;                                                                           \
        }                                                                                      \
    } while (0)

// Every member of Tables (a member added there is added here).
static bool tables_equal(const Tables &a, const Tables &b)
{
#define EQ(m) (a.m == b.m)
    return EQ(owned) && EQ(prepared) && EQ(n_fallback) && EQ(n_big) && EQ(d_big) && EQ(d_tiles) &&
           EQ(d_desc) && EQ(d_desc4) && EQ(d_spans) && EQ(d_fallback) && EQ(d_order) &&
           EQ(n_early) && EQ(n_list) && EQ(n_blend) && EQ(mb_slots) && EQ(n_dense) &&
           EQ(n_degraded) && EQ(d_dense) && EQ(d_owner) && EQ(d_binfo) && EQ(d_blist) &&
           EQ(d_mbdesc) && EQ(d_mbtab) && EQ(d_mbfoot) && EQ(d_mbg1) && EQ(d_mbg2) &&
           EQ(mb_chunk) && EQ(n_bands) && EQ(n_bands_in) && EQ(gxb) && EQ(d_bands) &&
           EQ(d_tile_bt) && EQ(d_bdesc) && EQ(d_bgrp) && EQ(d_bdesc16) && EQ(n_bands_lds) &&
           EQ(mb_mixed_px) && EQ(mb_r1) && EQ(n_strips) && EQ(sw_jb) && EQ(d_strips) &&
           EQ(d_region) && EQ(d_sdesc) && EQ(d_skip) && EQ(sw_px) && EQ(sw_desc_rows) &&
           EQ(dma_bytes) && EQ(box_bytes);
#undef EQ
}

// The allocations of a band-pass multi-band plan, in prepare's order (stops at the first failure).
static hipError_t fill(const Api *A, Tables &t)
{
    hipError_t e = t.alloc(A, &t.d_owner, 100);
    if (e == hipSuccess) e = t.alloc(A, &t.d_binfo, 8);
    if (e == hipSuccess) e = t.alloc(A, &t.d_blist, 20);
    if (e == hipSuccess) e = t.alloc(A, &t.d_mbdesc, 64);
    if (e == hipSuccess) e = t.alloc(A, &t.d_mbg1, 64);
    if (e == hipSuccess) e = t.alloc(A, &t.d_order, 16);
    if (e == hipSuccess) e = t.alloc(A, &t.d_bands, 3);
    if (e == hipSuccess) e = t.alloc(A, &t.d_bdesc16, 3);
    if (e == hipSuccess) e = t.alloc(A, &t.d_tiles, 4);
    if (e == hipSuccess) e = t.alloc(A, &t.d_fallback, 10);
    if (e != hipSuccess) return e;
    t.d_dense = t.d_blist + 11;      // aliases, as prepare_blend / prepare set them
    t.d_big = t.d_fallback + 5;
    t.n_blend = 4, t.mb_slots = 2, t.n_bands = 3, t.n_list = 16, t.mb_r1 = 77, t.prepared = true;
    return hipSuccess;
}
constexpr int kFill = 10;

int main()
{
    const Api *A = stub::api();
    auto &g_live = stub::g.live;
    auto &g_freed = stub::g.freed;
    int &g_mallocs = stub::g.mallocs, &g_bad_free = stub::g.bad_free;
    // (the k-th hipMalloc fails, counted from here; 0: none)
    const auto reset_device = [](int fail_at) { stub::reset(fail_at, true); };

    // (e) a fresh plan: no device allocation, no host memory behind its tables
    reset_device(0);
    {
        mcs_plan *p = new mcs_plan();
        CHECK(g_mallocs == 0 && p->t.owned.capacity() == 0);
        CHECK(tables_equal(p->t, Tables{}));
        delete p;
    }

    // (a) allocations, then release: each freed once, nothing else freed, a fresh Tables after;
    // (d) the aliases d_dense / d_big never reach hipFree
    {
        reset_device(0);
        mcs_plan *p = new mcs_plan();
        p->kp.skip = (const uint8_t *)0x40;
        CHECK(fill(A, p->t) == hipSuccess && g_mallocs == kFill);
        const std::set<void *> allocated = stub::live_set();
        const void *dense = p->t.d_dense, *big = p->t.d_big;
        CHECK(p->t.owned.size() == (size_t)kFill && !allocated.count((void *)dense));
        mcs::host::release_tables(A, p);
        CHECK(g_live.empty() && g_bad_free == 0 && g_freed.size() == (size_t)kFill);
        CHECK(std::set<void *>(g_freed.begin(), g_freed.end()) == allocated);
        for (void *q : g_freed) CHECK(q != dense && q != big);
        CHECK(tables_equal(p->t, Tables{}) && p->t.owned.capacity() == 0);
        CHECK(p->kp.skip == nullptr);
        mcs::host::release_tables(A, p);   // (again: nothing to free)
        CHECK(g_freed.size() == (size_t)kFill);
        delete p;
    }

    // (b) the k-th allocation fails: release leaves nothing outstanding, frees nothing twice
    for (int k = 1; k <= kFill; k++) {
        reset_device(k);
        mcs_plan *p = new mcs_plan();
        CHECK(fill(A, p->t) == hipErrorOutOfMemory);
        CHECK(g_live.size() == (size_t)(k - 1) && p->t.owned.size() == (size_t)(k - 1));
        mcs::host::release_tables(A, p);
        CHECK(g_live.empty() && g_bad_free == 0 && g_freed.size() == (size_t)(k - 1));
        CHECK(tables_equal(p->t, Tables{}));
        delete p;
    }

    // (c) drop, then release: the dropped table is freed once, its pointer nulled; the rest stay
    {
        reset_device(0);
        mcs_plan *p = new mcs_plan();
        CHECK(fill(A, p->t) == hipSuccess);
        void *g1 = p->t.d_mbg1, *order = p->t.d_order;
        p->t.drop(A, &p->t.d_mbg1);
        CHECK(p->t.d_mbg1 == nullptr && g_freed == std::vector<void *>{g1});
        CHECK(p->t.owned.size() == (size_t)(kFill - 1) && p->t.d_order == order);
        p->t.drop(A, &p->t.d_mbg1);   // (a null pointer: nothing happens)
        CHECK(g_freed.size() == 1);
        // replaced, as prepare_bands replaces d_order
        p->t.drop(A, &p->t.d_order);
        CHECK(p->t.alloc(A, &p->t.d_order, 32) == hipSuccess && p->t.d_order != order);
        mcs::host::release_tables(A, p);
        CHECK(g_live.empty() && g_bad_free == 0 && g_freed.size() == (size_t)(kFill + 1));
        delete p;
    }

    // prepare() itself, feather plan on the stub device (no blend tiles come back): every
    // failing allocation leaves the plan as before the call, and the retry prepares it
    {
        reset_device(0);
        mcs_plan *p = new mcs_plan();
        p->fd.out_w = 200, p->fd.out_h = 70, p->fd.channels = 3, p->fd.interp = 1;
        p->fd.n_cams = 2, p->fd.n_stages = 1;
        p->blend = p->kp.blend = MCS_BLEND_FEATHER;
        CHECK(mcs::host::prepare(A, p, nullptr) == MCS_OK && p->t.prepared);
        const int n = g_mallocs;
        CHECK(n >= 9 && g_live.size() == (size_t)n && p->t.owned.size() == (size_t)n);
        mcs::host::release_tables(A, p);
        CHECK(g_live.empty() && g_bad_free == 0);
        for (int k = 1; k <= n; k++) {
            reset_device(k);
            CHECK(mcs::host::prepare(A, p, nullptr) == MCS_E_HIP);
            CHECK(g_live.empty() && g_bad_free == 0 && g_freed.size() == (size_t)(k - 1));
            CHECK(tables_equal(p->t, Tables{}) && p->t.owned.capacity() == 0);
            stub::fail_at(0);
            CHECK(mcs::host::prepare(A, p, nullptr) == MCS_OK && p->t.prepared);
            CHECK(g_live.size() == (size_t)n);
            mcs::host::release_tables(A, p);
            CHECK(g_live.empty() && g_bad_free == 0);
        }
        delete p;
    }

    if (g_bad == 0) printf("ok\n");
    return g_bad ? 1 : 0;
}
