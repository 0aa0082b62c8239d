// Host check of the call-scoped owner of temporary memory (csrc/mcs_scratch.h; built and run by
// tests/test_host_calls_native_cpu.py, also with -fsanitize=address,undefined) on the stub HIP
// runtime (stub_hip.h): what it allocates is freed exactly once when it goes out of scope; keep()
// takes a pointer out; a failing allocation at any position leaves nothing outstanding and frees
// nothing twice; the destructor synchronises the stream once, before the first free, unless a
// synchronise through sync() / synced() succeeded since the last allocation; an owner that never
// allocated calls nothing.  Links no library source.  Prints "ok" or the failed checks.
#include <cstdio>

#include "mcs_common.h"
#include "mcs_scratch.h"
#define STUB_HIP_DEFINE_FAIL   // (mcs_runtime.cpp is not linked)
#include "stub_hip.h"

static int g_bad = 0;
#define CHECK(cond)                                                                            \
    do {                                                                                       \
        if (!(cond)) {                                                                         \
            printf("line %d: %s\n", __LINE__, #cond);                                          \
            g_bad++;                                                                           \
        }                                                                                      \
    } while (0)

static hipStream_t const STREAM = (hipStream_t)(uintptr_t)0x5000;
constexpr int kAllocs = 5;

// A call in the library's style: kAllocs allocations (device and pinned), the first failure
// returns.  *kept: the fourth allocation, taken out of the owner.
static int five(const mcs::rt::Api *A, uint8_t **kept)
{
    mcs::Scratch sc(A, STREAM);
    uint8_t *a = nullptr, *d = nullptr;
    int32_t *b = nullptr, *c = nullptr;
    double *e = nullptr;
    HIP_TRY(sc.dev(&a, 100));
    HIP_TRY(sc.pinned(&b, 2));
    HIP_TRY(sc.dev(&c, 7));
    HIP_TRY(sc.dev(&d, 1));
    *kept = sc.keep(d);
    HIP_TRY(sc.pinned(&e, 3));
    b[1] = 5, e[2] = 1.0;      // (pinned memory is host memory of the size asked for)
    HIP_TRY_AS("five", sc.sync());
    return MCS_OK;
}

static size_t syncs()
{
    size_t n = 0;
    for (const stub::Event &e : stub::g.log) n += e.kind == 'S';
    return n;
}

int main()
{
    const mcs::rt::Api *A = stub::api();
    stub::State &g = stub::g;

    // allocate, then destroy: each pointer freed once, device and pinned
    stub::reset();
    {
        mcs::Scratch sc(A, STREAM);
        uint8_t *a = nullptr;
        float *b = nullptr;
        uint16_t *h = nullptr;
        CHECK(sc.dev(&a, 10) == hipSuccess && sc.dev(&b, 4) == hipSuccess && a && b);
        CHECK(sc.pinned(&h, 8) == hipSuccess && h && h[7] == 0);
        CHECK(g.live.size() == 2 && g.live[b] == 16 && g.pinned.size() == 1 && g.pinned[h] == 16);
        CHECK(g.releases == 0);
    }
    CHECK(g.live.empty() && g.pinned.empty() && g.bad_free == 0 && g.releases == 3);
    CHECK(g.freed.size() == 2);

    // keep(): the pointer survives the owner and is not freed; the others are
    stub::reset();
    uint8_t *kept = nullptr;
    {
        mcs::Scratch sc(A, STREAM);
        uint8_t *a = nullptr, *b = nullptr, *c = nullptr;
        CHECK(sc.dev(&a, 1) == hipSuccess && sc.dev(&b, 2) == hipSuccess &&
              sc.dev(&c, 3) == hipSuccess);
        kept = sc.keep(b);
        CHECK(kept == b && sc.keep(b) == b);                   // (again: nothing happens)
        CHECK(sc.keep((uint8_t *)nullptr) == nullptr);
    }
    CHECK(g.live.size() == 1 && g.live.count(kept) && g.bad_free == 0 && g.freed.size() == 2);
    for (void *q : g.freed) CHECK(q != kept);

    // the k-th allocation fails: nothing outstanding but what was kept, nothing freed twice
    for (int k = 1; k <= kAllocs; k++) {
        stub::reset(k);
        kept = nullptr;
        CHECK(five(A, &kept) == MCS_E_HIP);
        CHECK((kept != nullptr) == (k > 4));
        CHECK(g.live.size() == (kept ? 1u : 0u) && g.pinned.empty() && g.bad_free == 0);
        CHECK(g.releases == k - 1 - (kept ? 1 : 0));
        CHECK(syncs() == (k > 1 ? 1u : 0u));                   // (drained before the frees)
        for (const stub::Event &e : g.log) CHECK(e.kind == 'S' && e.releases == 0);
    }
    stub::reset();
    CHECK(five(A, &kept) == MCS_OK && g.live.size() == 1 && g.pinned.empty() && g.bad_free == 0);
    CHECK(syncs() == 1 && g.releases == kAllocs - 1);          // (its own synchronise, no other)
    // ... and when that synchronise fails (call kAllocs + 1): one more, before the first free
    stub::reset(kAllocs + 1);
    CHECK(five(A, &kept) == MCS_E_HIP && g.live.size() == 1 && g.pinned.empty());
    CHECK(syncs() == 1 && g.log.back().releases == 0 && g.releases == kAllocs - 1);

    // queued work, no sync(): exactly one synchronise of the owner's stream, before the first free
    stub::reset();
    {
        mcs::Scratch sc(A, STREAM);
        uint8_t *a = nullptr, *b = nullptr;
        CHECK(sc.dev(&a, 64) == hipSuccess && sc.pinned(&b, 64) == hipSuccess);
        CHECK(A->hipMemsetAsync(a, 0, 64, STREAM) == hipSuccess);
        CHECK(syncs() == 0);
    }
    CHECK(syncs() == 1 && g.log.size() == 2 && g.log[1].kind == 'S');
    CHECK(g.log[1].stream == STREAM && g.log[1].releases == 0 && g.releases == 2);

    // after sync(): none; an allocation after it queues again; synced(e) counts as sync() does,
    // a failed synchronise does not
    stub::reset();
    {
        mcs::Scratch sc(A, STREAM);
        uint8_t *a = nullptr;
        CHECK(sc.dev(&a, 64) == hipSuccess && sc.sync() == hipSuccess && syncs() == 1);
    }
    CHECK(syncs() == 1 && g.live.empty() && g.releases == 1);
    stub::reset();
    {
        mcs::Scratch sc(A, STREAM);
        uint8_t *a = nullptr, *b = nullptr;
        CHECK(sc.dev(&a, 64) == hipSuccess && sc.sync() == hipSuccess);
        CHECK(sc.dev(&b, 64) == hipSuccess);
    }
    CHECK(syncs() == 2 && g.log[1].releases == 0 && g.live.empty());
    stub::reset();
    {
        mcs::Scratch sc(A, STREAM);
        uint8_t *a = nullptr;
        CHECK(sc.dev(&a, 64) == hipSuccess);
        CHECK(sc.synced(hipErrorUnknown) == hipErrorUnknown && sc.synced(hipSuccess) == hipSuccess);
    }
    CHECK(syncs() == 0 && g.live.empty());
    stub::reset();
    {
        mcs::Scratch sc(A, STREAM);
        uint8_t *a = nullptr;
        CHECK(sc.dev(&a, 64) == hipSuccess && sc.synced(hipErrorUnknown) == hipErrorUnknown);
    }
    CHECK(syncs() == 1 && g.live.empty());
    // everything kept: nothing to free, so nothing to wait for
    stub::reset();
    {
        mcs::Scratch sc(A, STREAM);
        uint8_t *a = nullptr;
        CHECK(sc.dev(&a, 64) == hipSuccess && sc.keep(a) == a);
    }
    CHECK(syncs() == 0 && g.live.size() == 1 && g.releases == 0);

    // an owner that never allocated: no runtime call at all
    stub::reset();
    {
        mcs::Scratch sc(A, STREAM);
    }
    CHECK(g.calls == 0 && g.log.empty() && g.releases == 0);

    // more pointers than it holds: refused, nothing leaked
    stub::reset();
    {
        mcs::Scratch sc(A, STREAM);
        uint8_t *q = nullptr;
        for (int i = 0; i < mcs::Scratch::kMax; i++) CHECK(sc.dev(&q, 1) == hipSuccess);
        CHECK(sc.dev(&q, 1) != hipSuccess && g.live.size() == (size_t)mcs::Scratch::kMax);
    }
    CHECK(g.live.empty() && g.bad_free == 0);

    if (g_bad == 0) printf("ok\n");
    return g_bad ? 1 : 0;
}
