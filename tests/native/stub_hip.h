// stub_hip.h -- the fake HIP runtime of the native checks in this folder: libmcs's host sources,
// compiled with g++, run on it without a GPU.  Header only; include it in the one source file of
// a program.  It provides
//   - device memory as fake pointers (never dereferenced) kept in a live set, with double and
//     unknown frees counted; pinned memory as real zeroed host memory (host code reads it);
//   - streams, events, graphs and executable graphs as fake handles, counted;
//   - a log, in order, of every launch (kernel name, grid, block, LDS bytes, stream, argument
//     block),
//     synchronise, memset and copy, under a mutex (the rig job runs a worker thread);
//   - a hook that fills a device-to-host copy;
//   - failure injection: the k-th runtime call fails (or the k-th hipMalloc alone).  Every call
//     that returns hipError_t counts, except the releases (hipFree, hipHostFree, hip*Destroy,
//     hipModuleUnload) and hipSetDevice of the device that is current (a guard's restore), which
//     always succeed: libmcs discards their status;
//   - what the host sources need of hip_rt.cpp and mcs_runtime.cpp: mcs::rt::api, runtime_name,
//     mcs::module_function and, with STUB_HIP_DEFINE_FAIL (programs that do not link
//     mcs_runtime.cpp), mcs::fail and mcs::clear_error.
#pragma once

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <set>
#include <string>
#include <vector>

#include "mcs_common.h"

namespace stub {

struct Event {
    char kind = 0;                 // 'L'aunch, 'S'ynchronise, 'M'emset, 'C'opy
    std::string name;              // launches: the kernel
    unsigned gx = 0, gy = 0, gz = 0, bx = 0, by = 0, bz = 0;
    unsigned lds = 0;              // launches: dynamic LDS bytes
    hipStream_t stream = nullptr;
    size_t bytes = 0;              // memsets and copies: their size; launches: the argument block's
    void *dst = nullptr;
    int call = 0;                  // which runtime call it was (the injection's count)
    int releases = 0;              // hipFree / hipHostFree calls before it
    std::vector<uint8_t> args;     // launches: the argument block
    // The argument block as a T: false unless it has T's size.
    template <class T>
    bool args_as(T *out) const
    {
        if (args.size() != sizeof(T)) return false;
        memcpy(out, args.data(), sizeof(T));
        return true;
    }
};

struct State {
    std::mutex mu;
    std::map<void *, size_t> live;     // device allocations and their sizes
    std::map<void *, size_t> pinned;   // pinned host allocations
    std::vector<void *> freed;         // what hipFree was given, in order
    std::set<uintptr_t> streams, events, graphs, execs;
    int mallocs = 0;                   // hipMalloc calls
    int bad_free = 0;                  // frees / destroys of something unknown or already freed
    int releases = 0;                  // hipFree / hipHostFree calls
    int calls = 0;                     // runtime calls that count for the injection
    int fail_at = 0;                   // fail the fail_at-th call (0: none) ...
    bool fail_mallocs_only = false;    // ... counting hipMalloc calls only
    std::vector<Event> log;
    // Called for every device-to-host copy after it is logged (may fill dst).
    void (*copy_hook)(void *dst, size_t bytes, hipStream_t s) = nullptr;
    std::map<std::string, uintptr_t> handles;   // module_function's registry
    std::map<uintptr_t, std::string> names;
    uintptr_t next = 0;
};
inline State g;

constexpr hipError_t kInjected = hipErrorOutOfMemory;

// Fails the k-th call from here (0: none), counting hipMalloc calls only if asked to.
inline void fail_at(int k, bool mallocs_only = false)
{
    std::lock_guard<std::mutex> lk(g.mu);
    g.calls = g.mallocs = 0;
    g.fail_at = k;
    g.fail_mallocs_only = mallocs_only;
}
// The same after clearing the device state, the counters and the log.
inline void reset(int k = 0, bool mallocs_only = false)
{
    fail_at(k, mallocs_only);
    std::lock_guard<std::mutex> lk(g.mu);
    for (auto &p : g.pinned) free(p.first);
    g.live.clear(), g.pinned.clear(), g.freed.clear(), g.streams.clear(), g.events.clear();
    g.graphs.clear(), g.execs.clear();
    g.log.clear();
    g.bad_free = g.releases = 0;
}
// The live device allocations.
inline std::set<void *> live_set()
{
    std::lock_guard<std::mutex> lk(g.mu);
    std::set<void *> out;
    for (auto &p : g.live) out.insert(p.first);
    return out;
}
// The first live device / pinned allocation of `bytes` bytes (nullptr: none).
inline void *alloc_of(const std::map<void *, size_t> &m, size_t bytes)
{
    std::lock_guard<std::mutex> lk(g.mu);
    for (auto &p : m)
        if (p.second == bytes) return p.first;
    return nullptr;
}
inline void *device_alloc_of(size_t bytes) { return alloc_of(g.live, bytes); }
inline void *pinned_alloc_of(size_t bytes) { return alloc_of(g.pinned, bytes); }

// (g.mu held) Whether this call is the one to fail.
inline bool hit(bool is_malloc = false)
{
    g.calls++;
    if (is_malloc) g.mallocs++;
    if (g.fail_mallocs_only) return is_malloc && g.mallocs == g.fail_at;
    return g.calls == g.fail_at;
}
#define STUB_CALL()                                                                            \
    std::lock_guard<std::mutex> lk(g.mu);                                                      \
    if (hit()) return kInjected
// A call that counts and does nothing else.
#define STUB_OK(name, args)                                                                    \
    inline hipError_t name args                                                                \
    {                                                                                          \
        STUB_CALL();                                                                           \
        return hipSuccess;                                                                     \
    }
inline uintptr_t fresh() { return 0x10000000ull * (uintptr_t)++g.next; }
inline void put(Event &e)
{
    e.call = g.calls;
    e.releases = g.releases;
    g.log.push_back(e);
}

inline hipError_t hipGetDeviceCount(int *n)
{
    STUB_CALL();
    *n = 1;
    return hipSuccess;
}
inline hipError_t hipGetDevice(int *d)
{
    STUB_CALL();
    *d = 0;
    return hipSuccess;
}
inline hipError_t hipSetDevice(int d)
{
    if (d == 0) return hipSuccess;   // (the one device, current already: DeviceGuard's restore)
    STUB_CALL();
    return hipErrorInvalidDevice;
}
inline const char *hipGetErrorString(hipError_t) { return "stub error"; }
inline hipError_t hipMalloc(void **p, size_t n)
{
    std::lock_guard<std::mutex> lk(g.mu);
    if (hit(true)) return kInjected;
    *p = (void *)fresh();
    g.live[*p] = n;
    return hipSuccess;
}
inline hipError_t hipFree(void *p)
{
    std::lock_guard<std::mutex> lk(g.mu);
    g.freed.push_back(p);
    g.releases++;
    if (!g.live.erase(p)) g.bad_free++;   // never allocated, or freed twice
    return hipSuccess;
}
inline hipError_t hipHostMalloc(void **p, size_t n, unsigned)
{
    STUB_CALL();
    *p = calloc(1, n ? n : 1);
    if (!*p) return hipErrorOutOfMemory;
    g.pinned[*p] = n;
    return hipSuccess;
}
inline hipError_t hipHostFree(void *p)
{
    std::lock_guard<std::mutex> lk(g.mu);
    g.releases++;
    if (g.pinned.erase(p)) free(p);
    else g.bad_free++;
    return hipSuccess;
}
inline hipError_t hipMemcpyAsync(void *dst, const void *, size_t n, hipMemcpyKind kind,
                                 hipStream_t s)
{
    {
        STUB_CALL();
        Event e;
        e.kind = 'C', e.stream = s, e.bytes = n, e.dst = dst;
        put(e);
    }
    // (other read-backs keep the zeros their host buffers start with)
    if (kind == hipMemcpyDeviceToHost && g.copy_hook) g.copy_hook(dst, n, s);
    return hipSuccess;
}
inline hipError_t hipMemcpy2DAsync(void *dst, size_t, const void *, size_t, size_t w, size_t h,
                                   hipMemcpyKind, hipStream_t s)
{
    STUB_CALL();
    Event e;
    e.kind = 'C', e.stream = s, e.bytes = w * h, e.dst = dst;
    put(e);
    return hipSuccess;
}
inline hipError_t hipMemsetAsync(void *dst, int, size_t n, hipStream_t s)
{
    STUB_CALL();
    Event e;
    e.kind = 'M', e.stream = s, e.bytes = n, e.dst = dst;
    put(e);
    return hipSuccess;
}
inline hipError_t stream_create(hipStream_t *s)
{
    STUB_CALL();
    const uintptr_t h = fresh() + 0x77000;
    g.streams.insert(h);
    *s = (hipStream_t)h;
    return hipSuccess;
}
inline hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned) { return stream_create(s); }
inline hipError_t hipStreamCreateWithPriority(hipStream_t *s, unsigned, int)
{
    return stream_create(s);
}
inline hipError_t hipDeviceGetStreamPriorityRange(int *least, int *greatest)
{
    STUB_CALL();
    *least = 0;
    *greatest = -1;
    return hipSuccess;
}
inline hipError_t hipStreamDestroy(hipStream_t s)
{
    std::lock_guard<std::mutex> lk(g.mu);
    if (!g.streams.erase((uintptr_t)s)) g.bad_free++;
    return hipSuccess;
}
inline hipError_t hipStreamSynchronize(hipStream_t s)
{
    STUB_CALL();
    Event e;
    e.kind = 'S', e.stream = s;
    put(e);
    return hipSuccess;
}
inline hipError_t event_create(hipEvent_t *ev)
{
    STUB_CALL();
    const uintptr_t h = fresh() + 0x55000;
    g.events.insert(h);
    *ev = (hipEvent_t)h;
    return hipSuccess;
}
inline hipError_t hipEventCreate(hipEvent_t *ev) { return event_create(ev); }
inline hipError_t hipEventCreateWithFlags(hipEvent_t *ev, unsigned) { return event_create(ev); }
STUB_OK(hipStreamWaitEvent, (hipStream_t, hipEvent_t, unsigned))
inline hipError_t hipEventDestroy(hipEvent_t ev)
{
    std::lock_guard<std::mutex> lk(g.mu);
    if (!g.events.erase((uintptr_t)ev)) g.bad_free++;
    return hipSuccess;
}
STUB_OK(hipEventRecord, (hipEvent_t, hipStream_t))
STUB_OK(hipEventSynchronize, (hipEvent_t))
inline hipError_t hipEventElapsedTime(float *ms, hipEvent_t, hipEvent_t)
{
    STUB_CALL();
    *ms = 0.f;
    return hipSuccess;
}
inline hipError_t hipModuleLoadData(hipModule_t *m, const void *)
{
    STUB_CALL();
    *m = (hipModule_t)fresh();
    return hipSuccess;
}
inline hipError_t hipModuleUnload(hipModule_t) { return hipSuccess; }
STUB_OK(hipStreamBeginCapture, (hipStream_t, hipStreamCaptureMode))
inline hipError_t hipStreamEndCapture(hipStream_t, hipGraph_t *gr)
{
    STUB_CALL();
    *gr = (hipGraph_t)fresh();
    g.graphs.insert((uintptr_t)*gr);
    return hipSuccess;
}
inline hipError_t hipGraphInstantiate(hipGraphExec_t *x, hipGraph_t, hipGraphNode_t *, char *,
                                      size_t)
{
    STUB_CALL();
    *x = (hipGraphExec_t)fresh();
    g.execs.insert((uintptr_t)*x);
    return hipSuccess;
}
STUB_OK(hipGraphLaunch, (hipGraphExec_t, hipStream_t))
inline hipError_t hipGraphExecDestroy(hipGraphExec_t x)
{
    std::lock_guard<std::mutex> lk(g.mu);
    if (!g.execs.erase((uintptr_t)x)) g.bad_free++;
    return hipSuccess;
}
inline hipError_t hipGraphDestroy(hipGraph_t gr)
{
    std::lock_guard<std::mutex> lk(g.mu);
    if (!g.graphs.erase((uintptr_t)gr)) g.bad_free++;
    return hipSuccess;
}
inline hipError_t hipModuleGetFunction(hipFunction_t *f, hipModule_t, const char *)
{
    STUB_CALL();
    *f = nullptr;
    return hipSuccess;
}
inline hipError_t hipModuleLaunchKernel(hipFunction_t f, unsigned gx, unsigned gy, unsigned gz,
                                        unsigned bx, unsigned by, unsigned bz, unsigned lds,
                                        hipStream_t s, void **, void **cfg)
{
    STUB_CALL();
    Event e;
    e.kind = 'L';
    const auto it = g.names.find((uintptr_t)f);
    if (it != g.names.end()) e.name = it->second;
    e.gx = gx, e.gy = gy, e.gz = gz, e.bx = bx, e.by = by, e.bz = bz, e.lds = lds;
    e.stream = s;
    if (cfg) {   // {BUFFER_POINTER, args, BUFFER_SIZE, &size, END}
        e.bytes = *(const size_t *)cfg[3];
        e.args.assign((const uint8_t *)cfg[1], (const uint8_t *)cfg[1] + e.bytes);
    }
    put(e);
    return hipSuccess;
}
#undef STUB_OK
#undef STUB_CALL

inline const mcs::rt::Api *api()
{
    static const mcs::rt::Api a = [] {
        mcs::rt::Api t = {};
#define STUB_SET(name, ret, args) t.name = stub::name;
        MCS_HIP_API(STUB_SET)
#undef STUB_SET
        return t;
    }();
    return &a;
}

// The log as text, one event a line (streams and pointers by their order of first appearance, so
// that two runs compare equal whatever their handles are).
inline std::vector<std::string> log_lines()
{
    std::lock_guard<std::mutex> lk(g.mu);
    std::map<uintptr_t, int> ids;
    const auto id = [&](const void *p) {
        if (!p) return 0;
        const auto r = ids.emplace((uintptr_t)p, (int)ids.size() + 1);
        return r.first->second;
    };
    std::vector<std::string> out;
    for (const Event &e : g.log) {
        char b[256];
        if (e.kind == 'L')
            snprintf(b, sizeof(b), "L %s grid %ux%ux%u block %ux%ux%u lds %u args %zu stream s%d",
                     e.name.c_str(), e.gx, e.gy, e.gz, e.bx, e.by, e.bz, e.lds, e.bytes,
                     id(e.stream));
        else if (e.kind == 'S')
            snprintf(b, sizeof(b), "S stream s%d", id(e.stream));
        else
            snprintf(b, sizeof(b), "%c %zu bytes stream s%d", e.kind, e.bytes, id(e.stream));
        out.push_back(b);
    }
    return out;
}

}  // namespace stub

// ---- what the linked host sources need of hip_rt.cpp and mcs_runtime.cpp
const mcs::rt::Api *mcs::rt::api() { return stub::api(); }
const char *mcs::rt::runtime_name() { return "stub"; }
int mcs::module_function(const rt::Api *, int, Module, const char *name, hipFunction_t *out)
{
    std::lock_guard<std::mutex> lk(stub::g.mu);
    uintptr_t &h = stub::g.handles[name];
    if (!h) {
        h = 0x700000 + 16 * stub::g.handles.size();
        stub::g.names[h] = name;
    }
    *out = (hipFunction_t)h;
    return MCS_OK;
}
#ifdef STUB_HIP_DEFINE_FAIL
int mcs::fail(int code, const char *, ...) { return code; }
void mcs::clear_error() {}
#endif
