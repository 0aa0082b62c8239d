// mcs_scratch.h -- the device and pinned-host memory one call allocates for its own duration
// (DESIGN.md section 4 "Host layout").  Host only.
#pragma once

#include <stddef.h>

#include "hip_rt.h"
#include "mcs.h"

namespace mcs {

// Owns what a call allocates for work on one stream and frees it when the call returns, by
// whichever path: each pointer still owned exactly once, after a synchronise of the stream if work
// may still be queued on it -- that is, unless a synchronise made through sync() / synced() has
// succeeded since the last allocation.  A call that ends in such a synchronise pays nothing more
// on its way out; one that leaves early is drained first.  keep() takes out what outlives the call.
struct Scratch {
    static constexpr int kMax = MCS_MAX_CAMS + 4;   // (mcs_plan_footprint: a mask per camera + 2)
    const rt::Api *const A;
    const hipStream_t s;
    void *own[kMax];
    bool host[kMax];
    int n = 0;
    bool queued = false;

    Scratch(const rt::Api *a, hipStream_t stream) : A(a), s(stream) {}
    Scratch(const Scratch &) = delete;   // (const members: no assignment either)
    ~Scratch()
    {
        if (n > 0 && queued) (void)A->hipStreamSynchronize(s);
        for (int i = 0; i < n; i++) (void)(host[i] ? A->hipHostFree(own[i]) : A->hipFree(own[i]));
    }

    // Device / pinned host memory for `count` elements at *ptr, owned by this call.
    template <class T>
    hipError_t dev(T **ptr, size_t count) { return take(ptr, count, false); }
    template <class T>
    hipError_t pinned(T **ptr, size_t count) { return take(ptr, count, true); }
    // Ends the ownership of `ptr` (it outlives the call) and returns it.
    template <class T>
    T *keep(T *ptr)
    {
        for (int i = 0; i < n; i++)
            if (own[i] == static_cast<void *>(ptr)) {
                n--;
                own[i] = own[n];
                host[i] = host[n];
                break;
            }
        return ptr;
    }
    // hipStreamSynchronize of the stream; synced(e): the result e of a synchronise made elsewhere.
    hipError_t sync() { return synced(A->hipStreamSynchronize(s)); }
    hipError_t synced(hipError_t e)
    {
        if (e == hipSuccess) queued = false;
        return e;
    }

private:
    template <class T>
    hipError_t take(T **ptr, size_t count, bool pin)
    {
        if (n == kMax) return hipErrorOutOfMemory;
        void *q = nullptr;
        const hipError_t e = pin ? A->hipHostMalloc(&q, count * sizeof(T), 0)
                                 : A->hipMalloc(&q, count * sizeof(T));
        if (e != hipSuccess) return e;
        own[n] = q;
        host[n] = pin;
        n++;
        queued = true;
        *ptr = static_cast<T *>(q);
        return hipSuccess;
    }
};

}  // namespace mcs
