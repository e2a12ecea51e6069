// dev_bufs.hpp -- the one owner of device allocations.  A DevBufs records every pointer it hands
// out and frees what is left when it goes: a plan keeps one for its d_* members, an entry point
// that allocates for one call keeps a local one.  No policy beyond that: every call is one
// hipMalloc / hipFree (nothing pooled or kept between calls).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <vector>

class DevBufs {
public:
    int device = 0;   // the device the pointers belong to (set before the first allocation)

    explicit DevBufs(int dev = 0) : device(dev) {}
    DevBufs(const DevBufs&) = delete;
    DevBufs& operator=(const DevBufs&) = delete;
    ~DevBufs() {
        if (ptrs_.empty()) return;
        (void)hipSetDevice(device);
        for (void* q : ptrs_) (void)free_one(q);
    }

    // max(count, 1) elements.  On failure *out is null and nothing is recorded.
    template <typename T>
    hipError_t alloc(T** out, size_t count) {
        *out = nullptr;
        ptrs_.push_back(nullptr);
        const hipError_t e = hipMalloc(&ptrs_.back(), std::max<size_t>(count, 1) * sizeof(T));
        if (e != hipSuccess) ptrs_.pop_back();
        else *out = static_cast<T*>(ptrs_.back());
        return e;
    }
    // ... zeroed on stream st (asynchronous: ordered before whatever st runs next)
    template <typename T>
    hipError_t zeroed(T** out, size_t count, hipStream_t st) {
        const hipError_t e = alloc(out, count);
        return e != hipSuccess ? e : hipMemsetAsync(*out, 0, std::max<size_t>(count, 1) * sizeof(T), st);
    }
    // Allocate and fill a device array on stream st; complete on return.  Every host -> device copy
    // of the library is ordered on the stream its consumers run on (or one they are forked from):
    // null-stream transfers are not ordered against the contexts' non-blocking streams, and a pageable
    // hipMemcpy may return before its DMA has landed.  (At least one element; an empty vector is
    // not copied.)
    template <typename T>
    hipError_t upload(T** out, const std::vector<T>& src, hipStream_t st) {
        hipError_t e = alloc(out, src.size());
        if (e != hipSuccess || src.empty()) return e;
        e = hipMemcpyAsync(*out, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice, st);
        return e != hipSuccess ? e : hipStreamSynchronize(st);
    }
    // Free p now, forget it and null it (a null p: nothing).  The caller has made sure nothing on the
    // device still uses it, and has the device set.
    template <typename T>
    hipError_t release(T*& p) {
        if (!p) return hipSuccess;
        const auto it = std::find(ptrs_.begin(), ptrs_.end(), static_cast<void*>(p));
        if (it != ptrs_.end()) ptrs_.erase(it);
        const hipError_t e = free_one(p);
        p = nullptr;
        return e;
    }
    // ... several at once (a re-allocation site drops its old buffers before it allocates the new)
    template <typename... T>
    void release_all(T*&... p) {
        ((void)release(p), ...);
    }

private:
    std::vector<void*> ptrs_;
    static hipError_t free_one(void* q) {
        const hipError_t e = hipFree(q);
#ifdef DBSLMM_DIAG
        if (e != hipSuccess) fprintf(stderr, "plan_destroy: hipFree(%p) -> %s\n", q, hipGetErrorString(e));
#endif
        return e;
    }
};

// The two timing events around one call's kernels, destroyed with the scope.
struct EventPair {
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    EventPair() = default;
    EventPair(const EventPair&) = delete;
    EventPair& operator=(const EventPair&) = delete;
    ~EventPair() {
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
    }
    hipError_t create() {
        const hipError_t e = hipEventCreate(&ev0);
        return e != hipSuccess ? e : hipEventCreate(&ev1);
    }
};
