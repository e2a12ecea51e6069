// dev_bufs.hpp -- the owners of HIP resources: DevBufs for device allocations, and below it the
// host-side ones (PinnedBuf, EventList, GraphExecs).  A DevBufs records every pointer it hands
// out and frees what is left when it goes: a plan keeps one for its d_* members, an entry point
// that allocates for one call keeps a local one.  No policy beyond that: every call is one
// hipMalloc / hipFree (nothing pooled or kept between calls).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <utility>
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

// A pinned host buffer that only grows: reserve(bytes) frees and allocates again only for a larger
// size (contents are not kept), with the flags given once.  Freed with its owner.
class PinnedBuf {
public:
    explicit PinnedBuf(unsigned flags = hipHostMallocDefault) : flags_(flags) {}
    PinnedBuf(const PinnedBuf&) = delete;
    PinnedBuf& operator=(const PinnedBuf&) = delete;
    ~PinnedBuf() { (void)drop(); }
    hipError_t reserve(size_t bytes) {
        if (bytes <= bytes_) return hipSuccess;
        hipError_t e = drop();
        if (e == hipSuccess && (e = hipHostMalloc(&p_, bytes, flags_)) == hipSuccess) bytes_ = bytes;
        return e;
    }
    template <typename T = void>
    T* get() const { return static_cast<T*>(p_); }

private:
    void* p_ = nullptr;
    size_t bytes_ = 0;
    unsigned flags_;
    hipError_t drop() {
        void* old = std::exchange(p_, nullptr);
        bytes_ = 0;
        return old ? hipHostFree(old) : hipSuccess;
    }
};

// A list of events that grows on demand (each created with the list's flags), and a list of
// instantiated graphs (null = not captured yet); reset() destroys what they hold.
struct EventList {
    std::vector<hipEvent_t> ev;
    unsigned flags;
    explicit EventList(unsigned fl = hipEventDisableTiming) : flags(fl) {}
    EventList(const EventList&) = delete;
    EventList& operator=(const EventList&) = delete;
    ~EventList() { reset(); }
    hipError_t grow(size_t n) {   // at least n events
        hipError_t rc = hipSuccess;
        for (hipEvent_t e; ev.size() < n && (rc = hipEventCreateWithFlags(&e, flags)) == hipSuccess;) ev.push_back(e);
        return rc;
    }
    hipEvent_t operator[](size_t i) const { return ev[i]; }
    void reset() {
        for (hipEvent_t e : ev) (void)hipEventDestroy(e);
        ev.clear();
    }
};
struct GraphExecs {
    std::vector<hipGraphExec_t> gx;
    GraphExecs() = default;
    GraphExecs(const GraphExecs&) = delete;
    GraphExecs& operator=(const GraphExecs&) = delete;
    ~GraphExecs() { reset(); }
    hipGraphExec_t& at(size_t i) {   // slot i (null until a graph is instantiated into it)
        if (gx.size() <= i) gx.resize(i + 1, nullptr);
        return gx[i];
    }
    void reset() {
        for (hipGraphExec_t g : gx)
            if (g) (void)hipGraphExecDestroy(g);
        gx.clear();
    }
};
