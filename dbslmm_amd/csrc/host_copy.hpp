// host_copy.hpp -- host-thread helpers of the uploads and downloads: a backing-off wait and memcpy
// spread over a few threads.  No HIP here: the stand-alone check (tests/host/copy_check.cpp) compiles
// this header alone, under the host sanitizers.
#pragma once
#include <algorithm>
#include <chrono>
#include <cstddef>
#include <cstring>
#include <thread>
#include <vector>

// wait until pred(): a short spin (a chunk is ~0.35 ms of work), then 20 us sleeps, so waiting
// threads do not take the cores of the host threads the caller runs meanwhile (the CLI parses
// its text files during the upload) on a machine with fewer cores than the pool
template <class P>
inline void backoff_wait(P pred) {
    for (int i = 0; !pred(); ++i) {
        if (i < 256) std::this_thread::yield();
        else std::this_thread::sleep_for(std::chrono::microseconds(20));
    }
}

// memcpy on up to 8 host threads (a result download lands in pinned memory; the caller's arrays
// are often fresh pages, so the page faults of the copy are spread over the threads too): a list of
// copies (a streamed run's remainder: scattered block ranges), the bytes of the concatenation split
// evenly over the threads, at least min_part each.
struct CopySeg {
    void* dst;
    const void* src;
    size_t n;
};
inline void par_memcpy_list(const std::vector<CopySeg>& segs, size_t min_part = size_t(512) << 10) {
    size_t total = 0;
    for (const CopySeg& s : segs) total += s.n;
    const unsigned hw = std::max(1u, std::min(8u, std::thread::hardware_concurrency()));
    const unsigned nt = static_cast<unsigned>(std::min<size_t>(hw, std::max<size_t>(1, total / min_part)));
    const size_t part = (total + nt - 1) / nt;
    auto work = [&segs, part](unsigned t) {   // bytes [t part, (t + 1) part) of the concatenation
        const size_t lo = t * part, hi = lo + part;
        size_t off = 0;
        for (const CopySeg& s : segs) {
            const size_t a = std::max(lo, off), z = std::min(hi, off + s.n);
            if (a < z) memcpy(static_cast<char*>(s.dst) + (a - off), static_cast<const char*>(s.src) + (a - off), z - a);
            off += s.n;
            if (off >= hi) break;
        }
    };
    std::vector<std::thread> th;
    for (unsigned t = 1; t < nt; ++t) th.emplace_back(work, t);
    work(0);
    for (auto& t : th) t.join();
}
// ... and one copy
inline void par_memcpy(void* dst, const void* src, size_t n) { par_memcpy_list({{dst, src, n}}, size_t(2) << 20); }
