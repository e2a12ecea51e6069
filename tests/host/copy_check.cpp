// copy_check.cpp -- a stand-alone check of the host-thread copy helpers (host_copy.hpp): no HIP, no
// library of the project.  Built with the host sanitizers by `make -C dbslmm_amd/csrc sanitize`
// (../bin/copy_asan) and run by tests/test_sanitizers.py; also `g++ -std=c++17 -pthread copy_check.cpp`.
//
// par_memcpy and par_memcpy_list are compared with a serial memcpy of the same ranges.  Every
// destination sits between guard bytes that must come out untouched, and the sizes put the thread
// boundaries inside, at the start of and at the end of a copy (below / at / above the per-thread
// floor, totals that the thread count does not divide).  The first violation prints and exits 1.
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../../dbslmm_amd/csrc/host_copy.hpp"

namespace {

std::string g_case;
#define CHECK(cond, ...)                                                         \
    do {                                                                         \
        if (!(cond)) {                                                           \
            char msg_[512];                                                      \
            snprintf(msg_, sizeof msg_, __VA_ARGS__);                            \
            fprintf(stderr, "copy_check: %s: %s -- %s\n", g_case.c_str(), #cond, msg_); \
            exit(1);                                                             \
        }                                                                        \
    } while (0)

constexpr size_t kGuard = 64;
constexpr unsigned char kGuardByte = 0xA5, kStale = 0x5A;
constexpr size_t KiB = size_t(1) << 10, MiB = size_t(1) << 20;

std::vector<unsigned char> pattern(size_t n, uint64_t seed) {
    std::vector<unsigned char> v(n);
    uint64_t x = seed * 0x9E3779B97F4A7C15ull + 1;
    for (size_t i = 0; i < n; ++i) {
        x = x * 6364136223846793005ull + 1442695040888963407ull;
        v[i] = static_cast<unsigned char>(x >> 56);
    }
    return v;
}

// A destination of n bytes at offset `shift` of its allocation, guard bytes on both sides.
struct Guarded {
    std::vector<unsigned char> mem;
    size_t shift, n;
    Guarded(size_t n_, size_t shift_) : mem(shift_ + kGuard + n_ + kGuard, kGuardByte), shift(shift_), n(n_) {
        std::fill(data(), data() + n, kStale);
    }
    unsigned char* data() { return mem.data() + shift + kGuard; }
    void check(const unsigned char* want) {
        for (size_t i = 0; i < shift + kGuard; ++i) CHECK(mem[i] == kGuardByte, "front guard byte %zu written", i);
        for (size_t i = shift + kGuard + n; i < mem.size(); ++i) CHECK(mem[i] == kGuardByte, "back guard byte %zu written", i);
        CHECK(n == 0 || memcmp(data(), want, n) == 0, "%zu bytes differ from the serial copy", n);
    }
};

void check_par_memcpy(size_t n) {
    g_case = "par_memcpy n = " + std::to_string(n);
    std::vector<unsigned char> src = pattern(n + 1, n);   // (read from offset 1 of its allocation)
    std::vector<unsigned char> want(n);
    if (n) memcpy(want.data(), src.data() + 1, n);
    Guarded dst(n, 1);
    par_memcpy(dst.data(), src.data() + 1, n);
    dst.check(want.data());
}

void check_list(const std::string& name, const std::vector<size_t>& lens) {
    g_case = "par_memcpy_list " + name;
    std::vector<std::vector<unsigned char>> src;
    std::vector<Guarded> dst;
    dst.reserve(lens.size());
    std::vector<CopySeg> segs;
    for (size_t i = 0; i < lens.size(); ++i) {
        src.push_back(pattern(lens[i] + 1, 1000 + i));
        dst.emplace_back(lens[i], 1);
    }
    for (size_t i = 0; i < lens.size(); ++i) segs.push_back({dst[i].data(), src[i].data() + 1, lens[i]});
    par_memcpy_list(segs);
    for (size_t i = 0; i < lens.size(); ++i) {
        std::vector<unsigned char> want(lens[i]);
        if (lens[i]) memcpy(want.data(), src[i].data() + 1, lens[i]);
        dst[i].check(want.data());
    }
}

}  // namespace

int main() {
    int cases = 0;
    for (size_t n : {size_t(0), size_t(1), 2 * MiB - 1, 2 * MiB, 4 * MiB + 1, 16 * MiB + 3}) {
        check_par_memcpy(n);
        ++cases;
    }
    const std::pair<const char*, std::vector<size_t>> lists[] = {
        {"empty", {}},
        {"zero-length segments", {0, 0, 0}},
        {"one byte", {1}},
        {"one 3 MiB segment", {3 * MiB}},
        {"mixed", {1, 512 * KiB - 1, 512 * KiB + 1, 0, 3 * MiB, 7}},
        {"1000 x 4099", std::vector<size_t>(1000, 4099)},
    };
    for (const auto& l : lists) {
        check_list(l.first, l.second);
        ++cases;
    }
    {
        g_case = "backoff_wait, true at once";
        int calls = 0;
        backoff_wait([&] { return ++calls > 0; });
        CHECK(calls == 1, "%d calls of the predicate", calls);
        ++cases;
    }
    {
        g_case = "backoff_wait, flipped by another thread";
        std::atomic<bool> flag{false};
        std::thread t([&] {
            std::this_thread::sleep_for(std::chrono::milliseconds(1));
            flag.store(true, std::memory_order_release);
        });
        backoff_wait([&] { return flag.load(std::memory_order_acquire); });
        CHECK(flag.load(), "returned before the flag was set");
        t.join();
        ++cases;
    }
    printf("ok %d cases\n", cases);
    return 0;
}
