// ldsc_check.cpp -- a stand-alone check of the LD score host code (ldsc_layout.hpp, ldsc_fit.hpp): no
// HIP, no library of the project.  Built with the host sanitizers by `make -C dbslmm_amd/csrc
// sanitize` (../bin/ldsc_asan) and run by tests/test_ldsc_host.py; also `g++ -std=c++17 ldsc_check.cpp`.
//
// Layout: for every row list below the 128-band is built and checked against what the kernels need
// of it, worked out here independently in O(n^2): the position order, the window [lo, hi] and
// n_window of every row, that every in-window pair lies in exactly one listed tile, that the diagonal
// is always listed, that every off-diagonal tile holds an in-window pair (so none crosses a
// chromosome change or a gap wider than the window), the row / column indices dbslmm_l2_reduce walks,
// and the missing-call flag of every tile.
// Regression: ldsc::fit on a fixed data set against the values of the NumPy restatement
// (tests/_ldsc_ref.py: ldsc_fit_ref), and its statuses.  The first violation prints and exits 1.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../dbslmm_amd/csrc/ldsc_fit.hpp"
#include "../../dbslmm_amd/csrc/ldsc_layout.hpp"

namespace {

std::string g_case;
#define CHECK(cond, ...)                                                          \
    do {                                                                          \
        if (!(cond)) {                                                            \
            char msg_[512];                                                       \
            snprintf(msg_, sizeof msg_, __VA_ARGS__);                             \
            fprintf(stderr, "ldsc_check: %s: %s -- %s\n", g_case.c_str(), #cond, msg_); \
            exit(1);                                                              \
        }                                                                         \
    } while (0)

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {   // xorshift64*
    g_rng ^= g_rng >> 12;
    g_rng ^= g_rng << 25;
    g_rng ^= g_rng >> 27;
    return static_cast<uint32_t>((g_rng * 0x2545F4914F6CDD1Dull) >> 32);
}

struct Rows {
    std::vector<int32_t> chr;
    std::vector<int64_t> bp;
    std::vector<uint8_t> miss;
};

bool in_window(const Rows& c, int32_t a, int32_t b, int64_t w) {
    const int64_t d = c.bp[a] - c.bp[b];
    return c.chr[a] == c.chr[b] && (d < 0 ? -d : d) <= w;
}

void check_case(const std::string& name, const Rows& c, int64_t window) {
    g_case = name;
    const int32_t n = static_cast<int32_t>(c.chr.size());
    const LdscLayout L = build_ldsc_layout(n, c.chr.data(), c.bp.data(), window, c.miss.empty() ? nullptr : c.miss.data());
    const int32_t TR = (n + 127) / 128;
    CHECK(L.n == n && L.n_trows == TR, "n %d trows %d", L.n, L.n_trows);
    CHECK(static_cast<int32_t>(L.order.size()) == n && static_cast<int32_t>(L.lo.size()) == n &&
          static_cast<int32_t>(L.hi.size()) == n, "sizes");
    std::vector<char> seen(static_cast<size_t>(n), 0);
    for (int32_t p = 0; p < n; ++p) {
        const int32_t k = L.order[p];
        CHECK(k >= 0 && k < n && !seen[k], "order[%d] = %d", p, k);
        seen[k] = 1;
        if (p > 0) {
            const int32_t a = L.order[p - 1];
            const bool le = c.chr[a] != c.chr[k] ? c.chr[a] < c.chr[k] : c.bp[a] != c.bp[k] ? c.bp[a] < c.bp[k] : a < k;
            CHECK(le, "positions %d, %d out of order", p - 1, p);
        }
    }
    // the window of every position and n_window, by counting
    std::vector<int32_t> nw(static_cast<size_t>(n) + 1, -7);
    ldsc_window_counts(L, nw.data());
    CHECK(nw[n] == -7, "ldsc_window_counts wrote past n_window");
    for (int32_t p = 0; p < n; ++p) {
        int32_t cnt = 0, first = -1, last = -1;
        for (int32_t q = 0; q < n; ++q)
            if (in_window(c, L.order[p], L.order[q], window)) {
                ++cnt;
                if (first < 0) first = q;
                last = q;
            }
        CHECK(L.lo[p] == first && L.hi[p] == last && last - first + 1 == cnt, "position %d: [%d, %d], counted [%d, %d] %d",
              p, L.lo[p], L.hi[p], first, last, cnt);
        CHECK(nw[L.order[p]] == cnt, "n_window[%d] = %d, counted %d", L.order[p], nw[L.order[p]], cnt);
    }
    // the band
    std::map<std::pair<int32_t, int32_t>, int> listed;
    for (size_t t = 0; t < L.tiles.size(); ++t) {
        const L2Tile& tl = L.tiles[t];
        CHECK(tl.ti >= 0 && tl.ti <= tl.tj && tl.tj < TR, "tile %zu = (%d, %d)", t, tl.ti, tl.tj);
        CHECK(listed.emplace(std::make_pair(tl.ti, tl.tj), static_cast<int>(t)).second, "tile (%d, %d) twice", tl.ti, tl.tj);
        if (t > 0)
            CHECK(L.tiles[t - 1].ti < tl.ti || (L.tiles[t - 1].ti == tl.ti && L.tiles[t - 1].tj < tl.tj),
                  "tile %zu not after its predecessor", t);
    }
    for (int32_t I = 0; I < TR; ++I) CHECK(listed.count({I, I}) == 1, "diagonal tile %d not listed", I);
    std::map<std::pair<int32_t, int32_t>, int> holds;
    for (int32_t p = 0; p < n; ++p)
        for (int32_t q = p; q < n; ++q)
            if (in_window(c, L.order[p], L.order[q], window)) {
                CHECK(listed.count({p / 128, q / 128}) == 1, "pair (%d, %d) in no listed tile", p, q);
                holds[{p / 128, q / 128}]++;
            }
    for (const auto& kv : listed)
        CHECK(holds.count(kv.first) == 1, "tile (%d, %d) holds no in-window pair", kv.first.first, kv.first.second);
    // the indices of the reduce kernel
    CHECK(static_cast<int32_t>(L.row_ptr.size()) == TR + 1 && static_cast<int32_t>(L.col_lo.size()) == TR, "index sizes");
    CHECK(L.row_ptr[0] == 0 && L.row_ptr[TR] == static_cast<int32_t>(L.tiles.size()), "row_ptr ends");
    for (int32_t I = 0; I < TR; ++I) {
        CHECK(L.row_ptr[I] < L.row_ptr[I + 1], "row %d empty", I);
        for (int32_t t = L.row_ptr[I]; t < L.row_ptr[I + 1]; ++t)
            CHECK(L.tiles[t].ti == I && L.tiles[t].tj == I + (t - L.row_ptr[I]), "row %d lists tile %d = (%d, %d)", I, t,
                  L.tiles[t].ti, L.tiles[t].tj);
    }
    for (int32_t J = 0; J < TR; ++J) {
        CHECK(L.col_lo[J] >= 0 && L.col_lo[J] <= J, "col_lo[%d] = %d", J, L.col_lo[J]);
        for (int32_t I = 0; I <= J; ++I) {
            const bool want = listed.count({I, J}) == 1;
            CHECK(want == (I >= L.col_lo[J]), "tile (%d, %d) listed %d, col_lo %d", I, J, want, L.col_lo[J]);
            if (want) {
                const int32_t t = L.row_ptr[I] + (J - I);
                CHECK(t < L.row_ptr[I + 1] && L.tiles[t].ti == I && L.tiles[t].tj == J, "tile (%d, %d) not at %d", I, J, t);
            }
        }
    }
    // the missing-call flags
    for (const L2Tile& tl : L.tiles) {
        bool any = false;
        for (int32_t T : {tl.ti, tl.tj})
            for (int32_t p = 128 * T; p < n && p < 128 * (T + 1); ++p)
                any = any || (!c.miss.empty() && c.miss[L.order[p]]);
        CHECK((tl.missing != 0) == any, "tile (%d, %d) missing %d, rows say %d", tl.ti, tl.tj, tl.missing, any);
    }
}

// n rows on n_chr chromosomes at random base pairs below span, in random (unsorted) order; one row
// in miss_every with a missing call (0: none)
Rows random_rows(int32_t n, int32_t n_chr, int64_t span, uint32_t miss_every) {
    Rows c;
    for (int32_t k = 0; k < n; ++k) {
        c.chr.push_back(1 + static_cast<int32_t>(rnd() % static_cast<uint32_t>(n_chr)));
        c.bp.push_back(static_cast<int64_t>(rnd() % static_cast<uint64_t>(span)));
        if (miss_every) c.miss.push_back(rnd() % miss_every == 0);
    }
    return c;
}

bool close(double got, double want) { return std::fabs(got - want) <= 1e-9 * std::fabs(want); }

void check_fit() {
    g_case = "fit";
    // the fixed data set of tests/test_ldsc_host.py::test_fixed_data_set_values_of_the_host_check
    const int n = 61;
    std::vector<double> l(n), N(n), chi2(n);
    for (int j = 0; j < n; ++j) {
        l[j] = 1 + ((j * 37) % 101) / 4.0;
        N[j] = 40000.0 + ((j * 7919) % 10000);
        chi2[j] = (1 + N[j] * 0.4 * l[j] / 1e5) * (0.2 + ((j * 53) % 17) / 4.0);
    }
    ldsc::Result r = ldsc::fit(n, chi2.data(), N.data(), l.data(), 1e5, false, 0.0, 7, 0.0);
    CHECK(r.status == ldsc::kOk && r.n_used == 61, "free: status %d n %lld", r.status, static_cast<long long>(r.n_used));
    CHECK(close(r.h2, 1.1868932222403816) && close(r.h2_se, 0.42493426955392644), "free: h2 %.17g se %.17g", r.h2, r.h2_se);
    CHECK(close(r.intercept, 1.2359638193077034) && close(r.intercept_se, 1.4667763580301476), "free: a %.17g se %.17g",
          r.intercept, r.intercept_se);
    CHECK(close(r.mean_chi2, 7.507473225409836), "mean chi2 %.17g", r.mean_chi2);
    r = ldsc::fit(n, chi2.data(), N.data(), l.data(), 1e5, true, 1.0, 7, 0.0);
    CHECK(r.status == ldsc::kOk, "fixed: status %d", r.status);
    CHECK(close(r.h2, 1.294347355001953) && close(r.h2_se, 0.14570548674778613), "fixed: h2 %.17g se %.17g", r.h2, r.h2_se);
    CHECK(r.intercept == 1.0 && r.intercept_se == 0.0, "fixed: a %.17g", r.intercept);
    r = ldsc::fit(n, chi2.data(), N.data(), l.data(), 1e5, false, 0.0, 7, 5.0);
    CHECK(r.status == ldsc::kOk && r.n_used == 25, "chisq_max: status %d n %lld", r.status, static_cast<long long>(r.n_used));
    CHECK(close(r.h2, 0.1704796896413038) && close(r.intercept, 2.0528521285892105), "chisq_max: h2 %.17g a %.17g", r.h2,
          r.intercept);
    // more blocks than SNPs: one SNP per block
    r = ldsc::fit(5, chi2.data(), N.data(), l.data(), 1e5, false, 0.0, 200, 0.0);
    CHECK(r.status == ldsc::kOk && std::isfinite(r.h2_se), "n = 5: status %d", r.status);
    // too few SNPs: n < 2 parameters each way; n = 0
    r = ldsc::fit(3, chi2.data(), N.data(), l.data(), 1e5, false, 0.0, 200, 0.0);
    CHECK(r.status == ldsc::kTooFew && std::isnan(r.h2), "n = 3 free: status %d", r.status);
    r = ldsc::fit(1, chi2.data(), N.data(), l.data(), 1e5, true, 1.0, 200, 0.0);
    CHECK(r.status == ldsc::kTooFew, "n = 1 fixed: status %d", r.status);
    r = ldsc::fit(0, nullptr, nullptr, nullptr, 1e5, false, 0.0, 200, 0.0);
    CHECK(r.status == ldsc::kTooFew && r.n_used == 0, "n = 0: status %d", r.status);
    r = ldsc::fit(3, chi2.data(), N.data(), l.data(), 1e5, true, 1.0, 200, 0.0);
    CHECK(r.status == ldsc::kOk, "n = 3 fixed: status %d", r.status);
    // singular: every x equal with a free intercept
    std::vector<double> l1(n, 12.5), N1(n, 45000.0);
    r = ldsc::fit(n, chi2.data(), N1.data(), l1.data(), 1e5, false, 0.0, 7, 0.0);
    CHECK(r.status == ldsc::kSingular && std::isnan(r.h2), "equal x: status %d", r.status);
    r = ldsc::fit(n, chi2.data(), N1.data(), l1.data(), 1e5, true, 1.0, 7, 0.0);
    CHECK(r.status == ldsc::kOk, "equal x, fixed intercept: status %d", r.status);
}

}  // namespace

int main() {
    int cases = 0;
    // row counts at the tile edges; one chromosome, everything inside the window
    for (int32_t n : {0, 1, 127, 128, 129, 257}) {
        check_case("dense n=" + std::to_string(n), random_rows(n, 1, 1000, 0), 1000);
        check_case("dense, missing calls n=" + std::to_string(n), random_rows(n, 1, 1000, 40), 1000);
        check_case("window 0 n=" + std::to_string(n), random_rows(n, 2, 30, 7), 0);
        cases += 3;
    }
    // several chromosomes that share bp values: no tile pair across
    for (int32_t n : {129, 300, 700}) {
        check_case("shared bp n=" + std::to_string(n), random_rows(n, 4, 50, 100), 10);
        check_case("shared bp, equal positions n=" + std::to_string(n), random_rows(n, 3, 4, 0), 0);
        cases += 2;
    }
    // a real band: a window far narrower than the span, unsorted input, several tile columns wide
    for (int32_t n : {300, 700, 1500}) {
        check_case("band n=" + std::to_string(n), random_rows(n, 2, 100000, 200), 20000);
        check_case("narrow band n=" + std::to_string(n), random_rows(n, 1, 100000, 0), 500);
        cases += 2;
    }
    // a gap wider than the window between two runs, at and off a tile edge
    for (int32_t first : {128, 150}) {
        Rows c;
        for (int32_t k = 0; k < 400; ++k) {
            c.chr.push_back(7);
            c.bp.push_back((k >= first ? 5000000 : 0) + static_cast<int64_t>(rnd() % 1000u));
            c.miss.push_back(k == 3);
        }
        check_case("gap after " + std::to_string(first), c, 1000);
        check_case("gap, window just short of it", c, 4999000);
        check_case("gap, window over it", c, 5001000);
        cases += 3;
    }
    check_fit();
    ++cases;
    printf("ok %d cases\n", cases);
    return 0;
}
