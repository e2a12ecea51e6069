// clump_check.cpp -- a stand-alone check of the clumping host code (clump_layout.hpp): no HIP, no
// library of the project.  Built with the host sanitizers by `make -C dbslmm_amd/csrc sanitize`
// (../bin/clump_asan) and run by tests/test_clump_host.py; also `g++ -std=c++17 clump_check.cpp`.
//
// For every candidate list below the layout is built and checked against what the kernel and the
// greedy walk need of it, worked out here independently in O(n^2): the position order, the band
// tile list (a tile is listed exactly when it holds a pair p < q on one chromosome within the
// window), its row and column indices, and clump_greedy over masks filled from a plain adjacency
// matrix against the greedy rule applied to that matrix.  The first violation prints and exits 1.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "../../dbslmm_amd/csrc/clump_layout.hpp"

namespace {

std::string g_case;
#define CHECK(cond, ...)                                                          \
    do {                                                                          \
        if (!(cond)) {                                                            \
            char msg_[512];                                                       \
            snprintf(msg_, sizeof msg_, __VA_ARGS__);                             \
            fprintf(stderr, "clump_check: %s: %s -- %s\n", g_case.c_str(), #cond, msg_); \
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

struct Cands {
    std::vector<int32_t> chr;
    std::vector<int64_t> bp;
};

bool in_window(const Cands& c, int32_t a, int32_t b, int64_t w) {
    const int64_t d = c.bp[a] - c.bp[b];
    return c.chr[a] == c.chr[b] && (d < 0 ? -d : d) <= w;
}

// layout + greedy of one list; link_rate: the share of in-window pairs the adjacency links
void check_case(const std::string& name, const Cands& c, int64_t window, uint32_t link_per_256) {
    g_case = name;
    const int32_t n = static_cast<int32_t>(c.chr.size());
    ClumpLayout L = build_clump_layout(n, c.chr.data(), c.bp.data(), window);
    clump_index_columns(L);
    // position order: a permutation sorted by (chr, bp, caller index)
    CHECK(L.n == n && L.n_trows == (n + 31) / 32, "n %d trows %d", L.n, L.n_trows);
    CHECK(static_cast<int32_t>(L.order.size()) == n && static_cast<int32_t>(L.rank.size()) == n, "sizes");
    std::vector<char> seen(static_cast<size_t>(n), 0);
    for (int32_t p = 0; p < n; ++p) {
        const int32_t k = L.order[p];
        CHECK(k >= 0 && k < n && !seen[k], "order[%d] = %d", p, k);
        seen[k] = 1;
        CHECK(L.rank[k] == p, "rank[%d] = %d, position %d", k, L.rank[k], p);
        if (p > 0) {
            const int32_t a = L.order[p - 1];
            const bool le = c.chr[a] != c.chr[k] ? c.chr[a] < c.chr[k] : c.bp[a] != c.bp[k] ? c.bp[a] < c.bp[k] : a < k;
            CHECK(le, "positions %d, %d out of order", p - 1, p);
        }
    }
    // the band: exactly the tiles with a pair p < q in the window
    std::set<std::pair<int32_t, int32_t>> want;
    for (int32_t p = 0; p < n; ++p)
        for (int32_t q = p + 1; q < n; ++q)
            if (in_window(c, L.order[p], L.order[q], window)) want.insert({p / 32, q / 32});
    CHECK(L.tiles.size() == want.size(), "%zu tiles listed, %zu hold a pair", L.tiles.size(), want.size());
    for (size_t t = 0; t < L.tiles.size(); ++t) {
        const ClumpTile& tl = L.tiles[t];
        CHECK(tl.ti >= 0 && tl.ti <= tl.tj && tl.tj < L.n_trows, "tile %zu = (%d, %d)", t, tl.ti, tl.tj);
        CHECK(want.count({tl.ti, tl.tj}) == 1, "tile (%d, %d) holds no pair", tl.ti, tl.tj);
        if (t > 0)
            CHECK(L.tiles[t - 1].ti < tl.ti || (L.tiles[t - 1].ti == tl.ti && L.tiles[t - 1].tj < tl.tj),
                  "tile %zu not after its predecessor", t);
    }
    // row and column indices
    CHECK(static_cast<int32_t>(L.row_ptr.size()) == L.n_trows + 1 && static_cast<int32_t>(L.col_ptr.size()) == L.n_trows + 1,
          "index sizes");
    CHECK(L.row_ptr[0] == 0 && L.row_ptr[L.n_trows] == static_cast<int32_t>(L.tiles.size()), "row_ptr ends");
    CHECK(L.col_ptr[0] == 0 && L.col_ptr[L.n_trows] == static_cast<int32_t>(L.tiles.size()), "col_ptr ends");
    for (int32_t T = 0; T < L.n_trows; ++T) {
        CHECK(L.row_ptr[T] <= L.row_ptr[T + 1] && L.col_ptr[T] <= L.col_ptr[T + 1], "pointers at %d", T);
        for (int32_t t = L.row_ptr[T]; t < L.row_ptr[T + 1]; ++t) CHECK(L.tiles[t].ti == T, "row %d lists tile %d", T, t);
        for (int32_t q = L.col_ptr[T]; q < L.col_ptr[T + 1]; ++q) {
            const int32_t t = L.col_tile[q];
            CHECK(t >= 0 && t < static_cast<int32_t>(L.tiles.size()) && L.tiles[t].tj == T, "column %d lists tile %d", T, t);
            if (q > L.col_ptr[T]) CHECK(L.col_tile[q - 1] < t, "column %d lists tile %d twice or out of order", T, t);
        }
    }
    // an adjacency on caller indices: symmetric, in-window pairs only, no self link
    std::vector<char> adj(static_cast<size_t>(n) * n, 0);
    for (int32_t a = 0; a < n; ++a)
        for (int32_t b = a + 1; b < n; ++b)
            if (in_window(c, a, b, window) && (rnd() & 255u) < link_per_256)
                adj[static_cast<size_t>(a) * n + b] = adj[static_cast<size_t>(b) * n + a] = 1;
    // the kernel's masks of that adjacency: bits only for positions p < q, both inside the list
    std::vector<uint32_t> masks(L.tiles.size() * kClumpMaskWords, 0);
    for (size_t t = 0; t < L.tiles.size(); ++t)
        for (int r = 0; r < 32; ++r)
            for (int cc = 0; cc < 32; ++cc) {
                const int32_t p = 32 * L.tiles[t].ti + r, q = 32 * L.tiles[t].tj + cc;
                if (p >= q || q >= n) continue;
                if (!adj[static_cast<size_t>(L.order[p]) * n + L.order[q]]) continue;
                masks[t * kClumpMaskWords + r] |= 1u << cc;
                masks[t * kClumpMaskWords + 32 + cc] |= 1u << r;
            }
    // every link lies in a listed tile (else the masks above lost it)
    for (int32_t p = 0; p < n; ++p)
        for (int32_t q = p + 1; q < n; ++q)
            if (adj[static_cast<size_t>(L.order[p]) * n + L.order[q]])
                CHECK(want.count({p / 32, q / 32}) == 1, "link (%d, %d) outside the band", p, q);
    std::vector<int32_t> got(static_cast<size_t>(n) + 1, -7), ref(static_cast<size_t>(n), -1);
    const int32_t ni = clump_greedy(L, masks.data(), got.data());
    CHECK(got[n] == -7, "clump_greedy wrote past index_of");
    int32_t ni_ref = 0;
    for (int32_t k = 0; k < n; ++k) {
        if (ref[k] >= 0) continue;
        ref[k] = k;
        ++ni_ref;
        for (int32_t j = 0; j < n; ++j)
            if (adj[static_cast<size_t>(k) * n + j] && ref[j] < 0) ref[j] = k;
    }
    CHECK(ni == ni_ref, "%d index SNPs, the plain walk finds %d", ni, ni_ref);
    for (int32_t k = 0; k < n; ++k) CHECK(got[k] == ref[k], "index_of[%d] = %d, the plain walk gives %d", k, got[k], ref[k]);
}

// n candidates on n_chr chromosomes at random base pairs below span, in random (unsorted) order
Cands random_cands(int32_t n, int32_t n_chr, int64_t span) {
    Cands c;
    for (int32_t k = 0; k < n; ++k) {
        c.chr.push_back(1 + static_cast<int32_t>(rnd() % static_cast<uint32_t>(n_chr)));
        c.bp.push_back(static_cast<int64_t>(rnd() % static_cast<uint64_t>(span)));
    }
    return c;
}

}  // namespace

int main() {
    int cases = 0;
    // candidate counts at the tile edges; one chromosome, everything inside the window
    for (int32_t n : {0, 1, 31, 32, 33, 65}) {
        check_case("dense n=" + std::to_string(n), random_cands(n, 1, 1000), 1000, 64);
        check_case("dense all-linked n=" + std::to_string(n), random_cands(n, 1, 1000), 1000, 256);
        check_case("dense none-linked n=" + std::to_string(n), random_cands(n, 1, 1000), 1000, 0);
        cases += 3;
    }
    // several chromosomes that share bp values (the same small range on each): no tile pair across
    for (int32_t n : {33, 65, 200}) {
        check_case("shared bp n=" + std::to_string(n), random_cands(n, 4, 50), 10, 128);
        check_case("shared bp, equal positions n=" + std::to_string(n), random_cands(n, 3, 4), 0, 200);
        cases += 2;
    }
    // a real band: a window far narrower than the span, unsorted input, more than one tile wide
    for (int32_t n : {65, 300, 700}) {
        check_case("band n=" + std::to_string(n), random_cands(n, 2, 100000), 20000, 96);
        check_case("narrow band n=" + std::to_string(n), random_cands(n, 1, 100000), 500, 256);
        cases += 2;
    }
    // a gap wider than the window between two runs, and the empty stretch it leaves in the band
    {
        Cands c;
        for (int32_t k = 0; k < 150; ++k) {
            c.chr.push_back(7);
            c.bp.push_back((k % 2 ? 5000000 : 0) + static_cast<int64_t>(rnd() % 1000u));
        }
        check_case("gap", c, 1000, 128);
        check_case("gap, window just short of it", c, 4999000, 128);
        check_case("gap, window over it", c, 5001000, 128);
        cases += 3;
    }
    // window_bp = 0: only candidates at one position are linked (repeats included)
    {
        Cands c;
        for (int32_t k = 0; k < 100; ++k) {
            c.chr.push_back(1 + k % 2);
            c.bp.push_back(10 * (k / 5));
        }
        check_case("window 0", c, 0, 256);
        check_case("window 0, sorted descending", Cands{std::vector<int32_t>(c.chr.rbegin(), c.chr.rend()),
                                                        std::vector<int64_t>(c.bp.rbegin(), c.bp.rend())}, 0, 256);
        cases += 2;
    }
    // the chain A - B - C in priority order A, B, C: C is linked to B only and stays an index SNP
    {
        g_case = "chain";
        const int32_t chr[3] = {1, 1, 1};
        const int64_t bp[3] = {100, 200, 300};
        ClumpLayout L = build_clump_layout(3, chr, bp, 1000);
        clump_index_columns(L);
        CHECK(L.tiles.size() == 1, "%zu tiles", L.tiles.size());
        std::vector<uint32_t> m(kClumpMaskWords, 0);
        m[0] = 1u << 1;  m[32 + 1] = 1u << 0;      // A - B
        m[1] = 1u << 2;  m[32 + 2] = 1u << 1;      // B - C
        int32_t idx[3];
        const int32_t ni = clump_greedy(L, m.data(), idx);
        CHECK(ni == 2 && idx[0] == 0 && idx[1] == 0 && idx[2] == 2, "index_of = %d %d %d", idx[0], idx[1], idx[2]);
        ++cases;
    }
    printf("ok %d cases\n", cases);
    return 0;
}
