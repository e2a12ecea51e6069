// clump_layout.hpp -- the host side of dbslmm_clump / dbslmm_ld_r2 (host only, no HIP): the
// position order of the candidates, the band of 32 x 32 pair tiles dbslmm_r2_tiles (clump.hip) runs
// over, and the greedy walk over the masks it returns.  Integer-only and deterministic;
// tests/host/clump_check.cpp checks every part from first principles under the host sanitizers.
//
// Candidates arrive in the caller's PRIORITY order (most significant first).  The tiles live in
// POSITION order -- sorted by (chr, bp, caller index) -- where the pairs that can be linked (same
// chromosome, |bp_i - bp_j| <= window_bp) of a candidate form one contiguous run, so the tiles that
// hold such a pair form a band along the diagonal: none across a chromosome change, none across a
// gap wider than the window.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <numeric>
#include <vector>

constexpr int kClumpTile = 32;          // tile edge of dbslmm_r2_tiles (one wave per tile)
constexpr int kClumpMaskWords = 64;     // per tile: 32 row masks, then 32 column masks

// tile (ti, tj), tj >= ti, of the pair matrix in position order
struct ClumpTile { int32_t ti, tj; };

struct ClumpLayout {
    int32_t n = 0;                      // candidates
    int32_t n_trows = 0;                // tile rows = ceil(n / 32)
    std::vector<int32_t> order;         // position p -> caller index
    std::vector<int32_t> rank;          // caller index -> position
    std::vector<ClumpTile> tiles;       // sorted by (ti, tj)
    std::vector<int32_t> row_ptr;       // tiles of tile row I: [row_ptr[I], row_ptr[I + 1])
    std::vector<int32_t> col_ptr;       // tiles of tile column J: col_tile[col_ptr[J] .. col_ptr[J + 1])
    std::vector<int32_t> col_tile;
};

// The band for clumping.  hi(p) = the last position q >= p on p's chromosome with bp_q - bp_p <=
// window_bp; it never decreases with p, so tile row I reaches tile column hi(last p of I) / 32 and
// every tile between the diagonal and that column holds a linked-candidate pair p < q.  The
// diagonal tile is listed when it holds one (two positions of the row within the window).
inline ClumpLayout build_clump_layout(int32_t n, const int32_t* chr, const int64_t* bp, int64_t window_bp) {
    ClumpLayout L;
    L.n = n;
    L.n_trows = (n + kClumpTile - 1) / kClumpTile;
    L.order.resize(static_cast<size_t>(n));
    std::iota(L.order.begin(), L.order.end(), 0);
    std::stable_sort(L.order.begin(), L.order.end(), [&](int32_t a, int32_t b) {
        return chr[a] != chr[b] ? chr[a] < chr[b] : bp[a] < bp[b];
    });
    L.rank.resize(static_cast<size_t>(n));
    for (int32_t p = 0; p < n; ++p) L.rank[static_cast<size_t>(L.order[p])] = p;
    std::vector<int32_t> hi(static_cast<size_t>(n));
    for (int32_t p = 0, q = 0; p < n; ++p) {            // two pointers: q = hi(p)
        q = std::max(q, p);
        const int32_t a = L.order[p];
        while (q + 1 < n && chr[L.order[q + 1]] == chr[a] && bp[L.order[q + 1]] - bp[a] <= window_bp) ++q;
        hi[static_cast<size_t>(p)] = q;
    }
    L.row_ptr.assign(static_cast<size_t>(L.n_trows) + 1, 0);
    for (int32_t I = 0; I < L.n_trows; ++I) {
        const int32_t p0 = kClumpTile * I, p1 = std::min(n, p0 + kClumpTile);   // positions [p0, p1)
        bool diag = false;
        for (int32_t p = p0; p + 1 < p1 && !diag; ++p) diag = hi[static_cast<size_t>(p)] > p;
        if (diag) L.tiles.push_back({I, I});
        for (int32_t J = I + 1; J <= hi[static_cast<size_t>(p1 - 1)] / kClumpTile; ++J) L.tiles.push_back({I, J});
        L.row_ptr[static_cast<size_t>(I) + 1] = static_cast<int32_t>(L.tiles.size());
    }
    return L;
}

// Every tile tj >= ti over n rows in the caller's own order: the dense matrix of dbslmm_ld_r2.
inline ClumpLayout build_dense_layout(int32_t n) {
    ClumpLayout L;
    L.n = n;
    L.n_trows = (n + kClumpTile - 1) / kClumpTile;
    L.order.resize(static_cast<size_t>(n));
    std::iota(L.order.begin(), L.order.end(), 0);
    L.rank = L.order;
    L.row_ptr.assign(static_cast<size_t>(L.n_trows) + 1, 0);
    for (int32_t I = 0; I < L.n_trows; ++I) {
        for (int32_t J = I; J < L.n_trows; ++J) L.tiles.push_back({I, J});
        L.row_ptr[static_cast<size_t>(I) + 1] = static_cast<int32_t>(L.tiles.size());
    }
    return L;
}

// the tiles of every tile column (the greedy walk needs a candidate's neighbours on both sides)
inline void clump_index_columns(ClumpLayout& L) {
    L.col_ptr.assign(static_cast<size_t>(L.n_trows) + 1, 0);
    for (const ClumpTile& t : L.tiles) L.col_ptr[static_cast<size_t>(t.tj) + 1]++;
    for (int32_t J = 0; J < L.n_trows; ++J) L.col_ptr[static_cast<size_t>(J) + 1] += L.col_ptr[static_cast<size_t>(J)];
    L.col_tile.resize(L.tiles.size());
    std::vector<int32_t> fill(L.col_ptr.begin(), L.col_ptr.end() - 1);
    for (size_t t = 0; t < L.tiles.size(); ++t)
        L.col_tile[static_cast<size_t>(fill[static_cast<size_t>(L.tiles[t].tj)]++)] = static_cast<int32_t>(t);
}

// PLINK's greedy rule over the kernel's masks.  masks: kClumpMaskWords words per tile of L.tiles;
// for tile (ti, tj) bit c of word r says that positions p = 32 ti + r and q = 32 tj + c, p < q, are
// linked (same chromosome, inside the window, r2 >= the threshold), and bit r of word 32 + c says
// the same of the same pair.  The walk follows the caller's order k = 0, 1, ...: a candidate not
// yet absorbed becomes an index SNP (index_of[k] = k) and absorbs its not yet absorbed neighbours
// (index_of = k) -- its neighbours only: absorption is not transitive.  Returns the index count.
inline int32_t clump_greedy(const ClumpLayout& L, const uint32_t* masks, int32_t* index_of) {
    for (int32_t k = 0; k < L.n; ++k) index_of[k] = -1;
    int32_t n_index = 0;
    auto absorb = [&](int32_t k, int32_t t0, uint32_t m) {
        for (; m; m &= m - 1) {
            const int32_t q = kClumpTile * t0 + __builtin_ctz(m);
            if (q >= L.n) continue;
            const int32_t kq = L.order[static_cast<size_t>(q)];
            if (index_of[kq] < 0) index_of[kq] = k;
        }
    };
    for (int32_t k = 0; k < L.n; ++k) {
        if (index_of[k] >= 0) continue;
        index_of[k] = k;
        ++n_index;
        const int32_t p = L.rank[static_cast<size_t>(k)], T = p / kClumpTile, e = p % kClumpTile;
        for (int32_t t = L.row_ptr[static_cast<size_t>(T)]; t < L.row_ptr[static_cast<size_t>(T) + 1]; ++t)
            absorb(k, L.tiles[static_cast<size_t>(t)].tj, masks[static_cast<size_t>(t) * kClumpMaskWords + e]);
        for (int32_t c = L.col_ptr[static_cast<size_t>(T)]; c < L.col_ptr[static_cast<size_t>(T) + 1]; ++c) {
            const int32_t t = L.col_tile[static_cast<size_t>(c)];
            absorb(k, L.tiles[static_cast<size_t>(t)].ti, masks[static_cast<size_t>(t) * kClumpMaskWords + kClumpTile + e]);
        }
    }
    return n_index;
}
