// ldsc_layout.hpp -- the host side of dbslmm_ld_scores (host only, no HIP): the position order of
// the listed rows, the window of every position, and the band of 128 x 128 pair tiles
// dbslmm_l2_tiles (ldscore.hip) runs over.  Integer-only and deterministic;
// tests/host/ldsc_check.cpp checks it from first principles under the host sanitizers.
//
// The construction is build_clump_layout's (clump_layout.hpp) at the 128-row tile of the dense
// case: rows sorted by (chr, bp, caller index), where the rows inside the window of a row form one
// contiguous run [lo(p), hi(p)], so the tiles that hold an in-window pair form a band along the
// diagonal: none across a chromosome change, none across a gap wider than the window.  The
// diagonal tile of every tile row is listed whatever the window (the self term of an LD score).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <numeric>
#include <vector>

constexpr int kL2Tile = 128;            // tile edge of dbslmm_l2_tiles (one workgroup per tile)
constexpr int kL2SlotWords = 256;       // per tile: 128 row sums, then 128 column sums (fp64)

// tile (ti, tj), tj >= ti, of the pair matrix in position order; missing != 0: one of its up to
// 256 rows has a missing call (the tile takes the four-product path)
struct L2Tile { int32_t ti, tj, missing, pad; };

struct LdscLayout {
    int32_t n = 0;                      // listed rows
    int32_t n_trows = 0;                // tile rows = ceil(n / 128)
    std::vector<int32_t> order;         // position p -> caller index
    std::vector<int32_t> lo, hi;        // position p -> first / last position inside its window
    std::vector<L2Tile> tiles;          // sorted by (ti, tj); row I holds (I, I), (I, I + 1), ... without a gap
    std::vector<int32_t> row_ptr;       // tiles of tile row I: [row_ptr[I], row_ptr[I + 1])
    std::vector<int32_t> col_lo;        // tile column J is held by the tile rows [col_lo[J], J]:
                                        // tile (I, J) has index row_ptr[I] + (J - I)
};

// row_missing (optional): per caller index, != 0 when the row has a missing call.
// hi(p) = the last position q >= p on p's chromosome with bp_q - bp_p <= window_bp and lo(p) the
// first such position on the other side; neither decreases with p, so tile row I reaches tile
// column hi(last p of I) / 128, every tile between the diagonal and that column holds an in-window
// pair p < q, and the tile rows that reach a tile column are consecutive.
inline LdscLayout build_ldsc_layout(int32_t n, const int32_t* chr, const int64_t* bp, int64_t window_bp,
                                    const uint8_t* row_missing) {
    LdscLayout L;
    L.n = n;
    L.n_trows = (n + kL2Tile - 1) / kL2Tile;
    L.order.resize(static_cast<size_t>(n));
    std::iota(L.order.begin(), L.order.end(), 0);
    std::stable_sort(L.order.begin(), L.order.end(), [&](int32_t a, int32_t b) {
        return chr[a] != chr[b] ? chr[a] < chr[b] : bp[a] < bp[b];
    });
    L.lo.resize(static_cast<size_t>(n));
    L.hi.resize(static_cast<size_t>(n));
    for (int32_t p = 0, q = 0, l = 0; p < n; ++p) {     // two pointers: q = hi(p), l = lo(p)
        q = std::max(q, p);
        const int32_t a = L.order[static_cast<size_t>(p)];
        while (q + 1 < n && chr[L.order[static_cast<size_t>(q) + 1]] == chr[a] &&
               bp[L.order[static_cast<size_t>(q) + 1]] - bp[a] <= window_bp)
            ++q;
        while (l < p && (chr[L.order[static_cast<size_t>(l)]] != chr[a] ||
                         bp[a] - bp[L.order[static_cast<size_t>(l)]] > window_bp))
            ++l;
        L.hi[static_cast<size_t>(p)] = q;
        L.lo[static_cast<size_t>(p)] = l;
    }
    std::vector<uint8_t> trow_missing(static_cast<size_t>(L.n_trows), 0);
    if (row_missing)
        for (int32_t p = 0; p < n; ++p)
            if (row_missing[L.order[static_cast<size_t>(p)]]) trow_missing[static_cast<size_t>(p / kL2Tile)] = 1;
    L.row_ptr.assign(static_cast<size_t>(L.n_trows) + 1, 0);
    L.col_lo.resize(static_cast<size_t>(L.n_trows));
    for (int32_t I = 0, J0 = 0; I < L.n_trows; ++I) {
        const int32_t last = std::min(n, kL2Tile * (I + 1)) - 1;
        const int32_t reach = L.hi[static_cast<size_t>(last)] / kL2Tile;
        for (int32_t J = I; J <= reach; ++J)
            L.tiles.push_back({I, J, trow_missing[static_cast<size_t>(I)] | trow_missing[static_cast<size_t>(J)], 0});
        for (J0 = std::max(J0, I); J0 <= reach; ++J0) L.col_lo[static_cast<size_t>(J0)] = I;   // first row to reach J0
        L.row_ptr[static_cast<size_t>(I) + 1] = static_cast<int32_t>(L.tiles.size());
    }
    return L;
}

// n_window of the entry point: listed rows inside the window of caller row k, k itself included
inline void ldsc_window_counts(const LdscLayout& L, int32_t* n_window) {
    for (int32_t p = 0; p < L.n; ++p)
        n_window[L.order[static_cast<size_t>(p)]] = L.hi[static_cast<size_t>(p)] - L.lo[static_cast<size_t>(p)] + 1;
}
