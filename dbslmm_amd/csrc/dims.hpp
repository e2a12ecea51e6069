// dims.hpp -- the tile sizes and limits that both the kernels and the plan's host layout
// (plan_layout.hpp) depend on (host only, no HIP).  Each is documented where its kernel lives.
#pragma once
#include <stdint.h>

namespace {
constexpr int kTile = 32;          // gram / cholesky tile edge (SNP slots)
}  // namespace

// one output tile of a Gram kernel: tile row ti, column tj <= ti of plan block `block` (-1: filler)
struct GramTile { int32_t block, ti, tj, pad; };

namespace gram {
constexpr int kGT = 128;                  // dbslmm_gram_big: output tile edge
constexpr int kHT = 256;                  // dbslmm_gram_huge: output tile edge
constexpr int kKpadAlign = 256;           // kpad: a multiple of dbslmm_gram_huge's K stage (gram::kHK)
}  // namespace gram

namespace chol {
constexpr int kSmallLd = 64;    // small path: ld <= 64 (m <= 63)
constexpr int kChebMaxM = 512;  // dbslmm_chol_cheb: ld > 64 blocks are below the tiled threshold
constexpr int kBT = 64;         // tiled-path tile edge (half the panel width)
constexpr int kRun2 = 1;        // trailing update: tiles per run (2 measured slower with two workgroups
                                // per CU: trail_bench m 9596 K 512, 63.5 vs 73.5 % of the f64 peak)
}  // namespace chol

namespace trsv {
constexpr int kT = 64;          // tile rows = the stored diagonal inverse blocks
}  // namespace trsv
