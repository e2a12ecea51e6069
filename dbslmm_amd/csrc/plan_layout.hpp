// plan_layout.hpp -- the host layout of a plan as a pure function of the problem, the options and
// the number of compute units (host only, no HIP): slots and per-block ld, the three Gram tile
// lists with their per-XCD queues, the Cholesky work order, the launch lists of the tiled
// factorisation (build_tiled) and the substitution ticket lists.  dbslmm_plan_create (plan.hip)
// calls build_plan_layout once and uploads what it returns; tests/host/layout_check.cpp checks the
// same lists from first principles on the CPU, under the host sanitizers.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <numeric>
#include <string>
#include <vector>

#include "../../include/dbslmm_hip.h"
#include "dims.hpp"
#include "out_ranges.hpp"

constexpr int kTiledMinDefault = 384;   // blocks with m >= this take the multi-workgroup path
                                        // (round 4, with the per-group substitutions: config 4
                                        // 44.1-44.3 -> 43.2-43.3 ms, one run in four 45.0; configs
                                        // 3 / 5 -0.1 / -0.2 ms; 512 before, 320 no better)
constexpr int kTiledMinSmall = 256;     // the same when no block reaches 512 SNPs (config 2)
constexpr int kGramBigMinDefault = 96;  // blocks with m >= this take the 128 x 128 Gram kernel
constexpr int kGramHugeMinDefault = 384; // ... and the 256 x 256 one from here (swept: configs 3, 5)
constexpr int kTChebMaxM = 4096;         // whole-block Chebyshev passes: blocks of <= 64 tiles
constexpr int kLeadMinDefault = 1536;    // lead group: m >= max(this, m_max / 8) (dbslmm_options.lead_min)
constexpr int kXcd = 8;                 // workgroup id e runs on XCD e % 8
constexpr int kSuper = 2;               // regions (128 columns) per super step
constexpr int kWideSuper = 4;           // ... for blocks of m >= kWideMin (half the C traffic per
constexpr int kWideMin = 4096;          //     flop; config 5 35.4 -> 34.3 ms/step)
constexpr int kTiledMaxM = 255 * 128;   // tiled path: 128-row tile and region indices < 256
constexpr int kGramSq = 4;              // 2D tile squares per XCD of the 256-tile Gram
constexpr int kTrailSq = 8;             // 2D squares (in 128-tiles) per XCD of the trailing update
constexpr int kRowEntryBytes = 16;      // one entry {sum, sumsq, nmiss, 0} of the image's row table

inline int64_t round_up(int64_t x, int64_t a) { return (x + a - 1) / a * a; }
// bytes of one .bed row of n_ref individuals
inline int64_t bed_row_bytes(int32_t n_ref) { return n_ref / 4 + (n_ref % 4 ? 1 : 0); }

// one launch of the tiled sequence: the active blocks and the prefix of their work items
struct TLaunch {
    int kind;         // 1 panel, 4 region, 5 trailing (128 x 128 tiles); items are int32 pairs
                      // carrying each block's own step
    int step;
    int32_t off;      // into d_tlist: act[n] then pfx[n + 1]
    int32_t n;
    int32_t items;    // workgroups
    int32_t nk = 1;   // trailing: K = 128 nk (regions step .. step+nk-1); region: pending panels
    int strm = 0;     // 0: the sequence's chain stream, 1: its bulk-trailing stream
};
// sync entries of a launch list (lookahead): kind 6 records tiled event `step` on stream `strm`,
// kind 7 makes stream `strm` wait for it
constexpr int kTlRecord = 6, kTlWait = 7;

struct PlanLayout {
    // what a plan keeps after its creation (the base of dbslmm_plan: each field lives here only)
    struct Kept {
        int64_t n_s = 0, n_l = 0, kpad = 0;
        int32_t n_slots = 0, n_nonempty = 0, n_tiles = 0;
        int64_t M_elems = 0;
        int32_t n_large = 0, n_small = 0;   // Cholesky paths (ld > 64 / ld <= 64); d_order = [large | small]
        int32_t n_tiled = 0;                // blocks on the multi-workgroup path (not in d_order)
        std::vector<TLaunch> tl;            // the tiled sequence (of the lead group when there is one)
        std::vector<TLaunch> tl_rest;       // the other tiled blocks' sequence (lead group only)
        int32_t n_btiles = 0;
        int32_t n_htiles = 0;
        int32_t n_htiles_lead = 0;         // ... of which the first n_htiles_lead are the lead group's,
        int32_t n_htiles_tiled = 0;        //     the first n_htiles_tiled the tiled blocks' (then the rest)
        bool early_fork = false;           // every tiled block's Gram is in those: the tiled sequences
                                           // may start before the other blocks' Gram
        std::vector<int32_t> h_ld;  // per non-empty block
        std::vector<int32_t> h_m;   // per non-empty block
        std::vector<int32_t> h_tb;  // blocks on the tiled path
        std::vector<int32_t> h_empty;  // original ids of empty blocks
        std::vector<int32_t> h_blk_id; // per non-empty block: its original id
        std::vector<int64_t> h_matoff; // per non-empty block: offset of its matrix in a copy
        std::vector<int32_t> h_slot_out;  // slot -> small index s, large -1-l, padding INT32_MIN
        std::vector<int32_t> h_ms, h_row0;   // per non-empty block: small SNPs, first slot
        bool has_large = false;        // some block has large SNPs
        std::vector<OutRange> h_orange;   // per route block: its ranges of the caller's arrays
        // workload figures
        double wl[DBSLMM_WORKLOAD_LEN] = {0};
        int32_t n_titems = 0, n_tflags = 0;
        int32_t tiled_min = 0;                   // blocks with m >= this are on the tiled path
        bool large_cheb_ok = true;               // dbslmm_options.large_cheb and every chol_large block
                                                 // fits dbslmm_chol_cheb (ld <= chol::kChebMaxM)
        // dbslmm_options.sub_split: the substitution lists are ordered [lead group | rest group], each
        // group a contiguous item range of d_tri_f / d_tri_b and block range of d_tb
        bool sub_split = false;
        int32_t n_titems_lead = 0, n_tb_lead = 0, sub_grid_lead = 0, sub_grid_rest = 0;
        // sub_split = 2: the rest group's h2f Chebyshev passes as whole-block launches (dbslmm_tcheb):
        // its blocks, largest first, and the LDS stride of the work vector (64 x the most tiles)
        bool sub_block = false;
        int32_t n_tcheb = 0, tcheb_vld = 0;
    };
    Kept keep;
    // uploaded once, then released
    std::vector<int32_t> slot_pos, slot_block;   // per slot: bed row (-1 = pad), block
    std::vector<double> z;                       // per slot
    std::vector<GramTile> tiles;                 // 32 x 32 tiles of the small blocks (dbslmm_gram_i8)
    std::vector<GramTile> btiles;                // 128 x 128 tiles of the mid blocks, per-XCD queues
    std::vector<GramTile> htiles;                // 256 x 256 tiles of the big blocks, per-XCD queues
    std::vector<int32_t> order;                  // [large | small] non-tiled blocks, each largest first
    std::vector<int32_t> tlist;                  // work items of tl, then of tl_rest
    std::vector<int32_t> tri_f, tri_b, foff;     // substitution tickets (b, I) / mirrored; first flag per block
    std::vector<int32_t> tcheb_list;             // sub_block: the rest group's blocks, largest first
    // the thresholds the options resolved to (lead_min INT64_MAX: no lead group)
    int64_t gram_big_min = 0, gram_huge_min = 0, lead_min = 0;
};

// Launch list of the tiled sequence for the blocks `tb0` (plan block indices), each replicated over
// `copies` independent factorisations (h2f tuning: item block id bq = b + c * nb addresses copy c).
// A block's factorisation is a chain of super steps of R regions (128 columns each; R = 4 for
// blocks of m >= kWideMin, else 2 -- a property of the block, so its factorisation does not
// depend on the other blocks of the sequence): region(0), then per super step
//   panel(r0) -> for r = r0+1 .. r0+R-1: region(r) [+ its pending update from panels r0 .. r-1]
//   -> panel(r) [+ the pending update of its rows' region-r columns] -> trailing K = 128 R of
//   everything right of the super step (the next first region included) -> region(r0 + R),
// then one persistent backward substitution (run_pbwd).  Every launch of a given slot holds the
// same kind of work for all blocks, each at its OWN local step (work items carry it): blocks are
// left-aligned (all start at launch 0; right alignment -- a block with fewer super steps starting
// later -- measured no gain at configs 3-5).  Each work item is two int32:
// [block / tile, (local step << 8) | pending panels or K multiple].
inline void build_tiled(const std::vector<int32_t>& mv, const std::vector<int32_t>& tb0, int copies,
                        int nb, std::vector<TLaunch>& tl, std::vector<int32_t>& tlist) {
    struct Blk { int32_t bq; int T64, Tz64, T2, Tz2, nr, R, S, off; };
    int Rmax = 1;
    const int run2 = chol::kRun2;
    std::vector<Blk> bl;
    int G = 0;
    for (int c = 0; c < copies; ++c)
        for (int32_t b : tb0) {
            Blk k;
            k.bq = b + c * nb;
            k.T64 = (mv[b] + chol::kBT - 1) / chol::kBT;
            k.Tz64 = mv[b] / chol::kBT;
            k.T2 = (mv[b] + 127) / 128;
            k.Tz2 = mv[b] / 128;
            k.nr = (k.T64 + 1) / 2;
            k.R = mv[b] >= kWideMin ? kWideSuper : kSuper;
            Rmax = std::max(Rmax, k.R);
            k.S = (k.nr + k.R - 1) / k.R;
            G = std::max(G, k.S);
            bl.push_back(k);
        }
    for (auto& k : bl) k.off = 0;   // left-aligned (right alignment measured: no gain at configs 3-5)
    auto push_pairs = [&](int kind, const std::vector<int32_t>& v) {   // plain pair list
        if (v.empty()) return;
        TLaunch L{kind, 0, static_cast<int32_t>(tlist.size()), static_cast<int32_t>(v.size() / 2),
                  static_cast<int32_t>(v.size() / 2)};
        tlist.insert(tlist.end(), v.begin(), v.end());
        tl.push_back(L);
    };
    auto region_launch = [&](const std::vector<int32_t>& v) { push_pairs(4, v); };
    auto panel_launch = [&](const std::vector<int32_t>& v) { push_pairs(1, v); };
    auto sync = [&](int kind, int ev, int strm) {
        TLaunch L{kind, ev, 0, 0, 0};
        L.strm = strm;
        tl.push_back(L);
    };
    auto trailing_launch = [&](std::vector<std::vector<int32_t>>& q, int run, int strm) {
        TLaunch L{5, 0, static_cast<int32_t>(tlist.size()), run, 0};
        L.strm = strm;
        size_t qmax = 0;
        for (const auto& v : q) qmax = std::max(qmax, v.size() / 2);
        // work item e (pair) runs on XCD e % 8
        for (size_t i = 0; i < qmax; ++i)
            for (int x = 0; x < kXcd; ++x) {
                if (2 * i < q[x].size()) {
                    tlist.push_back(q[x][2 * i]);
                    tlist.push_back(q[x][2 * i + 1]);
                } else {
                    tlist.push_back(-1);
                    tlist.push_back(0);
                }
            }
        L.items = static_cast<int32_t>((tlist.size() - L.off) / 2);
        if (L.items > 0) tl.push_back(L);
    };
    {   // region 0 of the blocks that start at super step 0
        std::vector<int32_t> v;
        for (const auto& k : bl)
            if (k.off == 0) { v.push_back(k.bq); v.push_back(0); }
        region_launch(v);
    }
    for (int g = 0; g < G; ++g) {
        auto active = [&](const Blk& k) { return g >= k.off && g - k.off < k.S; };
        std::vector<int32_t> v;
        for (const auto& k : bl)      // panel(r0)
            if (active(k)) {
                const int r0 = (g - k.off) * k.R;
                for (int i = 2 * r0 + 2; i <= k.Tz64; ++i) { v.push_back((k.bq << 16) | i); v.push_back(r0 << 8); }
            }
        panel_launch(v);
        for (int j = 1; j < Rmax; ++j) {
            std::vector<int32_t> rv, pv;
            for (const auto& k : bl)
                if (active(k) && j < k.R) {
                    const int r = (g - k.off) * k.R + j;
                    if (r >= k.nr) continue;
                    rv.push_back(k.bq);
                    rv.push_back((r << 8) | j);
                    for (int i = 2 * r + 2; i <= k.Tz64; ++i) { pv.push_back((k.bq << 16) | i); pv.push_back((r << 8) | j); }
                }
            region_launch(rv);
            panel_launch(pv);
        }
        // trailing: 128 x 128 tiles (I, J) right of the super step, rl + jlo <= J <= rl + jhi (near:
        // the block's next R columns, far: the rest), LPT over per-XCD queues by tile row
        auto trailing = [&](bool near, int strm, int run_force) {
            std::vector<std::vector<int32_t>> q(kXcd);
            std::vector<int64_t> load(kXcd, 0);
            int64_t ntiles = 0;
            for (const auto& k : bl)
                if (active(k)) {
                    const int r0 = (g - k.off) * k.R, rl = std::min(r0 + k.R, k.nr) - 1;
                    if (rl + 1 >= k.nr) continue;
                    const int jlo = near ? 1 : k.R + 1, jhi = near ? k.R : 1 << 20;
                    for (int I = rl + jlo; I <= k.Tz2; ++I) {
                        const int jm = std::min(std::min(I, k.T2 - 1), rl + jhi);
                        if (jm >= rl + jlo) ntiles += jm - (rl + jlo) + 1;
                    }
                }
            const int run = run_force ? run_force : (ntiles >= 1024 ? run2 : 1);
            // 2-D placement: the tiles are cut into squares of kTrailSq x kTrailSq (tile rows I x tile
            // columns J), a square's tiles go to one XCD, squares LPT over the XCDs.  The ~32 CUs of
            // an XCD then work on one or two squares at a time, which read kTrailSq row panels and
            // kTrailSq column panels between them through that XCD's L2 (keyed on the tile row
            // alone, every XCD read every column panel from HBM)
            // (smaller squares when a launch has few tiles, so the LPT over the XCDs stays balanced)
            const int sq_w = ntiles >= 16 * kTrailSq * kTrailSq ? kTrailSq : ntiles >= 512 ? kTrailSq / 2 : 2;
            struct Sq { int32_t bq, meta; int i0, i1, j0, j1; int64_t n; };
            std::vector<Sq> sqs;
            for (const auto& k : bl)
                if (active(k)) {
                    const int r0 = (g - k.off) * k.R, rl = std::min(r0 + k.R, k.nr) - 1;
                    if (rl + 1 >= k.nr) continue;
                    const int jlo = near ? 1 : k.R + 1, jhi = near ? k.R : 1 << 20;
                    const int meta = (r0 << 8) | (rl - r0 + 1);
                    const int jcap = std::min(k.T2 - 1, rl + jhi);
                    for (int i0 = rl + jlo; i0 <= k.Tz2; i0 += sq_w)
                        for (int j0 = rl + jlo; j0 <= std::min(i0 + sq_w - 1, jcap); j0 += sq_w) {
                            const int i1 = std::min(i0 + sq_w - 1, k.Tz2), j1 = std::min(j0 + sq_w - 1, jcap);
                            int64_t n = 0;
                            for (int I = i0; I <= i1; ++I) n += std::max(0, std::min(I, j1) - j0 + 1);
                            if (n > 0) sqs.push_back(Sq{k.bq, meta, i0, i1, j0, j1, n});
                        }
                }
            std::stable_sort(sqs.begin(), sqs.end(), [](const Sq& a, const Sq& b) { return a.n > b.n; });
            for (const Sq& sq : sqs) {
                const int x = static_cast<int>(std::min_element(load.begin(), load.end()) - load.begin());
                for (int I = sq.i0; I <= sq.i1; ++I) {
                    const int jm = std::min(I, sq.j1);
                    for (int J = sq.j0; J <= jm; J += run) {
                        q[x].push_back((sq.bq << 16) | (I << 8) | J);
                        q[x].push_back(sq.meta);
                    }
                }
                load[x] += sq.n;
            }
            trailing_launch(q, run, strm);
        };
        // lookahead: the next super step's R tile columns ("near": chain stream, one tile per
        // work item) are updated first; the rest ("far": stream 1) overlaps the next super step's
        // regions and panels.  Tiles of near(g) were far(g-1)'s.
        sync(kTlRecord, 2 * g, 0);
        if (g > 0) sync(kTlWait, 2 * g - 1, 0);
        trailing(true, 0, 1);
        sync(kTlWait, 2 * g, 1);
        trailing(false, 1, 0);
        sync(kTlRecord, 2 * g + 1, 1);
        {   // next super step's first region; region 0 of the blocks that start at g + 1
            std::vector<int32_t> v;
            for (const auto& k : bl) {
                if (active(k)) {
                    const int r0 = (g - k.off) * k.R, rn = r0 + k.R;
                    if (rn < k.nr) { v.push_back(k.bq); v.push_back(rn << 8); }
                } else if (k.off == g + 1) {
                    v.push_back(k.bq);
                    v.push_back(0);
                }
            }
            region_launch(v);
        }
    }
    if (G > 0) sync(kTlWait, 2 * G - 1, 0);   // the last far update
    // (the backward substitution is one persistent launch after the sequence: run_pbwd)
}

// The layout of problem `pr` under options `op` on a GPU of n_cu compute units.  Reads the CSR
// arrays, the bed rows' indices and the z-scores, never the genotype bytes.  DBSLMM_OK, or
// DBSLMM_E_ARG with the reason in err.
inline int build_plan_layout(const dbslmm_problem& pr, const dbslmm_options& op, int n_cu, PlanLayout& out,
                             std::string& err) {
    if (!(op.tiled_min >= 0 && op.gram_big_min >= 0 && op.gram_huge_min >= 0 &&
          (op.h2f_mode == 0 || op.h2f_mode == 1) && op.cheb_tol >= 0.0 &&
          (op.large_cheb == 0 || op.large_cheb == -1) && (op.cheb_fused == 0 || op.cheb_fused == 1) &&
          op.debug_delay_us >= -100000 && op.debug_delay_us <= 100000 &&
          (op.debug_stop == 0 || op.debug_stop == 1) && op.sub_split >= -1 && op.sub_split <= 2 &&
          op.sub_grid_lead >= 0 && op.sub_grid_rest >= 0 && op.shard_copies >= 0 &&
          op.shard_copies <= 64 && op.h2f_iter >= 0 && op.h2f_iter <= 2 && op.solver >= 0 &&
          op.solver <= 2 && op.pcg_tol >= 0.0 && op.pcg_maxit >= 0 && op.stream_out >= -1 &&
          op.stream_out <= 1 && op.pcg_block_wgs >= 0)) {
        err = "bad dbslmm_options";
        return DBSLMM_E_ARG;
    }
    out = PlanLayout{};
    PlanLayout::Kept& k = out.keep;
    const bool has_l = pr.l_ptr != nullptr;
    const int64_t n_snp_bed = (pr.bed_len - 3) / bed_row_bytes(pr.n_ref);
    k.n_s = pr.s_ptr[pr.num_block];
    k.n_l = has_l ? pr.l_ptr[pr.num_block] : 0;
    k.kpad = round_up(pr.n_ref, gram::kKpadAlign);   // the FP4 Gram's K stage (gram_big: 128 divides it)

    std::vector<int32_t>&slot_pos = out.slot_pos, &slot_block = out.slot_block, &slot_out = k.h_slot_out;
    std::vector<int32_t>&row0 = k.h_row0, &mv = k.h_m, &msv = k.h_ms, &ldv = k.h_ld, &blk_id = k.h_blk_id;
    std::vector<double>& z = out.z;
    std::vector<int64_t>& matoff = k.h_matoff;
    std::vector<GramTile>& tiles = out.tiles;
    const int64_t gram_big_min = op.gram_big_min > 0 ? op.gram_big_min : kGramBigMinDefault;
    // the 256-tile kernel pays once its K loop outweighs its 512 KB fp64 epilogue per tile
    const int64_t gram_huge_min = op.gram_huge_min > 0 ? op.gram_huge_min
                                  : k.kpad >= 4096 ? kGramHugeMinDefault : 2 * kGramHugeMinDefault;
    std::vector<std::vector<GramTile>> xq(kXcd), hq(kXcd), lq(kXcd), nq(kXcd);
    std::vector<double> xload(kXcd, 0.0), hload(kXcd, 0.0), lload(kXcd, 0.0), nload(kXcd, 0.0);
    int64_t moff = 0;
    double ops_alg = 0, ops_exec = 0, chol_flops_large = 0, chol_flops_small = 0, chol_flops_tiled = 0;
    // SNPs per original block (checked for monotone offsets in the block loop below) and the most
    std::vector<int64_t> mb(std::max(0, pr.num_block));
    int64_t mmax = 0;
    for (int b = 0; b < pr.num_block; ++b) {
        mb[b] = pr.s_ptr[b + 1] - pr.s_ptr[b] + (has_l ? pr.l_ptr[b + 1] - pr.l_ptr[b] : 0);
        mmax = std::max(mmax, mb[b]);
    }
    int64_t tiled_min = kTiledMinDefault;
    if (op.tiled_min > 0) {
        tiled_min = std::max<int64_t>(64, op.tiled_min);
    } else if (mmax < 512) {
        // no block reaches the default: the single-workgroup solve of the largest blocks is then
        // the critical path itself, and spreading the blocks of >= kTiledMinSmall SNPs over many
        // workgroups shortens it (config 2: 0.66 -> 0.55 ms/step); with bigger blocks the tiled
        // sequence is the critical path and the mid-size blocks stay in its shadow
        tiled_min = kTiledMinSmall;
    }
    k.tiled_min = static_cast<int32_t>(std::min<int64_t>(tiled_min, INT32_MAX));
    // lead group: the tiled blocks with the longest factorisation chains (m >= lead_min); their
    // Gram tiles form the first 256-tile launch and their sequence starts right after it
    int64_t lead_min = INT64_MAX;
    if (op.lead_min >= 0) {
        // (round 4, config 4 same box, with the substitution grids below: lead >= 1536 on
        // 80 / 176 workgroups 42.02 / 42.11 ms against 42.85-42.97 for max(2048, m_max / 2) on
        // 64 / 192; 1280 42.47, 1792 42.44, 1536 on 64 / 192 43.10, on 72 / 184 42.35,
        // on 96 / 160 43.29 -- profiles/r04/ab/lead_grids.txt)
        lead_min = op.lead_min > 0 ? op.lead_min : std::max<int64_t>(kLeadMinDefault, mmax / 8);
        lead_min = std::max({lead_min, tiled_min, gram_huge_min});
        int64_t n_lead = 0, n_rest = 0;
        for (int64_t m : mb) {
            if (m >= lead_min) ++n_lead;
            else if (m >= tiled_min) ++n_rest;
        }
        if (n_lead == 0 || n_rest == 0) lead_min = INT64_MAX;   // nothing to overlap
    }
    out.gram_big_min = gram_big_min;
    out.gram_huge_min = gram_huge_min;
    out.lead_min = lead_min;
    std::vector<char> is_tiled;
    for (int b = 0; b < pr.num_block; ++b) {
        const int64_t s0 = pr.s_ptr[b], ms = pr.s_ptr[b + 1] - s0;
        const int64_t l0 = has_l ? pr.l_ptr[b] : 0, ml = has_l ? pr.l_ptr[b + 1] - l0 : 0;
        if (ms < 0 || ml < 0) { err = "CSR offsets not monotone"; return DBSLMM_E_ARG; }
        const int64_t m = mb[b];
        if (m == 0) { k.h_empty.push_back(b); continue; }
        const int nb = static_cast<int>(row0.size());
        const bool tiled = m >= tiled_min;
        // packed work items: 128-row tile / region indices in 8 bits, block (x copies) in 15
        if (tiled && (m >= kTiledMaxM || nb >= 32767)) {
            err = "LD block too large for the tiled path (m must be < 32640 SNPs)";
            return DBSLMM_E_ARG;
        }
        is_tiled.push_back(tiled);
        // + the z row of the bordered matrix; the tiled path works on 128 x 128 regions
        const int64_t ld = round_up(m + 1, tiled ? 2 * chol::kBT : kTile);
        row0.push_back(static_cast<int32_t>(slot_pos.size()));
        mv.push_back(static_cast<int32_t>(m));
        msv.push_back(static_cast<int32_t>(ms));
        ldv.push_back(static_cast<int32_t>(ld));
        blk_id.push_back(b);
        matoff.push_back(moff);
        moff += ld * ld;
        for (int64_t i = 0; i < ms; ++i) {
            const int32_t r = pr.s_pos[s0 + i];
            if (r < 0 || r >= n_snp_bed) { err = "small SNP bed row out of range"; return DBSLMM_E_ARG; }
            slot_pos.push_back(r);
            slot_block.push_back(nb);
            slot_out.push_back(static_cast<int32_t>(s0 + i));
            z.push_back(pr.z_s[s0 + i]);
        }
        for (int64_t i = 0; i < ml; ++i) {
            const int32_t r = pr.l_pos[l0 + i];
            if (r < 0 || r >= n_snp_bed) { err = "large SNP bed row out of range"; return DBSLMM_E_ARG; }
            slot_pos.push_back(r);
            slot_block.push_back(nb);
            slot_out.push_back(static_cast<int32_t>(-1 - (l0 + i)));
            z.push_back(pr.z_l[l0 + i]);
        }
        for (int64_t i = m; i < ld; ++i) {
            slot_pos.push_back(-1);
            slot_block.push_back(nb);
            slot_out.push_back(INT32_MIN);
            z.push_back(0.0);
        }
        if (m >= gram_huge_min) {   // 256 x 256 tiles
            const int T = static_cast<int>((m + gram::kHT - 1) / gram::kHT);
            auto& q = m >= lead_min ? lq : tiled ? hq : nq;
            auto& ld_ = m >= lead_min ? lload : tiled ? hload : nload;
            // squares of kGramSq x kGramSq tiles (lower triangle), each on the least-loaded XCD:
            // the workgroups in flight on an XCD share kGramSq row panels of each operand
            for (int si = 0; si < T; si += kGramSq)
                for (int sj = 0; sj <= si; sj += kGramSq) {
                    const int x = static_cast<int>(std::min_element(ld_.begin(), ld_.end()) - ld_.begin());
                    for (int ti = si; ti < std::min(T, si + kGramSq); ++ti)
                        for (int tj = sj; tj < std::min(ti + 1, sj + kGramSq); ++tj) {
                            q[x].push_back({nb, ti, tj, 0});
                            ld_[x] += 1;
                        }
                }
            // MFMA work actually issued (dbslmm_gram_huge): 32 x 32 sub-tiles with rows and
            // columns < m, and on a diagonal tile not strictly above its diagonal
            int64_t sub = 0;
            for (int ti = 0; ti < T; ++ti)
                for (int tj = 0; tj <= ti; ++tj) {
                    const int64_t rv = std::min<int64_t>(gram::kHT, m - int64_t(gram::kHT) * ti);
                    const int64_t cv = std::min<int64_t>(gram::kHT, m - int64_t(gram::kHT) * tj);
                    const int64_t ni = (rv + 31) / 32, nj = (cv + 31) / 32;
                    sub += ti != tj ? ni * nj : ni * (ni + 1) / 2;   // (diagonal: rv == cv)
                }
            ops_exec += 2.0 * k.kpad * 32 * 32 * sub;
        } else if (m >= gram_big_min) {   // 128 x 128 tiles, the block's queue on the least-loaded XCD
            const int T = static_cast<int>((m + gram::kGT - 1) / gram::kGT);
            const int x = static_cast<int>(std::min_element(xload.begin(), xload.end()) - xload.begin());
            for (int ti = 0; ti < T; ++ti)
                for (int tj = 0; tj <= ti; ++tj) xq[x].push_back({nb, ti, tj, 0});
            xload[x] += T * (T + 1) / 2;
            // (dbslmm_gram_big: whole 128 x 128 tiles; a diagonal tile skips its upper quadrant)
            ops_exec += 2.0 * k.kpad * gram::kGT * gram::kGT * (T * (T - 1) / 2 + 0.75 * T);
        } else {
            const int T = static_cast<int>((m + kTile - 1) / kTile);   // tiles holding SNP rows
            for (int ti = 0; ti < T; ++ti)
                for (int tj = 0; tj <= ti; ++tj) tiles.push_back({nb, ti, tj, 0});
            ops_exec += 2.0 * k.kpad * kTile * kTile * (T * (T + 1) / 2);
        }
        ops_alg += static_cast<double>(pr.n_ref) * m * (m + 1);
        (tiled ? chol_flops_tiled : ld > chol::kSmallLd ? chol_flops_large : chol_flops_small) +=
            m * static_cast<double>(m) * m / 3.0 + 2.0 * m * m;
    }
    k.n_nonempty = static_cast<int32_t>(row0.size());
    k.n_slots = static_cast<int32_t>(slot_pos.size());
    for (size_t b = 0; b < mv.size(); ++b) k.has_large = k.has_large || mv[b] > msv[b];
    k.n_tiles = static_cast<int32_t>(tiles.size());
    std::vector<GramTile>& btiles = out.btiles;
    {
        size_t qmax = 0;
        for (const auto& q : xq) qmax = std::max(qmax, q.size());
        btiles.assign(qmax * kXcd, GramTile{-1, 0, 0, 0});
        for (int x = 0; x < kXcd; ++x)
            for (size_t i = 0; i < xq[x].size(); ++i) btiles[i * kXcd + x] = xq[x][i];
        k.n_btiles = static_cast<int32_t>(btiles.size());
    }
    // [lead group's queues | the other tiled blocks' | the non-tiled blocks'], entry e on XCD e % 8
    std::vector<GramTile>& htiles = out.htiles;
    for (const auto* qs : {&lq, &hq, &nq}) {
        size_t qmax = 0;
        for (const auto& q : *qs) qmax = std::max(qmax, q.size());
        const size_t base = htiles.size();
        htiles.resize(base + qmax * kXcd, GramTile{-1, 0, 0, 0});
        for (int x = 0; x < kXcd; ++x)
            for (size_t i = 0; i < (*qs)[x].size(); ++i) htiles[base + i * kXcd + x] = (*qs)[x][i];
        if (qs == &lq) k.n_htiles_lead = static_cast<int32_t>(htiles.size());
        if (qs == &hq) k.n_htiles_tiled = static_cast<int32_t>(htiles.size());
    }
    {
        // (without tiled blocks stream2 runs chol_small, which needs the whole Gram)
        bool all_huge = true, any_tiled = false;
        for (size_t b = 0; b < mv.size(); ++b) {
            any_tiled = any_tiled || is_tiled[b];
            if (is_tiled[b] && mv[b] < gram_huge_min) all_huge = false;
        }
        // (lead_min < 0: no overlap of the Gram and the factorisation at all)
        k.early_fork = all_huge && any_tiled && op.lead_min >= 0;
    }
    k.n_htiles = static_cast<int32_t>(htiles.size());
    k.M_elems = moff;
    (void)build_out_ranges(pr.num_block, pr.s_ptr, has_l ? pr.l_ptr : nullptr, k.h_orange);   // (offsets checked above)
    // Cholesky work lists: large blocks (ld > 64, one workgroup each) then small blocks (one
    // wave each), each largest first (longest-processing-time order)
    std::vector<int32_t>& order = out.order;
    order.resize(k.n_nonempty);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int c) { return mv[a] > mv[c]; });
    order.erase(std::remove_if(order.begin(), order.end(), [&](int b) { return is_tiled[b] != 0; }),
                order.end());
    int32_t large_ld_max = 0;
    for (int32_t b : order) {
        (ldv[b] > chol::kSmallLd ? k.n_large : k.n_small)++;
        if (ldv[b] > chol::kSmallLd) large_ld_max = std::max(large_ld_max, ldv[b]);
    }
    // dbslmm_chol_cheb holds a block's vectors in LDS for ld <= kChebMaxM (the default tiled_min
    // guarantees it; a larger tiled_min leaves bigger blocks on chol_large, whose h2f copies are
    // then all factored)
    k.large_cheb_ok = op.large_cheb == 0 && large_ld_max <= chol::kChebMaxM;
    {
        std::vector<int32_t> tb_lead, tb_rest;
        for (int b = 0; b < k.n_nonempty; ++b)
            if (is_tiled[b]) {
                k.h_tb.push_back(b);
                (mv[b] >= lead_min ? tb_lead : tb_rest).push_back(b);
            }
        k.n_tiled = static_cast<int32_t>(k.h_tb.size());
        if (tb_lead.empty()) {
            build_tiled(mv, k.h_tb, 1, k.n_nonempty, k.tl, out.tlist);
        } else {
            build_tiled(mv, tb_lead, 1, k.n_nonempty, k.tl, out.tlist);
            build_tiled(mv, tb_rest, 1, k.n_nonempty, k.tl_rest, out.tlist);
        }
    }
    // substitution work lists (trsv.hip): 64-row tiles of the tiled blocks; forward in order of
    // (tile, block), backward in order of (tiles from the end, block) -- every dependency of an
    // item comes earlier in its list
    std::vector<int32_t>&tri_f = out.tri_f, &tri_b = out.tri_b, &foff = out.foff;
    foff.assign(std::max(1, k.n_nonempty), 0);
    {
        auto sub_tiles = [&](int32_t b) { return (mv[b] + trsv::kT - 1) / trsv::kT; };
        int32_t nf = 0;
        int tmx = 1;
        for (int32_t b : k.h_tb) {
            foff[b] = nf;
            nf += sub_tiles(b);
            tmx = std::max(tmx, sub_tiles(b));
        }
        k.n_tflags = nf;
        // ticket order: tile position relative to the block's length minus alpha T / Tmax (bigger
        // blocks' tiles are claimed earlier: their chains are longer; ties: longer block first),
        // monotone in the position within each block, so every dependency comes earlier.  Split
        // substitutions (sub_split): the lead group's items first, then the rest group's, each
        // group in that order (and d_tb = [lead blocks | rest blocks])
        // (config 4, same box: one sequence 45.1-45.5 ms per step; split on 64 / 192 workgroups
        // 43.9-44.1; 96 / 160 44.9; 128 / 128 47.1; a rest grid of every CU 51-56 -- its
        // persistent workgroups then hold the CUs the lead factorisation's tail still needs)
        // (cheb_fused = 1 runs every Chebyshev pass of ALL tiled items in one launch: no groups)
        k.sub_split = op.sub_split >= 0 && !k.tl_rest.empty() && op.cheb_fused != 1;
        // lead workgroups by the lead group's share f of the factor bytes a pass streams:
        // 2.05 f^1.5 of the CUs, within [1/16, 1/2]: config 4's f = 0.285 gives the 80 of 256 tuned
        // there in round 4; a shard whose lead group is small (the bulk device of the 8-GPU plan,
        // f = 0.135: 26) gives its rest group the CUs instead of leaving 5/16 of the chip to a few
        // short chains (that device 19.4 ms at 80 lead workgroups, 17.1 at 24 / 32, 18.3 at 16)
        double lb = 0.0, ab = 0.0;   // tiles of the factor: the lead group's, all
        for (int32_t b : k.h_tb) {
            const double T = sub_tiles(b), by = T * (T + 1) / 2;
            ab += by;
            if (mv[b] >= lead_min) lb += by;
        }
        {
            const double share = ab > 0 ? lb / ab : 0.0;
            const int g = static_cast<int>(std::lround(n_cu * 2.05 * share * std::sqrt(share)));
            k.sub_grid_lead = op.sub_grid_lead > 0 ? op.sub_grid_lead
                                                   : std::clamp(g, std::max(1, n_cu / 16), std::max(1, n_cu / 2));
        }
        k.sub_grid_rest = op.sub_grid_rest > 0 ? op.sub_grid_rest : std::max(1, n_cu - k.sub_grid_lead);
        auto grp_of = [&](int32_t b) { return k.sub_split && mv[b] < lead_min ? 1 : 0; };
        struct It { int grp; double key; int T; int32_t b, I; };
        std::vector<It> v;
        constexpr double alpha = 0.25;
        for (int32_t b : k.h_tb) {
            const int T = sub_tiles(b);
            for (int I = 0; I < T; ++I) v.push_back({grp_of(b), static_cast<double>(I) / T - alpha * T / tmx, T, b, I});
        }
        std::stable_sort(v.begin(), v.end(), [&](const It& x, const It& y) {
            return x.grp != y.grp ? x.grp < y.grp : x.key != y.key ? x.key < y.key : x.T > y.T;
        });
        k.n_titems_lead = static_cast<int32_t>(std::count_if(v.begin(), v.end(), [](const It& x) { return x.grp == 0; }));
        if (k.sub_split) {
            std::stable_partition(k.h_tb.begin(), k.h_tb.end(), [&](int32_t b) { return grp_of(b) == 0; });
            k.n_tb_lead = static_cast<int32_t>(std::count_if(k.h_tb.begin(), k.h_tb.end(),
                                                             [&](int32_t b) { return grp_of(b) == 0; }));
        }
        // whole-block Chebyshev passes for the rest group (sub_split = 2): every rest block within
        // kTChebMaxM (the work vector of NR copies in LDS; one workgroup streams the block alone)
        if (k.sub_split && op.sub_split == 2) {
            std::vector<int32_t> rb(k.h_tb.begin() + k.n_tb_lead, k.h_tb.end());
            int32_t tmax_r = 0;
            for (int32_t b : rb) tmax_r = std::max(tmax_r, sub_tiles(b));
            if (!rb.empty() && tmax_r * trsv::kT <= kTChebMaxM) {
                std::stable_sort(rb.begin(), rb.end(), [&](int32_t x, int32_t y) { return mv[x] > mv[y]; });
                out.tcheb_list = rb;
                k.sub_block = true;
                k.n_tcheb = static_cast<int32_t>(rb.size());
                k.tcheb_vld = tmax_r * trsv::kT;
            }
        }
        for (const It& x : v) {
            tri_f.push_back(x.b);
            tri_f.push_back(x.I);
            tri_b.push_back(x.b);
            tri_b.push_back(x.T - 1 - x.I);   // backward: the same order from the other end
        }
        k.n_titems = static_cast<int32_t>(tri_f.size() / 2);
        // factor bytes one substitution launch reads: T (T + 1) / 2 tiles per block
        k.wl[13] = ab * trsv::kT * trsv::kT * sizeof(double);
    }
    const double n_snp = static_cast<double>(k.n_s + k.n_l);
    k.wl[0] = n_snp;
    // bytes the statistics gather reads per slot: its image row, the row's table entry, its block
    k.wl[1] = static_cast<double>(k.n_slots) * (sizeof(int32_t) + kRowEntryBytes + sizeof(int32_t));
    // bytes it writes: S, mu, 1/sd per slot and the blocks' missing-call flags
    k.wl[2] = static_cast<double>(k.n_slots) * 3 * sizeof(double) + static_cast<double>(k.n_nonempty) * sizeof(int32_t);
    k.wl[3] = ops_alg;
    k.wl[4] = ops_exec;
    k.wl[5] = chol_flops_large;
    k.wl[6] = k.n_nonempty;
    k.wl[7] = k.n_tiles + k.n_btiles + k.n_htiles;
    k.wl[8] = chol_flops_small;
    k.wl[9] = k.n_large;
    k.wl[10] = chol_flops_tiled;
    k.wl[11] = k.n_tiled;
    auto is_launch = [](const TLaunch& L) { return L.kind < kTlRecord; };
    k.wl[12] = static_cast<double>(std::count_if(k.tl.begin(), k.tl.end(), is_launch) +
                                   std::count_if(k.tl_rest.begin(), k.tl_rest.end(), is_launch));
    k.wl[14] = 0;
    k.wl[15] = -1;
    return DBSLMM_OK;
}
