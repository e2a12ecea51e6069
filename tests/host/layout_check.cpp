// layout_check.cpp -- a stand-alone check of the plan's host layout (plan_layout.hpp): no HIP, no
// library of the project.  Built with the host sanitizers by `make -C dbslmm_amd/csrc sanitize`
// (../bin/layout_asan) and run by tests/test_sanitizers.py; also `g++ -std=c++17 layout_check.cpp`.
//
// For every problem and option set below the layout is built and its lists are checked against
// what the kernels need of them, worked out here independently: slot arithmetic, exact tile
// coverage of the three Gram lists, the Cholesky work order, a replay of the tiled launch lists
// (each region, panel item and trailing tile exactly once, after what it depends on -- across the
// sequence's two streams by the events the list itself records and waits for) and the order of
// the substitution tickets.  The first violation prints a message and exits 1.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "../../dbslmm_amd/csrc/plan_layout.hpp"

namespace {

std::string g_case;
[[noreturn]] void fail(const std::string& what) {
    fprintf(stderr, "layout_check: %s: %s\n", g_case.c_str(), what.c_str());
    exit(1);
}
#define CHECK(cond, ...)                                       \
    do {                                                       \
        if (!(cond)) {                                         \
            char msg_[512];                                    \
            snprintf(msg_, sizeof msg_, __VA_ARGS__);          \
            fail(std::string(#cond) + " -- " + msg_);         \
        }                                                      \
    } while (0)

int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// A problem of the given block sizes: block b's first `m - m / 3` SNPs small and the rest large
// (all small without large SNPs), bed rows in a scrambled order, any z.  The layout never reads the
// genotype bytes, so bed stays a non-null pointer that is never dereferenced.
struct Problem {
    std::vector<int64_t> s_ptr{0}, l_ptr{0};
    std::vector<int32_t> s_pos, l_pos;
    std::vector<double> z_s, z_l;
    dbslmm_problem pr{};
    dbslmm_options op{};
    Problem(const std::vector<int>& ms, bool has_l, int32_t n_ref) {
        int64_t total = 0;
        for (int m : ms) total += m;
        int64_t row = 0;
        for (int m : ms) {
            const int ml = has_l ? m / 3 : 0;
            for (int i = 0; i < m; ++i, ++row) {
                const int32_t r = static_cast<int32_t>((row * 7919) % std::max<int64_t>(1, total));   // a permutation
                (i < m - ml ? s_pos : l_pos).push_back(r);
                (i < m - ml ? z_s : z_l).push_back(0.25 * static_cast<double>(row % 17) - 2.0);
            }
            s_ptr.push_back(static_cast<int64_t>(s_pos.size()));
            l_ptr.push_back(static_cast<int64_t>(l_pos.size()));
        }
        static const uint8_t never_read = 0;
        pr.bed = &never_read;
        pr.n_ref = n_ref;
        pr.bed_len = 3 + bed_row_bytes(n_ref) * std::max<int64_t>(1, total);
        pr.n_obs = 10000;
        pr.sigma_s = 1e-4;
        pr.tau = 0.8;
        pr.num_block = static_cast<int32_t>(ms.size());
        // (data() of an empty vector may be null; the layout reads no element then)
        pr.s_ptr = s_ptr.data();
        pr.s_pos = s_pos.data();
        pr.z_s = z_s.data();
        pr.l_ptr = has_l ? l_ptr.data() : nullptr;
        pr.l_pos = has_l ? l_pos.data() : nullptr;
        pr.z_l = has_l ? z_l.data() : nullptr;
        pr.opts = &op;
    }
    int64_t m(int b) const { return s_ptr[b + 1] - s_ptr[b] + l_ptr[b + 1] - l_ptr[b]; }
};

// the thresholds the options select, by the rules of dbslmm_options (include/dbslmm_hip.h)
struct Thresholds { int64_t tiled_min, big_min, huge_min, lead_min; };
Thresholds thresholds(const Problem& P) {
    const dbslmm_options& op = P.op;
    int64_t mmax = 0;
    for (int b = 0; b < P.pr.num_block; ++b) mmax = std::max(mmax, P.m(b));
    Thresholds t;
    t.tiled_min = op.tiled_min > 0 ? std::max(64, op.tiled_min) : mmax < 512 ? kTiledMinSmall : kTiledMinDefault;
    t.big_min = op.gram_big_min > 0 ? op.gram_big_min : kGramBigMinDefault;
    const int64_t kpad = ceil_div(P.pr.n_ref, 256) * 256;
    t.huge_min = op.gram_huge_min > 0 ? op.gram_huge_min : kpad >= 4096 ? kGramHugeMinDefault : 2 * kGramHugeMinDefault;
    t.lead_min = INT64_MAX;
    if (op.lead_min >= 0) {
        const int64_t base = op.lead_min > 0 ? op.lead_min : std::max<int64_t>(kLeadMinDefault, mmax / 8);
        const int64_t lm = std::max({base, t.tiled_min, t.huge_min});
        bool any_lead = false, any_rest = false;
        for (int b = 0; b < P.pr.num_block; ++b) {
            any_lead = any_lead || P.m(b) >= lm;
            any_rest = any_rest || (P.m(b) < lm && P.m(b) >= t.tiled_min);
        }
        if (any_lead && any_rest) t.lead_min = lm;   // a lead group needs something to overlap with
    }
    return t;
}

void check_slots(const Problem& P, const PlanLayout& L, const Thresholds& t) {
    const PlanLayout::Kept& k = L.keep;
    int nb = 0;
    int64_t row = 0, moff = 0;
    std::vector<int32_t> empty;
    bool has_large = false;
    for (int b = 0; b < P.pr.num_block; ++b) {
        const int64_t m = P.m(b), ms = P.s_ptr[b + 1] - P.s_ptr[b], ml = m - ms;
        if (m == 0) { empty.push_back(b); continue; }
        CHECK(nb < static_cast<int>(k.h_m.size()), "block %d missing", b);
        const int64_t ld = ceil_div(m + 1, m >= t.tiled_min ? 128 : 32) * (m >= t.tiled_min ? 128 : 32);
        CHECK(k.h_m[nb] == m && k.h_ms[nb] == ms && k.h_blk_id[nb] == b, "block %d: m %d ms %d id %d", b, k.h_m[nb], k.h_ms[nb], k.h_blk_id[nb]);
        CHECK(k.h_ld[nb] == ld, "block %d (m %lld): ld %d, expected %lld", b, (long long)m, k.h_ld[nb], (long long)ld);
        CHECK(k.h_row0[nb] == row && k.h_matoff[nb] == moff, "block %d: row0 %d matoff %lld", b, k.h_row0[nb], (long long)k.h_matoff[nb]);
        CHECK(static_cast<int64_t>(L.slot_pos.size()) >= row + ld, "slots of block %d missing", b);
        for (int64_t i = 0; i < ld; ++i) {
            const int64_t s = row + i;
            CHECK(L.slot_block[s] == nb, "slot %lld: block %d", (long long)s, L.slot_block[s]);
            const int32_t pos = i < ms ? P.s_pos[P.s_ptr[b] + i] : i < m ? P.l_pos[P.l_ptr[b] + i - ms] : -1;
            const int64_t out = i < ms ? P.s_ptr[b] + i : i < m ? -1 - (P.l_ptr[b] + i - ms) : INT32_MIN;
            const double z = i < ms ? P.z_s[P.s_ptr[b] + i] : i < m ? P.z_l[P.l_ptr[b] + i - ms] : 0.0;
            CHECK(L.slot_pos[s] == pos && k.h_slot_out[s] == out && L.z[s] == z, "slot %lld of block %d: pos %d out %d",
                  (long long)s, b, L.slot_pos[s], k.h_slot_out[s]);
        }
        has_large = has_large || ml > 0;
        row += ld;
        moff += ld * ld;
        ++nb;
    }
    CHECK(k.n_nonempty == nb && static_cast<int>(k.h_m.size()) == nb && k.h_ld.size() == k.h_m.size() &&
          k.h_ms.size() == k.h_m.size() && k.h_row0.size() == k.h_m.size() && k.h_matoff.size() == k.h_m.size() &&
          k.h_blk_id.size() == k.h_m.size(), "n_nonempty %d, expected %d", k.n_nonempty, nb);
    CHECK(k.n_slots == row && static_cast<int64_t>(L.slot_pos.size()) == row && L.slot_block.size() == L.slot_pos.size() &&
          k.h_slot_out.size() == L.slot_pos.size() && L.z.size() == L.slot_pos.size(), "n_slots %d, expected %lld", k.n_slots, (long long)row);
    CHECK(k.M_elems == moff, "M_elems %lld, expected %lld", (long long)k.M_elems, (long long)moff);
    CHECK(k.h_empty == empty, "h_empty has %zu entries, expected %zu", k.h_empty.size(), empty.size());
    CHECK(k.has_large == has_large, "has_large %d", k.has_large);
    CHECK(k.n_s == P.s_ptr.back() && k.n_l == (P.pr.l_ptr ? P.l_ptr.back() : 0), "n_s %lld n_l %lld", (long long)k.n_s, (long long)k.n_l);
    // slot_out: a bijection onto {0 .. n_s - 1} u {-1 .. -n_l}, INT32_MIN on exactly the pads
    std::vector<char> seen_s(k.n_s, 0), seen_l(k.n_l, 0);
    for (size_t s = 0; s < k.h_slot_out.size(); ++s) {
        const int32_t o = k.h_slot_out[s];
        CHECK((o == INT32_MIN) == (L.slot_pos[s] == -1), "slot %zu: out %d, pos %d", s, o, L.slot_pos[s]);
        if (o == INT32_MIN) continue;
        CHECK(o >= 0 ? o < k.n_s : -1 - o < k.n_l, "slot %zu: out %d out of range", s, o);
        char& mark = o >= 0 ? seen_s[o] : seen_l[-1 - o];
        CHECK(!mark, "slot %zu: out %d twice", s, o);
        mark = 1;
    }
    CHECK(std::count(seen_s.begin(), seen_s.end(), 1) == k.n_s && std::count(seen_l.begin(), seen_l.end(), 1) == k.n_l,
          "slot_out misses an output");
    CHECK(k.h_orange.size() == k.h_m.size(), "h_orange: %zu ranges", k.h_orange.size());
}

// tiles [t0, t1) of `list` hold, once each, every lower-triangle tile of edge `edge` of exactly the
// blocks `want` selects, and fillers (block -1) only where `fillers`
template <typename Want>
void check_tile_list(const PlanLayout::Kept& k, const std::vector<GramTile>& list, size_t t0, size_t t1, int edge,
                     bool fillers, const char* name, Want want) {
    CHECK(t0 <= t1 && t1 <= list.size(), "%s: range %zu .. %zu of %zu", name, t0, t1, list.size());
    std::set<std::tuple<int, int, int>> seen;
    for (size_t e = t0; e < t1; ++e) {
        const GramTile& g = list[e];
        if (g.block == -1) {
            CHECK(fillers, "%s[%zu]: a filler", name, e);
            continue;
        }
        CHECK(g.block >= 0 && g.block < k.n_nonempty && want(g.block), "%s[%zu]: block %d does not belong here", name, e, g.block);
        const int T = static_cast<int>(ceil_div(k.h_m[g.block], edge));
        CHECK(g.tj >= 0 && g.tj <= g.ti && g.ti < T, "%s[%zu]: tile (%d, %d) of block %d (%d tile rows)", name, e, g.ti, g.tj, g.block, T);
        CHECK(seen.insert({g.block, g.ti, g.tj}).second, "%s[%zu]: tile (%d, %d) of block %d twice", name, e, g.ti, g.tj, g.block);
    }
    size_t expected = 0;
    for (int b = 0; b < k.n_nonempty; ++b)
        if (want(b)) {
            const size_t T = static_cast<size_t>(ceil_div(k.h_m[b], edge));
            expected += T * (T + 1) / 2;
        }
    CHECK(seen.size() == expected, "%s: %zu tiles, expected %zu", name, seen.size(), expected);
}

void check_gram(const Problem& P, const PlanLayout& L, const Thresholds& t) {
    const PlanLayout::Kept& k = L.keep;
    CHECK(L.gram_big_min == t.big_min && L.gram_huge_min == t.huge_min && L.lead_min == t.lead_min && k.tiled_min == t.tiled_min,
          "thresholds: big %lld huge %lld lead %lld tiled %d", (long long)L.gram_big_min, (long long)L.gram_huge_min,
          (long long)L.lead_min, k.tiled_min);
    auto m = [&](int b) { return static_cast<int64_t>(k.h_m[b]); };
    CHECK(k.n_tiles == static_cast<int>(L.tiles.size()) && k.n_btiles == static_cast<int>(L.btiles.size()) &&
          k.n_htiles == static_cast<int>(L.htiles.size()), "tile counts %d %d %d", k.n_tiles, k.n_btiles, k.n_htiles);
    CHECK(0 <= k.n_htiles_lead && k.n_htiles_lead <= k.n_htiles_tiled && k.n_htiles_tiled <= k.n_htiles,
          "htiles segments %d %d %d", k.n_htiles_lead, k.n_htiles_tiled, k.n_htiles);
    CHECK(k.n_btiles % 8 == 0 && k.n_htiles_lead % 8 == 0 && (k.n_htiles_tiled - k.n_htiles_lead) % 8 == 0 &&
          (k.n_htiles - k.n_htiles_tiled) % 8 == 0, "per-XCD queues: lengths %d %d %d %d", k.n_btiles, k.n_htiles_lead,
          k.n_htiles_tiled, k.n_htiles);
    check_tile_list(k, L.tiles, 0, L.tiles.size(), 32, false, "tiles", [&](int b) { return m(b) < t.big_min && m(b) < t.huge_min; });
    check_tile_list(k, L.btiles, 0, L.btiles.size(), 128, true, "btiles", [&](int b) { return m(b) >= t.big_min && m(b) < t.huge_min; });
    check_tile_list(k, L.htiles, 0, k.n_htiles_lead, 256, true, "htiles (lead)", [&](int b) { return m(b) >= t.huge_min && m(b) >= t.lead_min; });
    check_tile_list(k, L.htiles, k.n_htiles_lead, k.n_htiles_tiled, 256, true, "htiles (tiled)",
                    [&](int b) { return m(b) >= t.huge_min && m(b) < t.lead_min && m(b) >= t.tiled_min; });
    check_tile_list(k, L.htiles, k.n_htiles_tiled, k.n_htiles, 256, true, "htiles (rest)",
                    [&](int b) { return m(b) >= t.huge_min && m(b) < t.tiled_min; });
    // early_fork: the tiled sequences may start before the non-tiled blocks' Gram exactly when the
    // 256-tile segments in front of it hold every tiled block's Gram (and the overlap is not off)
    bool any_tiled = false, all_huge = true;
    for (int b = 0; b < k.n_nonempty; ++b)
        if (m(b) >= t.tiled_min) { any_tiled = true; all_huge = all_huge && m(b) >= t.huge_min; }
    CHECK(k.early_fork == (any_tiled && all_huge && P.op.lead_min >= 0), "early_fork %d", k.early_fork);
}

void check_order(const Problem& P, const PlanLayout& L, const Thresholds& t) {
    const PlanLayout::Kept& k = L.keep;
    std::vector<char> seen(k.n_nonempty, 0);
    int n_tiled = 0, ld_max = 0;
    for (int b = 0; b < k.n_nonempty; ++b) n_tiled += k.h_m[b] >= t.tiled_min;
    CHECK(k.n_tiled == n_tiled && k.n_large + k.n_small + k.n_tiled == k.n_nonempty &&
          static_cast<int>(L.order.size()) == k.n_large + k.n_small, "n_large %d n_small %d n_tiled %d of %d, order %zu",
          k.n_large, k.n_small, k.n_tiled, k.n_nonempty, L.order.size());
    for (size_t i = 0; i < L.order.size(); ++i) {
        const int32_t b = L.order[i];
        CHECK(b >= 0 && b < k.n_nonempty && !seen[b] && k.h_m[b] < t.tiled_min, "order[%zu] = %d", i, b);
        seen[b] = 1;
        const bool large = static_cast<int>(i) < k.n_large;
        CHECK(large ? k.h_ld[b] > 64 : k.h_ld[b] <= 64, "order[%zu]: block %d of ld %d in the %s part", i, b, k.h_ld[b], large ? "large" : "small");
        if (i > 0 && static_cast<int>(i) != k.n_large)
            CHECK(k.h_m[L.order[i - 1]] >= k.h_m[b], "order[%zu]: m %d after m %d", i, k.h_m[b], k.h_m[L.order[i - 1]]);
        if (large) ld_max = std::max(ld_max, k.h_ld[b]);
    }
    CHECK(k.large_cheb_ok == (P.op.large_cheb == 0 && ld_max <= 512), "large_cheb_ok %d (largest ld %d)", k.large_cheb_ok, ld_max);
}

// Replay of one tiled launch list over the blocks tb x copies.  Positions in the list are the time
// axis: launches of one stream run in list order; a launch of stream s runs after launch y of the
// other stream only if s has waited for an event the other stream recorded at or behind y.
void check_tiled(const std::vector<int32_t>& mv, const std::vector<int32_t>& tb, int copies, int nb,
                 const std::vector<TLaunch>& tl, const std::vector<int32_t>& tlist, const char* name) {
    struct At { int strm = -1, idx = -1; };
    struct Blk {
        int m = 0, Tz64 = 0, nr = 0, Tz2 = 0, R = 0;
        int next_region = 0;
        std::vector<int> region_at;            // [r] list position
        std::vector<int> panel_at;             // [r * (Tz64 + 1) + i]
        std::vector<At> writer;                // [i * nr + J]: last launch that wrote 64-row tile i of column region J
        std::vector<int> next_step;            // [I * nr + J]: super steps whose trailing update the 128-tile has had
    };
    std::map<int, Blk> blk;
    for (int c = 0; c < copies; ++c)
        for (int32_t b : tb) {
            Blk k;
            k.m = mv[b];
            k.Tz64 = k.m / 64;                               // 64-row tiles 0 .. Tz64 (the last holds the z row m)
            k.nr = static_cast<int>(ceil_div(k.m, 128));     // regions: 128-column groups of the m SNP columns
            k.Tz2 = k.m / 128;
            k.R = k.m >= kWideMin ? kWideSuper : kSuper;
            CHECK(k.Tz2 < 256 && k.nr <= 256, "%s: block %d of m %d: tile indices past 8 bits", name, b, k.m);
            k.region_at.assign(k.nr, -1);
            k.panel_at.assign(static_cast<size_t>(k.nr) * (k.Tz64 + 1), -1);
            k.writer.assign(static_cast<size_t>(k.Tz64 + 1) * k.nr, At{});
            k.next_step.assign(static_cast<size_t>(k.Tz2 + 1) * k.nr, 0);
            const int bq = b + c * nb;
            CHECK(bq < 32768, "%s: block id %d past 15 bits", name, bq);
            blk[bq] = std::move(k);
        }
    int seen[2] = {-1, -1};   // [s]: the latest position of the other stream that stream s is known to run after
    std::map<int, At> events;
    for (int ix = 0; ix < static_cast<int>(tl.size()); ++ix) {
        const TLaunch& L = tl[ix];
        const int s = L.strm;
        CHECK(s == 0 || s == 1, "%s[%d]: stream %d", name, ix, s);
        auto after = [&](const At& y) { return y.idx < 0 || (y.strm == s ? y.idx < ix : seen[s] >= y.idx); };
        auto after_chain = [&](int idx) { return idx >= 0 && after(At{0, idx}); };   // regions and panels: chain stream
        if (L.kind == kTlRecord) {
            events[L.step] = At{s, ix};
            continue;
        }
        if (L.kind == kTlWait) {
            const auto e = events.find(L.step);
            CHECK(e != events.end() && e->second.strm != s, "%s[%d]: waits for event %d, which the other stream has not recorded before",
                  name, ix, L.step);
            seen[s] = std::max(seen[s], e->second.idx);
            continue;
        }
        CHECK(L.kind == 1 || L.kind == 4 || L.kind == 5, "%s[%d]: kind %d", name, ix, L.kind);
        CHECK(L.off >= 0 && L.items > 0 && L.n > 0 && static_cast<size_t>(L.off) + 2 * static_cast<size_t>(L.items) <= tlist.size(),
              "%s[%d]: off %d n %d items %d of %zu", name, ix, L.off, L.n, L.items, tlist.size());
        CHECK(L.kind == 5 ? L.items % 8 == 0 : (L.n == L.items && s == 0), "%s[%d]: kind %d n %d items %d stream %d", name, ix,
              L.kind, L.n, L.items, s);
        for (int e = 0; e < L.items; ++e) {
            const int32_t it = tlist[L.off + 2 * e], meta = tlist[L.off + 2 * e + 1];
            if (L.kind == 5 && it < 0) {
                CHECK(it == -1 && meta == 0, "%s[%d] item %d: filler (%d, %d)", name, ix, e, it, meta);
                continue;
            }
            CHECK(it >= 0 && meta >= 0, "%s[%d] item %d: (%d, %d) negative: a field past its width", name, ix, e, it, meta);
            const int bq = L.kind == 4 ? it : it >> 16;
            const auto f = blk.find(bq);
            CHECK(f != blk.end(), "%s[%d] item %d: block id %d is not in the sequence", name, ix, e, bq);
            Blk& k = f->second;
            const int r = meta >> 8, cnt = meta & 255;   // local step < 2^23 (meta >= 0); pending panels or K multiple
            if (L.kind == 4) {   // region r, with the pending update of the panels of regions r - cnt .. r - 1
                CHECK(r == k.next_region && r < k.nr, "%s[%d]: region %d of block %d, expected region %d of %d", name, ix, r, bq, k.next_region, k.nr);
                CHECK(cnt == r % k.R, "%s[%d]: region %d of block %d with %d pending panels", name, ix, r, bq, cnt);
                k.next_region++;
                k.region_at[r] = ix;
                CHECK(k.next_step[static_cast<size_t>(r) * k.nr + r] == r / k.R, "%s[%d]: region %d of block %d has had %d trailing updates",
                      name, ix, r, bq, k.next_step[static_cast<size_t>(r) * k.nr + r]);
                for (int i = 2 * r; i <= std::min(2 * r + 1, k.Tz64); ++i) {
                    At& w = k.writer[static_cast<size_t>(i) * k.nr + r];
                    CHECK(after(w), "%s[%d]: region %d of block %d may start before launch %d has updated it", name, ix, r, bq, w.idx);
                    for (int q = r - cnt; q < r; ++q)
                        CHECK(after_chain(k.panel_at[static_cast<size_t>(q) * (k.Tz64 + 1) + i]), "%s[%d]: region %d of block %d before panel (%d, %d)",
                              name, ix, r, bq, i, q);
                    w = At{s, ix};
                }
            } else if (L.kind == 1) {   // panel item: 64-row tile i below region r
                const int i = it & 0xFFFF;
                CHECK(r < k.nr && 2 * r + 2 <= i && i <= k.Tz64, "%s[%d]: panel (%d, %d) of block %d (m %d)", name, ix, i, r, bq, k.m);
                CHECK(cnt == r % k.R, "%s[%d]: panel (%d, %d) of block %d with %d pending panels", name, ix, i, r, bq, cnt);
                int& at = k.panel_at[static_cast<size_t>(r) * (k.Tz64 + 1) + i];
                CHECK(at < 0, "%s[%d]: panel (%d, %d) of block %d twice", name, ix, i, r, bq);
                CHECK(k.region_at[r] >= 0 && k.region_at[r] < ix, "%s[%d]: panel (%d, %d) of block %d before its region", name, ix, i, r, bq);
                CHECK(k.next_step[static_cast<size_t>(i / 2) * k.nr + r] == r / k.R, "%s[%d]: panel (%d, %d) of block %d has had %d trailing updates",
                      name, ix, i, r, bq, k.next_step[static_cast<size_t>(i / 2) * k.nr + r]);
                At& w = k.writer[static_cast<size_t>(i) * k.nr + r];
                CHECK(after(w), "%s[%d]: panel (%d, %d) of block %d may start before launch %d has updated it", name, ix, i, r, bq, w.idx);
                for (int q = r - cnt; q < r; ++q)
                    CHECK(after_chain(k.panel_at[static_cast<size_t>(q) * (k.Tz64 + 1) + i]), "%s[%d]: panel (%d, %d) of block %d before panel (%d, %d)",
                          name, ix, i, r, bq, i, q);
                at = ix;
                w = At{s, ix};
            } else {   // trailing: tiles (I, J0 ..) of one run, K = the cnt regions of super step r / R
                const int I = (it >> 8) & 255, J0 = it & 255;
                const int rl = std::min(r + k.R, k.nr) - 1;
                CHECK(r % k.R == 0 && r < k.nr && cnt == rl - r + 1 && rl + 1 < k.nr, "%s[%d]: trailing of block %d at region %d, K of %d regions",
                      name, ix, bq, r, cnt);
                const int J1 = std::min(J0 + L.n - 1, std::min(I, k.nr - 1));   // (the kernel's clipping of a run)
                CHECK(I <= k.Tz2 && J0 > rl && J0 <= J1, "%s[%d]: trailing tile (%d, %d) of block %d at region %d (m %d)", name, ix, I, J0, bq, r, k.m);
                for (int J = J0; J <= J1; ++J) {
                    int& st = k.next_step[static_cast<size_t>(I) * k.nr + J];
                    CHECK(st == r / k.R, "%s[%d]: trailing tile (%d, %d) of block %d: update of super step %d, expected %d", name, ix, I, J, bq,
                          r / k.R, st);
                    ++st;
                    for (int i : {2 * I, 2 * I + 1, 2 * J, 2 * J + 1}) {
                        if (i > k.Tz64) continue;
                        for (int q = r; q <= rl; ++q)
                            CHECK(after_chain(k.panel_at[static_cast<size_t>(q) * (k.Tz64 + 1) + i]),
                                  "%s[%d]: trailing tile (%d, %d) of block %d may start before panel (%d, %d)", name, ix, I, J, bq, i, q);
                    }
                    for (int i = 2 * I; i <= std::min(2 * I + 1, k.Tz64); ++i) {
                        At& w = k.writer[static_cast<size_t>(i) * k.nr + J];
                        CHECK(after(w), "%s[%d]: trailing tile (%d, %d) of block %d may start before launch %d has written it", name, ix, I, J,
                              bq, w.idx);
                        w = At{s, ix};
                    }
                }
            }
        }
    }
    for (const auto& kv : blk) {
        const Blk& k = kv.second;
        CHECK(k.next_region == k.nr, "%s: block %d: %d of %d regions", name, kv.first, k.next_region, k.nr);
        for (int r = 0; r < k.nr; ++r)
            for (int i = 2 * r + 2; i <= k.Tz64; ++i)
                CHECK(k.panel_at[static_cast<size_t>(r) * (k.Tz64 + 1) + i] >= 0, "%s: block %d: panel (%d, %d) never issued", name, kv.first, i, r);
        // every 128-tile (I, J <= I) right of a super step has had that step's update: J / R of them
        for (int I = 0; I <= k.Tz2; ++I)
            for (int J = 0; J <= std::min(I, k.nr - 1); ++J)
                CHECK(k.next_step[static_cast<size_t>(I) * k.nr + J] == J / k.R, "%s: block %d: tile (%d, %d) had %d trailing updates, needs %d",
                      name, kv.first, I, J, k.next_step[static_cast<size_t>(I) * k.nr + J], J / k.R);
    }
}

void check_subst(const Problem& P, const PlanLayout& L, const Thresholds& t, int n_cu) {
    const PlanLayout::Kept& k = L.keep;
    auto T = [&](int b) { return static_cast<int>(ceil_div(k.h_m[b], 64)); };
    auto is_lead = [&](int b) { return k.h_m[b] >= t.lead_min; };
    std::vector<int32_t> tiled;
    int64_t n_items = 0, n_lead_items = 0, n_lead = 0;
    for (int b = 0; b < k.n_nonempty; ++b)
        if (k.h_m[b] >= t.tiled_min) {
            tiled.push_back(b);
            CHECK(L.foff[b] == n_items, "foff[%d] = %d, expected %lld", b, L.foff[b], (long long)n_items);
            n_items += T(b);
            if (is_lead(b)) { n_lead_items += T(b); ++n_lead; }
        }
    const bool split = P.op.sub_split >= 0 && t.lead_min != INT64_MAX && P.op.cheb_fused != 1;
    CHECK(k.sub_split == split, "sub_split %d, expected %d", k.sub_split, split);
    CHECK((t.lead_min != INT64_MAX) == !k.tl_rest.empty(), "tl_rest has %zu entries, lead_min %lld", k.tl_rest.size(), (long long)t.lead_min);
    CHECK(k.n_tflags == n_items && k.n_titems == n_items && L.tri_f.size() == 2 * static_cast<size_t>(n_items) &&
          L.tri_b.size() == L.tri_f.size() && static_cast<int>(L.foff.size()) == std::max(1, k.n_nonempty),
          "n_tflags %d n_titems %d, expected %lld", k.n_tflags, k.n_titems, (long long)n_items);
    CHECK(k.n_titems_lead == (split ? n_lead_items : n_items) && k.n_tb_lead == (split ? n_lead : 0),
          "n_titems_lead %d n_tb_lead %d", k.n_titems_lead, k.n_tb_lead);
    std::vector<int> next(k.n_nonempty, 0);
    for (int64_t e = 0; e < n_items; ++e) {
        const int32_t b = L.tri_f[2 * e], I = L.tri_f[2 * e + 1];
        CHECK(b >= 0 && b < k.n_nonempty && k.h_m[b] >= t.tiled_min, "tri_f[%lld]: block %d", (long long)e, b);
        CHECK(I == next[b] && I < T(b), "tri_f[%lld]: (%d, %d) but the block's next tile is %d of %d", (long long)e, b, I, next[b], T(b));
        next[b]++;
        CHECK(L.tri_b[2 * e] == b && L.tri_b[2 * e + 1] == T(b) - 1 - I, "tri_b[%lld]: (%d, %d) is not the mirror of (%d, %d)", (long long)e,
              L.tri_b[2 * e], L.tri_b[2 * e + 1], b, I);
        if (split) CHECK(is_lead(b) == (e < k.n_titems_lead), "tri_f[%lld]: block %d on the wrong side of the lead split", (long long)e, b);
    }
    for (int32_t b : tiled) CHECK(next[b] == T(b), "tri_f: block %d has %d of %d tiles", b, next[b], T(b));
    std::vector<int32_t> tb = k.h_tb;
    if (split)
        for (size_t i = 0; i < tb.size(); ++i)
            CHECK(is_lead(tb[i]) == (static_cast<int>(i) < k.n_tb_lead), "h_tb[%zu] = %d on the wrong side of the lead split", i, tb[i]);
    std::sort(tb.begin(), tb.end());
    CHECK(tb == tiled, "h_tb is not the %zu tiled blocks", tiled.size());
    CHECK(k.sub_grid_lead >= 1 && k.sub_grid_rest >= 1, "grids %d %d", k.sub_grid_lead, k.sub_grid_rest);
    if (P.op.sub_grid_lead > 0) CHECK(k.sub_grid_lead == P.op.sub_grid_lead, "sub_grid_lead %d", k.sub_grid_lead);
    if (P.op.sub_grid_rest > 0) CHECK(k.sub_grid_rest == P.op.sub_grid_rest, "sub_grid_rest %d", k.sub_grid_rest);
    // both defaulted: the two persistent grids share the chip (each keeps one workgroup, so a
    // one-CU device gets two)
    if (P.op.sub_grid_lead == 0 && P.op.sub_grid_rest == 0)
        CHECK(k.sub_grid_lead + k.sub_grid_rest <= std::max(2, n_cu), "grids %d + %d on %d CUs", k.sub_grid_lead, k.sub_grid_rest, n_cu);
    // whole-block passes of the rest group: every rest block's work vector fits (<= 4096 rows)
    int tmax_rest = 0;
    std::vector<int32_t> rest;
    for (int32_t b : tiled)
        if (!is_lead(b)) { rest.push_back(b); tmax_rest = std::max(tmax_rest, T(b)); }
    const bool sub_block = split && P.op.sub_split == 2 && !rest.empty() && 64 * tmax_rest <= 4096;
    CHECK(k.sub_block == sub_block && k.n_tcheb == (sub_block ? static_cast<int>(rest.size()) : 0) &&
          k.tcheb_vld == (sub_block ? 64 * tmax_rest : 0) && static_cast<int>(L.tcheb_list.size()) == k.n_tcheb,
          "sub_block %d n_tcheb %d tcheb_vld %d", k.sub_block, k.n_tcheb, k.tcheb_vld);
    std::vector<int32_t> tc = L.tcheb_list;
    for (size_t i = 1; i < tc.size(); ++i) CHECK(k.h_m[tc[i - 1]] >= k.h_m[tc[i]], "tcheb_list[%zu]: not largest first", i);
    std::sort(tc.begin(), tc.end());
    if (sub_block) CHECK(tc == rest, "tcheb_list is not the rest group");
}

void check_workload(const Problem& P, const PlanLayout& L, const Thresholds& t) {
    const PlanLayout::Kept& k = L.keep;
    double ops = 0.0, sub_bytes = 0.0;
    int launches = 0;
    for (int b = 0; b < k.n_nonempty; ++b) {
        const double m = k.h_m[b], T = static_cast<double>(ceil_div(k.h_m[b], 64));
        ops += P.pr.n_ref * m * (m + 1);
        if (k.h_m[b] >= t.tiled_min) sub_bytes += T * (T + 1) / 2 * 64 * 64 * 8;
    }
    for (const auto* tl : {&k.tl, &k.tl_rest})
        for (const TLaunch& l : *tl) launches += l.kind != kTlRecord && l.kind != kTlWait;
    CHECK(k.wl[0] == static_cast<double>(k.n_s + k.n_l) && k.wl[3] == ops && k.wl[6] == k.n_nonempty &&
          k.wl[7] == k.n_tiles + k.n_btiles + k.n_htiles && k.wl[9] == k.n_large && k.wl[11] == k.n_tiled &&
          k.wl[12] == launches && k.wl[13] == sub_bytes && k.wl[14] == 0 && k.wl[15] == -1,
          "workload figures: %g %g %g %g %g %g %g %g", k.wl[0], k.wl[3], k.wl[6], k.wl[7], k.wl[9], k.wl[11], k.wl[12], k.wl[13]);
}

int g_layouts = 0;
void check_case(const std::string& name, const std::vector<int>& ms, bool has_l, int32_t n_ref, int n_cu,
                const dbslmm_options& op, int copies = 0) {
    g_case = name;
    Problem P(ms, has_l, n_ref);
    P.op = op;
    PlanLayout L;
    std::string err;
    const int rc = build_plan_layout(P.pr, P.op, n_cu, L, err);
    CHECK(rc == DBSLMM_OK, "refused: %s", err.c_str());
    const Thresholds t = thresholds(P);
    check_slots(P, L, t);
    check_gram(P, L, t);
    check_order(P, L, t);
    const PlanLayout::Kept& k = L.keep;
    std::vector<int32_t> lead, rest;
    for (int b = 0; b < k.n_nonempty; ++b)
        if (k.h_m[b] >= t.tiled_min) (t.lead_min == INT64_MAX || k.h_m[b] >= t.lead_min ? lead : rest).push_back(b);
    check_tiled(k.h_m, lead, 1, k.n_nonempty, k.tl, L.tlist, "tl");
    check_tiled(k.h_m, rest, 1, k.n_nonempty, k.tl_rest, L.tlist, "tl_rest");
    check_subst(P, L, t, n_cu);
    check_workload(P, L, t);
    if (copies > 1) {   // the merged sequence of an h2f run: every tiled block x copies (run_impl)
        std::vector<TLaunch> tl;
        std::vector<int32_t> tlist;
        build_tiled(k.h_m, k.h_tb, copies, k.n_nonempty, tl, tlist);
        check_tiled(k.h_m, k.h_tb, copies, k.n_nonempty, tl, tlist, "tl_multi");
    }
    ++g_layouts;
}

void check_refused(const std::string& name, Problem& P, const std::string& message) {
    g_case = name;
    PlanLayout L;
    std::string err;
    const int rc = build_plan_layout(P.pr, P.op, 256, L, err);
    CHECK(rc == DBSLMM_E_ARG && err == message, "rc %d, \"%s\"; expected \"%s\"", rc, err.c_str(), message.c_str());
}

}  // namespace

int main() {
    // block sizes at the rounding and class boundaries: ld = roundup(m + 1, 32 / 128), the small /
    // large Cholesky split (ld 64), the Gram kernels (96, 384 / 768), tiled_min (256 / 384), the
    // default lead group (1536), wide super steps and the whole-block passes (4096)
    const std::vector<int> all = {0, 1, 31, 32, 63, 64, 95, 96, 127, 128, 129, 255, 256, 383, 384, 511, 512, 513,
                                  1535, 1536, 4095, 4096, 4097};
    const dbslmm_options def{};
    auto with = [&](auto set) { dbslmm_options o{}; set(o); return o; };
    check_case("all sizes, defaults", all, true, 503, 256, def, 3);
    check_case("all sizes, n_ref 4100 (256-tile Gram from 384)", all, true, 4100, 256, def);
    check_case("all sizes, tiled_min 64", all, true, 503, 256, with([](dbslmm_options& o) { o.tiled_min = 64; }), 3);
    check_case("all sizes, lead_min -1", all, true, 503, 256, with([](dbslmm_options& o) { o.lead_min = -1; }));
    check_case("all sizes, lead_min 128", all, true, 503, 256, with([](dbslmm_options& o) { o.lead_min = 128; }));
    check_case("all sizes, lead_min 128, small Gram thresholds", all, true, 503, 256,
               with([](dbslmm_options& o) { o.lead_min = 128; o.tiled_min = 64; o.gram_huge_min = 128; o.gram_big_min = 32; }));
    check_case("all sizes, sub_split -1", all, true, 503, 256, with([](dbslmm_options& o) { o.sub_split = -1; }));
    check_case("all sizes, sub_split 2", all, true, 503, 256, with([](dbslmm_options& o) { o.sub_split = 2; }));
    check_case("sizes to 1536, sub_split 2, lead_min 1024", {513, 1535, 1536, 384, 64, 1024}, true, 503, 256,
               with([](dbslmm_options& o) { o.sub_split = 2; o.lead_min = 1024; }));
    check_case("all sizes, cheb_fused, fixed grids", all, true, 503, 256,
               with([](dbslmm_options& o) { o.cheb_fused = 1; o.sub_grid_lead = 7; o.sub_grid_rest = 300; }));
    check_case("all sizes, large_cheb off, tiled_min 1024", all, true, 503, 256,
               with([](dbslmm_options& o) { o.large_cheb = -1; o.tiled_min = 1024; }));
    check_case("largest block 511", {0, 1, 31, 32, 63, 64, 95, 96, 127, 128, 129, 255, 256, 383, 384, 511}, true, 503, 256, def, 2);
    check_case("LMM only", all, false, 503, 256, def);
    check_case("only empty blocks", {0, 0, 0}, true, 503, 256, def);
    check_case("no blocks", {}, true, 503, 256, def);
    check_case("all sizes, 1 CU", all, true, 503, 1, def);
    check_case("all sizes, 304 CUs", all, true, 503, 304, def);
    check_case("a tiled block of 32639 SNPs", {32639, 100}, true, 503, 256, def);

    {
        Problem P({100, 32640}, true, 503);
        check_refused("a tiled block of 32640 SNPs", P, "LD block too large for the tiled path (m must be < 32640 SNPs)");
    }
    {
        Problem P({100, 200, 300}, true, 503);
        P.s_ptr[2] = P.s_ptr[1] - 1;
        check_refused("CSR offsets not monotone", P, "CSR offsets not monotone");
    }
    {
        Problem P({100, 200, 300}, true, 503);
        P.s_pos[150] = 600;   // the .bed holds rows 0 .. 599
        check_refused("small bed row past the image", P, "small SNP bed row out of range");
        P.s_pos[150] = 0;
        P.l_pos[7] = -1;
        check_refused("negative large bed row", P, "large SNP bed row out of range");
    }
    {
        Problem P({100}, true, 503);
        P.op.sub_split = 3;
        check_refused("bad options", P, "bad dbslmm_options");
    }
    printf("ok %d layouts\n", g_layouts);
    return 0;
}
