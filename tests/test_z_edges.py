"""The solve at the edges of its right-hand side: z scaled by +-2^k, and one non-finite z in one block.

Every test runs _common.pcg_case() (blocks of 70 / 600 / 200 / 1030 / 1100 / 0 / 40 SNPs, large SNPs
in two of them, d = 1 / (sigma_s n) = 20) over ROUTES: the PCG route (whole-block kernel beside the
chip-wide kernels, everything chip-wide, 1 and 3 copies, the fp64 Sigma of a block with a missing
call, stream_out on and off, three shards) and, with solver = 1, the factorisation route (default
dispatch, tiled_min = 64, a lead group, run_multi of three sigmas by Chebyshev, CG, the merged
factorisation, sub_split = 2 and cheb_fused = 1, LMM-only, three shards).  Every run asserts
plan.workload()["pcg_route"].

A -- homogeneity.  Every stopping rule is relative (|r| <= tol lambda |x|, r = 0, Chebyshev's a priori
count, CG on the factor with its comparisons against 0), so multiplying every z by c = +-2^k commutes
with every rounding: beta(c z) == c beta(z) elementwise under ==, with the same statuses and the
same block_iters, for c in {-1, 2^40, 2^-40, -2^100}.  No tolerance.  CPU precondition: c z is exact
and z^2, (c z)^2 stay inside the normal fp64 range (the residuals fall by 1e-12 relative, their
squares by 1e-24: far inside too).  Magnitudes whose squares overflow or underflow are OUTSIDE what
this asserts (the PCG's rr == 0.0 test would call an underflowed residual
converged).

B -- one poisoned block.  One entry of one block's z is NaN, +Inf or -Inf (COMBOS: each block kind
with each value once, at the first, a middle and the last joint index [small | large]; the last
index of a block with large SNPs is a z_l entry).  CPU precondition, from the oracle alone: its
direct solve of the poisoned problem is non-finite in every beta of that block at every sigma and
equals the clean solve everywhere else.  On the GPU: every other block's betas, status and
block_iters are the clean run's bit for bit in every copy (the poisoned plan is a fresh one; it runs
twice; a clean plan on the same context follows it -- a plan owns its z, so "the clean run after the
poisoned one" is a second plan on the context the poisoned one used); every beta of the poisoned
block is non-finite; its status is DBSLMM_BLOCK_NOT_CONVERGED on the PCG route, where it ran exactly
pcg_maxit = twice the clean run's largest block_iters, and DBSLMM_BLOCK_OK in every copy on the
factorisation route (include/dbslmm_hip.h); a streamed run's arrays equal
download(); the score drops exactly that block's SNPs; the variance does not move; units plans
fill what the sharded context fills.

C -- the CLI on a 3-chromosome panel whose summary files hold a `nan` beta, an `inf` beta and an
se of 1e-19 (z ~ 1e16 .. 1e18: finite, solved normally), on the production route and with -h2f.
"""
import dataclasses
import functools
import os
import subprocess

import numpy as np
import pytest

import oracle as O
import ref_numpy as R
from _common import PCG_LARGE, PCG_SIZES, ROOT, pcg_case

F3 = (0.8, 1.0, 1.2)
F1 = (1.0,)
DEVS = [0, 0, 0]
SCALES = {"minus1": -1.0, "2p40": 2.0 ** 40, "2m40": 2.0 ** -40, "minus2p100": -(2.0 ** 100)}

# id -> (family, pcg_case keywords, plan options, h2f factors, devices)
ROUTES = {
    "pcg-default-3": ("pcg", {}, {}, F3, 0),
    "pcg-default-1": ("pcg", {}, {}, F1, 0),
    "pcg-chipwide-3": ("pcg", {}, dict(pcg_whole=-1), F3, 0),
    "pcg-chipwide-1": ("pcg", {}, dict(pcg_whole=-1), F1, 0),
    "pcg-miss-3": ("pcg", dict(miss_block=2), {}, F3, 0),
    "pcg-nostream-3": ("pcg", {}, dict(stream_out=0), F3, 0),
    "pcg-sharded-3": ("pcg", {}, {}, F3, DEVS),
    "fac-default-1": ("fac", {}, dict(solver=1), F1, 0),
    "fac-tiled64-1": ("fac", {}, dict(solver=1, tiled_min=64), F1, 0),
    "fac-lead-1": ("fac", {}, dict(solver=1, tiled_min=64, lead_min=1000), F1, 0),
    "fac-cheb-3": ("fac", {}, dict(solver=1, h2f_iter=1), F3, 0),
    "fac-cg-3": ("fac", {}, dict(solver=1, h2f_iter=2), F3, 0),
    "fac-merged-3": ("fac", {}, dict(solver=1, h2f_mode=1), F3, 0),
    "fac-whole-3": ("fac", {}, dict(solver=1, tiled_min=64, lead_min=1000, sub_split=2, h2f_iter=1), F3, 0),
    "fac-fused-3": ("fac", {}, dict(solver=1, tiled_min=64, h2f_iter=1, cheb_fused=1), F3, 0),
    "fac-lmm-3": ("fac", dict(lmm=True), dict(solver=1), F3, 0),
    "fac-sharded-3": ("fac", {}, dict(solver=1), F3, DEVS),
}
ITERATED = ("fac-cheb-3", "fac-cg-3", "fac-whole-3", "fac-fused-3", "fac-lmm-3")

# (block, value, joint index): W = a whole-block-kernel block, C = chip-wide blocks (> 1024 SNPs: with
# large SNPs, and the multi-shift one), S = the 40-SNP block, F = the block whose Sigma is fp64 in the
# miss_block variant (elsewhere a whole-block block with large SNPs: one sequence per copy)
W, F, C0, C, S = 1, 2, 3, 4, 6
NAN, INF = float("nan"), float("inf")
COMBOS = [(W, NAN, "first"), (W, INF, "middle"), (W, -INF, "last"),
          (C, NAN, "last"), (C, INF, "first"), (C, -INF, "middle"), (C0, INF, "middle"),
          (S, NAN, "middle"), (S, INF, "last"), (S, -INF, "first"),
          (F, NAN, "first"), (F, INF, "last"), (F, -INF, "middle")]


def _cid(combo):
    b, v, where = combo
    return f"b{b}-{'nan' if v != v else 'pinf' if v > 0 else 'ninf'}-{where}"


# ----------------------------------------------------------------------------- problems
def block_m(prob, b):
    ms = int(prob.s_ptr[b + 1] - prob.s_ptr[b])
    return ms, 0 if prob.l_ptr is None else int(prob.l_ptr[b + 1] - prob.l_ptr[b])


def of(prob, res, b):
    """[beta_s | beta_l] of block b from (beta_s, beta_l, ...)."""
    s = res[0][prob.s_ptr[b]:prob.s_ptr[b + 1]]
    return s if prob.l_ptr is None else np.concatenate([s, res[1][prob.l_ptr[b]:prob.l_ptr[b + 1]]])


def poison(prob, combo):
    """Put the combo's value at its joint index of its block; returns "z_s" or "z_l"."""
    b, value, where = combo
    ms, ml = block_m(prob, b)
    j = {"first": 0, "middle": (ms + ml) // 2, "last": ms + ml - 1}[where]
    prob.z_s = prob.z_s.copy()
    if j < ms:
        prob.z_s[prob.s_ptr[b] + j] = value
        return "z_s"
    prob.z_l = prob.z_l.copy()
    prob.z_l[prob.l_ptr[b] + j - ms] = value
    return "z_l"


def scale(prob, c):
    prob.z_s = prob.z_s * c
    if prob.z_l is not None:
        prob.z_l = prob.z_l * c


def problem(route, edit=None, **more):
    """A fresh case of the route (its options, plus `more`), its z edited before any plan sees it."""
    _, kw, opts, _, _ = ROUTES[route]
    c = pcg_case(**kw, **dict(opts, **more))
    if edit is not None:
        edit(c.prob)
    return c


def sigmas_of(route, prob):
    return [prob.sigma_s * f for f in ROUTES[route][3]]


# ----------------------------------------------------------------------------- CPU preconditions
def test_routes_and_combos_cover_what_they_claim():
    """Every block kind meets NaN, +Inf and -Inf once, z_l is hit in both blocks with large SNPs,
    every position is used for every kind that has three combos; both families have every route
    kind the module docstring lists."""
    assert (PCG_SIZES, PCG_LARGE) == ((70, 600, 200, 1030, 1100, 0, 40), (0, 0, 2, 0, 3, 0, 0))
    for b in (W, C, S, F):
        mine = [x for x in COMBOS if x[0] == b]
        assert sorted(_cid(x).split("-")[1] for x in mine) == ["nan", "ninf", "pinf"]
        assert sorted(x[2] for x in mine) == ["first", "last", "middle"]
    assert PCG_SIZES[W] <= 1024 and PCG_LARGE[W] == 0 and PCG_SIZES[C] > 1024 and PCG_LARGE[C] > 0
    assert PCG_SIZES[C0] > 1024 and PCG_LARGE[C0] == 0 and PCG_SIZES[S] == 40 and PCG_LARGE[F] > 0
    hits = {x: poison(pcg_case().prob, x) for x in COMBOS}
    assert {x[0] for x, h in hits.items() if h == "z_l"} == {C, F}
    assert ROUTES["pcg-miss-3"][1]["miss_block"] == F
    fam = [v[0] for v in ROUTES.values()]
    assert fam.count("pcg") == 7 and fam.count("fac") == 10
    assert sum(1 for v in ROUTES.values() if v[4] == DEVS) == 2


@pytest.mark.parametrize("name", list(SCALES))
def test_scaling_is_exact_and_inside_the_normal_range(name):
    """c z is exact (c is a power of two and no product leaves the normal range: dividing gives z
    back bit for bit, and the mantissas are z's), and z^2, (c z)^2 are normal fp64 numbers."""
    c = SCALES[name]
    assert np.frexp(abs(c))[0] == 0.5
    tiny, huge = np.finfo(np.float64).tiny, np.finfo(np.float64).max
    for kw in ({}, dict(lmm=True)):
        p = pcg_case(**kw).prob
        for z in (p.z_s,) + (() if p.z_l is None else (p.z_l,)):
            cz = z * c
            assert np.array_equal(cz / c, z) and np.array_equal(np.frexp(np.abs(cz))[0], np.frexp(np.abs(z))[0])
            assert np.all(z != 0.0)
            for v in (z, cz):
                sq = v * v
                assert np.all(sq >= tiny) and np.all(sq <= huge) and np.all(np.isfinite(sq))
            # the squares of residuals 1e-12 of z (and 1e-3 below that for single entries) too
            assert np.min(np.abs(cz)) * 1e-15 > np.sqrt(tiny) and np.max(np.abs(cz)) * 1e3 < np.sqrt(huge)


VARIANTS = {"plain": {}, "miss": dict(miss_block=F), "lmm": dict(lmm=True)}


@functools.lru_cache(maxsize=None)
def oracle_direct(variant, combo, factor):
    kw = VARIANTS[variant]
    p = pcg_case(**kw).prob
    if combo is not None:
        poison(p, combo)
    bs, bl, st, _ = O.est(p.bed, p.n_ref, p.n_obs, p.sigma_s * factor, p.s_ptr, p.s_pos, p.z_s, p.l_ptr, p.l_pos,
                          p.z_l, tau=p.tau, method="direct", threads=8)
    return bs, bl, st


def combos_of(variant):
    if variant == "miss":
        return [x for x in COMBOS if x[0] == F]          # (the other blocks are the plain problem's)
    return COMBOS


@pytest.mark.parametrize("f", F3)
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_oracle_poisons_exactly_one_block(variant, f):
    """The reference's algebra from the oracle alone: a non-finite z entry makes every beta of its
    block non-finite at every sigma and leaves every other block at the clean solve's values."""
    p = pcg_case(**VARIANTS[variant]).prob
    ref = oracle_direct(variant, None, f)
    assert np.all(np.isfinite(ref[0])) and np.all(np.isfinite(ref[1]))
    for combo in combos_of(variant):
        got = oracle_direct(variant, combo, f)
        for b in range(p.num_block):
            g, r = of(p, got, b), of(p, ref, b)
            if b == combo[0]:
                assert g.size == sum(block_m(p, b)) > 0 and not np.any(np.isfinite(g)), (variant, f, combo)
            else:
                np.testing.assert_array_equal(g, r, err_msg=f"{variant} {f} {combo} block {b}")


# ----------------------------------------------------------------------------- GPU plumbing
_CTX = {}


def ctx(route):
    from dbslmm_amd import Context
    dev = ROUTES[route][4]
    key = tuple(dev) if isinstance(dev, list) else dev
    if key not in _CTX:
        _CTX[key] = Context(dev)
    return _CTX[key]


@dataclasses.dataclass
class Run:
    copies: list          # [(beta_s, beta_l, status)] in the caller's arrays
    iters: np.ndarray
    wl: dict
    down: tuple


def solve(route, c, runs=1, keep=False):
    """run_multi of the route's sigmas on a fresh plan, `runs` times: a Run each (and the plan)."""
    from dbslmm_amd import Plan
    fam = ROUTES[route][0]
    p = c.prob
    sig = sigmas_of(route, p)
    n = len(sig)
    plan = Plan(ctx(route), p)
    out = []
    for _ in range(runs):
        arrays = (np.full((n, p.n_s), -7.25), np.full((n, p.n_l), -7.25), np.full((n, p.num_block), -99, dtype=np.int32))
        copies = plan.run_multi(sig, out=arrays)
        wl = plan.workload()
        assert wl["pcg_route"] == (1 if fam == "pcg" else 0), (route, wl["pcg_route"])
        out.append(Run(copies, plan.block_iters(), wl, plan.download()))
    check_route(route, out[-1].wl)
    if keep:
        return out, plan
    plan.close()
    return out


def check_route(route, wl):
    """What shows that the options took the dispatch they name (one device: a sharded plan's
    counts are per shard)."""
    fam, kw, opts, factors, dev = ROUTES[route]
    if fam == "pcg" or dev == DEVS:
        return
    tmin = opts.get("tiled_min", 384)
    sizes = [m for m in PCG_SIZES if m > 0]
    assert wl["blocks_tiled"] == sum(1 for m in sizes if m >= tmin), (route, wl["blocks_tiled"])
    if route in ITERATED:
        assert wl["cheb_base"] == 1 and wl["cheb_iters"] > 0, (route, wl["cheb_base"], wl["cheb_iters"])
    else:
        assert wl["cheb_iters"] == 0, (route, wl["cheb_iters"])


_CLEAN = {}


def clean(route):
    """The clean problem on the route, once: (Run with the default cap, cap, Run with pcg_maxit =
    cap).  cap = twice the largest block_iters of the first run (PCG route; 0 = the default on the
    factorisation route, whose block_iters are all 0)."""
    if route not in _CLEAN:
        first = solve(route, problem(route))[0]
        cap = 2 * int(first.iters.max())
        if ROUTES[route][0] == "pcg":
            assert 10 <= cap <= 200, cap
            capped = solve(route, problem(route, pcg_maxit=cap))[0]
            same(capped, first, f"{route}: the cap changes nothing in a clean run")
        else:
            assert cap == 0
            capped = first
        p = problem(route).prob
        for k, r in enumerate(capped.copies):
            assert np.all(np.isfinite(r[0])) and np.all(np.isfinite(r[1])), (route, k)
            assert r[2].tolist() == [1 if m == 0 else 0 for m in PCG_SIZES], (route, k, r[2])
        assert np.all((capped.iters > 0) == ((np.array(PCG_SIZES) > 0) & (ROUTES[route][0] == "pcg")))
        _CLEAN[route] = (first, cap, capped)
    return _CLEAN[route]


def same(a, b, what, skip=None, prob=None):
    """Two Runs equal bit for bit (NaNs at the same places): every copy's betas and statuses and
    the block_iters; skip: a block left out (needs prob)."""
    assert len(a.copies) == len(b.copies)
    if skip is None:
        for k, (x, y) in enumerate(zip(a.copies, b.copies)):
            for u, v in zip(x, y):
                np.testing.assert_array_equal(u, v, err_msg=f"{what}, copy {k}")
        np.testing.assert_array_equal(a.iters, b.iters, err_msg=what)
        return
    keep = np.arange(prob.num_block) != skip
    for k, (x, y) in enumerate(zip(a.copies, b.copies)):
        for blk in np.flatnonzero(keep):
            np.testing.assert_array_equal(of(prob, x, blk), of(prob, y, blk), err_msg=f"{what}, copy {k}, block {blk}")
        np.testing.assert_array_equal(x[2][keep], y[2][keep], err_msg=f"{what}, copy {k}: statuses")
    np.testing.assert_array_equal(a.iters[keep], b.iters[keep], err_msg=f"{what}: block_iters")


def check_poisoned(route, combo, run, what, ref=None):
    """One poisoned Run against the clean one of the same options (ref: clean(route)'s)."""
    from dbslmm_amd import BLOCK_NOT_CONVERGED, BLOCK_OK
    fam = ROUTES[route][0]
    cap = clean(route)[1]
    ref = ref or clean(route)[2]
    p = problem(route).prob
    b = combo[0]
    same(run, ref, what, skip=b, prob=p)
    for k, r in enumerate(run.copies):
        v = of(p, r, b)
        assert v.size == PCG_SIZES[b] and not np.any(np.isfinite(v)), (what, k, int(np.isfinite(v).sum()))
        assert r[2][b] == (BLOCK_NOT_CONVERGED if fam == "pcg" else BLOCK_OK), (what, k, r[2])
    assert run.iters[b] == cap, (what, run.iters, cap)
    if fam == "pcg":
        for u, v in zip(run.down, run.copies[-1]):       # (stream_out on or off: the caller's arrays)
            np.testing.assert_array_equal(u, v, err_msg=f"{what}: download()")


# ----------------------------------------------------------------------------- A on the GPU
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCALES))
@pytest.mark.parametrize("route", list(ROUTES))
def test_scaled_z_scales_beta_bit_for_bit(route, name):
    c = SCALES[name]
    ref = clean(route)[0]
    got = solve(route, problem(route, edit=lambda p: scale(p, c)))[0]
    for k, (g, r) in enumerate(zip(got.copies, ref.copies)):
        for j in (0, 1):
            want = c * r[j]
            bad = np.flatnonzero(~((g[j] == want) | (np.isnan(g[j]) & np.isnan(want))))
            assert bad.size == 0, (route, name, k, "beta_l" if j else "beta_s", bad[:5], g[j][bad[:5]], want[bad[:5]])
        np.testing.assert_array_equal(g[2], r[2], err_msg=f"{route} {name}: status of copy {k}")
    np.testing.assert_array_equal(got.iters, ref.iters, err_msg=f"{route} {name}: block_iters")
    assert got.wl["pcg_iters"] == ref.wl["pcg_iters"] and got.wl["cheb_iters"] == ref.wl["cheb_iters"]


# ----------------------------------------------------------------------------- B on the GPU
@pytest.mark.gpu
@pytest.mark.parametrize("combo", COMBOS, ids=[_cid(x) for x in COMBOS])
@pytest.mark.parametrize("route", list(ROUTES))
def test_poisoned_block_stays_alone(route, combo):
    _, cap, ref = clean(route)
    c = problem(route, edit=lambda p: poison(p, combo), **({"pcg_maxit": cap} if cap else {}))
    runs, plan = solve(route, c, runs=2, keep=True)
    what = f"{route} {_cid(combo)}"
    check_poisoned(route, combo, runs[0], what + ", a fresh plan")
    check_poisoned(route, combo, runs[1], what + ", the plan's second run")
    # a clean plan on the context the poisoned plan used (and still holds buffers on)
    after = solve(route, problem(route, **({"pcg_maxit": cap} if cap else {})))[0]
    plan.close()
    same(after, ref, what + ": the clean run after the poisoned one")


FAMILY = {"pcg": "pcg-default-3", "fac": "fac-cg-3"}
CONSUMER_COMBOS = [(C, NAN, "last"), (W, INF, "middle"), (F, -INF, "middle")]


@pytest.mark.gpu
@pytest.mark.parametrize("combo", CONSUMER_COMBOS, ids=[_cid(x) for x in CONSUMER_COMBOS])
@pytest.mark.parametrize("fam", list(FAMILY))
def test_score_drops_the_poisoned_block_and_variance_does_not_move(fam, combo):
    """plan.score (counts and std) after a poisoned run: every copy's dropped count is the clean
    run's plus the block's SNPs, and the scores are bit for bit the clean run's with weight 0 on
    that block's SNPs (score.hip: a SNP whose beta w is not finite contributes nothing).
    plan.variance reads the matrix alone: bit for bit the clean run's."""
    route = FAMILY[fam]
    _, cap, ref = clean(route)
    more = {"pcg_maxit": cap} if cap else {}
    b = combo[0]
    cc = problem(route, **more)
    p = cc.prob
    ws, wl = np.ones(p.n_s), np.ones(p.n_l)
    ws[p.s_ptr[b]:p.s_ptr[b + 1]] = 0.0
    wl[p.l_ptr[b]:p.l_ptr[b + 1]] = 0.0
    (crun,), cplan = solve(route, cc, keep=True)
    same(crun, ref, "the clean plan")
    pc = problem(route, edit=lambda q: poison(q, combo), **more)
    (prun,), pplan = solve(route, pc, keep=True)
    check_poisoned(route, combo, prun, f"{route} {_cid(combo)}")
    for mode in ("counts", "std"):
        want, d0 = cplan.score(cc.tbed, cc.ind, cc.ts_pos, cc.tl_pos, mode=mode, w_s=ws, w_l=wl)
        got, d1 = pplan.score(pc.tbed, pc.ind, pc.ts_pos, pc.tl_pos, mode=mode, w_s=np.ones(p.n_s), w_l=np.ones(p.n_l))
        assert got.shape == want.shape == (len(ROUTES[route][3]), int((cc.ind != 0).sum()))
        assert np.all(np.isfinite(got)) and np.any(got != 0.0)
        assert d1.tolist() == (d0 + PCG_SIZES[b]).tolist(), (mode, d0, d1)
        np.testing.assert_array_equal(got, want, err_msg=f"{route} {_cid(combo)} {mode}")
    v0 = cplan.variance(cc.tbed, cc.ind, cc.ts_pos, cc.tl_pos)
    v1 = pplan.variance(pc.tbed, pc.ind, pc.ts_pos, pc.tl_pos)
    assert np.all(np.isfinite(v0)) and np.any(v0 != 0.0)
    np.testing.assert_array_equal(v1, v0, err_msg=f"{route} {_cid(combo)}: variance")
    cplan.close()
    pplan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("fam", list(FAMILY))
def test_units_plans_fill_what_the_sharded_context_fills(fam):
    """Plan.units over the three device indices of the problem's shard plan, a poisoned block
    among them: together the arrays of the sharded context's run, bit for bit.  On the
    factorisation route the shard plan splits the copies of the two big blocks over the devices
    (each copy factored directly), and the context follows that plan with shard_copies = 3: the
    clean reference here is the sharded context's run with that option, and the poisoned block is
    one of the split ones."""
    from dbslmm_amd import Context, Plan
    from dbslmm_amd.dist import shard_units_problem
    route = {"pcg": "pcg-sharded-3", "fac": "fac-sharded-3"}[fam]
    combo = (C, NAN, "last")
    _, cap, ref = clean(route)
    more = {"pcg_maxit": cap} if cap else {"shard_copies": 3}
    c = problem(route, edit=lambda q: poison(q, combo), **more)
    if fam == "fac":
        ref = solve(route, problem(route, **more))[0]
        assert all(np.all(np.isfinite(r[0])) and np.all(np.isfinite(r[1])) for r in ref.copies)
    sharded = solve(route, c)[0]
    check_poisoned(route, combo, sharded, f"{route} {_cid(combo)}", ref=ref)
    p = c.prob
    sig = sigmas_of(route, p)
    ud, _ = shard_units_problem(p, sig, 3)
    full = np.array(PCG_SIZES) > 0
    assert set(ud[full].reshape(-1).tolist()) == {0, 1, 2}
    assert (len(set(ud[C].tolist())) == 3) == (fam == "fac")         # (copy-split on the factorisation route alone)
    bs, bl = np.full((3, p.n_s), -7.25), np.full((3, p.n_l), -7.25)
    st = np.full((3, p.num_block), -99, dtype=np.int32)
    one = Context(0)
    for d in range(3):
        u = Plan.units(one, p, ud, d)
        u.run_multi(sig, out=(bs, bl, st))
        assert u.workload()["pcg_route"] == (1 if fam == "pcg" else 0)
        u.close()
    for k in range(3):
        np.testing.assert_array_equal(bs[k], sharded.copies[k][0])
        np.testing.assert_array_equal(bl[k], sharded.copies[k][1])
        np.testing.assert_array_equal(st[k][full], sharded.copies[k][2][full])
    one.close()


# ----------------------------------------------------------------------------- C: the CLI
CLI = os.path.join(ROOT, "dbslmm_amd", "bin", "dbslmm")
CLI_N, CLI_NSNP, CLI_H = 100000, 1000000, 0.5            # d = nsnp / (h n) = 20: the production route
CLI_H2F = ("0.8", "1", "1.2")
BAR = 1e-10


class CliCase:
    pass


@pytest.fixture(scope="module")
def cli_case(tmp_path_factory):
    """A 3-chromosome synthetic panel and two sets of summary files: clean, and with three rows of
    three different blocks of small SNPs edited -- beta `nan`, beta `inf`, se 1e-19."""
    from dbslmm_amd import synth
    from test_cli import _oracle_host
    d = tmp_path_factory.mktemp("z_edges_cli")
    panel = synth.simulate(7000, 250, pop="EUR", chroms=[19, 20, 21], seed=5, large_every=3, miss_rate=0.002)
    f = synth.write_plink(panel, str(d / "p"))
    bim = R.read_bim(f["ref"], panel.n_ref, True)
    c = CliCase()
    c.dir, c.panel, c.f = d, panel, f
    c.blocks, _, _, c.info_s, c.info_l, bad = _oracle_host(f, bim, 0.2)
    assert bad == [] and len(c.info_s) + len(c.info_l) == panel.m
    # three blocks of the three chromosomes with at least 40 small SNPs each
    blk_s = np.array([e["block"] for e in c.info_s])
    sizes = np.bincount(blk_s, minlength=len(c.blocks))
    pick = []
    for chrom in ("chr19", "chr20", "chr21"):
        own = [b for b, x in enumerate(c.blocks) if x[0] == chrom and sizes[b] >= 40]
        pick.append(own[len(own) // 2])
    c.blk = dict(zip(("nan", "inf", "huge"), pick))
    c.snp = {k: c.info_s[int(np.flatnonzero(blk_s == b)[sizes[b] // 2])]["snp"] for k, b in c.blk.items()}
    lines = open(f["s"]).read().splitlines()
    out, seen = [], set()
    for line in lines:
        t = line.split("\t")
        for k, snp in c.snp.items():
            if t[1] == snp:
                seen.add(k)
                if k == "huge":
                    t[9] = "1e-19"
                else:
                    t[8] = k
        out.append("\t".join(t))
    assert seen == {"nan", "inf", "huge"}
    c.s_bad = str(d / "summ_s_bad.txt")
    open(c.s_bad, "w").write("\n".join(out) + "\n")
    _, _, _, c.info_s_bad, c.info_l_bad, bad = _oracle_host(dict(f, s=c.s_bad), bim, 0.2)
    assert bad == [] and [e["snp"] for e in c.info_s_bad] == [e["snp"] for e in c.info_s]
    c.row_block = np.array([e["block"] for e in c.info_l + c.info_s])
    c.expected = {}
    return c


def cli_expected(c, h):
    """ref_numpy.est (direct: one Cholesky per block) of the edited files at heritability h, once."""
    if h not in c.expected:
        c.expected[h] = R.est(c.panel.bed, c.panel.n_ref, CLI_N, h / CLI_NSNP, len(c.blocks), c.info_s_bad,
                              c.info_l_bad, tau=0.8, method="chol")
    return c.expected[h]


def test_cli_summary_edits_from_the_restatement_alone(cli_case):
    """readSumm's z of the three edited rows (NaN, +Inf, ~1e16 .. 1e18 and finite), and the
    restatement's solve of the edited files: every beta of the `nan` and of the `inf` block is NaN
    (so every row is written: the writer skips only an infinite beta / sqrt(2 maf (1 - maf))), the
    huge-z block is finite, every other block is the clean files' solve."""
    c = cli_case
    z = {e["snp"]: e["z"] for e in c.info_s_bad}
    assert np.isnan(z[c.snp["nan"]]) and z[c.snp["inf"]] == np.inf
    assert np.isfinite(z[c.snp["huge"]]) and 1e15 < abs(z[c.snp["huge"]]) < 1e19
    assert len(set(c.blk.values())) == 3
    res = cli_expected(c, CLI_H)
    clean = R.est(c.panel.bed, c.panel.n_ref, CLI_N, CLI_H / CLI_NSNP, len(c.blocks), c.info_s, c.info_l, tau=0.8,
                  method="chol")
    got, ref = np.concatenate([res.beta_l, res.beta_s]), np.concatenate([clean.beta_l, clean.beta_s])
    assert np.all(np.isfinite(ref))
    for b in np.unique(c.row_block):
        k = c.row_block == b
        if b in (c.blk["nan"], c.blk["inf"]):
            assert np.all(np.isnan(got[k])), (b, got[k])
        elif b == c.blk["huge"]:
            assert np.all(np.isfinite(got[k])) and np.max(np.abs(got[k])) > 1e6 * np.max(np.abs(ref[k]))
        else:
            np.testing.assert_array_equal(got[k], ref[k])
    assert len(R.format_eff(res)) == len(R.format_eff(clean)) == c.panel.m


def _cli(args, cwd):
    return subprocess.run([CLI] + args, capture_output=True, text=True, cwd=str(cwd), timeout=300)


def _rows(path):
    return [x.split() for x in open(path).read().splitlines() if x.strip()]


def check_cli_file(c, path, clean_path, h, what):
    res = cli_expected(c, h)
    exp = [x.split() for x in R.format_eff(res)]
    got, cl = _rows(path), _rows(clean_path)
    key = lambda rows: [(x[0], x[1], x[4]) for x in rows]
    assert key(got) == key(exp) == key(cl) and len(got) == c.panel.m, what
    ref = np.concatenate([res.beta_l, res.beta_s])
    val = np.array([float(x[2]) for x in got])
    text = open(path).read().splitlines(), open(clean_path).read().splitlines()
    for b in np.unique(c.row_block):
        k = np.flatnonzero(c.row_block == b)
        if b in (c.blk["nan"], c.blk["inf"]):
            # nan / inf exactly where the restatement prints them (the sign of a NaN is not a value)
            for i in k:
                assert got[i][2].lstrip("-") == exp[i][2].lstrip("-") == "nan", (what, b, got[i], exp[i])
                assert got[i][3].lstrip("-") == exp[i][3].lstrip("-") == "nan", (what, b, got[i], exp[i])
        elif b == c.blk["huge"]:
            err = float(np.max(np.abs(val[k] - ref[k])) / np.max(np.abs(ref[k])))
            print(f"{what}: the huge-z block vs the direct solve {err:.3e}")
            assert np.all(np.isfinite(val[k])) and err <= BAR, (what, err)
        else:
            assert [text[0][i] for i in k] == [text[1][i] for i in k], (what, b)


def cli_base(c, s):
    f = c.f
    return ["-s", s, "-l", f["l"], "-r", f["ref"], "-b", f["b"], "-n", str(CLI_N), "-nsnp", str(CLI_NSNP), "-mafMax",
            "0.2", "--precise-out", "-h", str(CLI_H)]


@pytest.mark.gpu
def test_cli_production_route_with_nonfinite_summary_rows(cli_case):
    from dbslmm_amd import Context, Plan, synth
    c = cli_case
    prob = synth.make_problem(c.panel)
    prob.n_obs, prob.sigma_s = CLI_N, CLI_H / CLI_NSNP
    plan = Plan(Context(0), prob)
    plan.run()
    plan.sync()
    assert plan.workload()["pcg_route"] == 1             # the route of these -n / -nsnp / -h
    plan.close()
    outs = {}
    for name, s in (("clean", c.f["s"]), ("bad", c.s_bad)):
        outs[name] = str(c.dir / f"prod_{name}")
        r = _cli(cli_base(c, s) + ["-eff", outs[name]], c.dir)
        assert r.returncode == 0, r.stderr
    check_cli_file(c, outs["bad"] + ".txt", outs["clean"] + ".txt", CLI_H, "production route")


@pytest.mark.gpu
def test_cli_h2f_with_nonfinite_summary_rows(cli_case):
    c = cli_case
    assert all(CLI_NSNP / (CLI_H * float(x) * CLI_N) >= 2.0 for x in CLI_H2F)
    outs = {}
    for name, s in (("clean", c.f["s"]), ("bad", c.s_bad)):
        outs[name] = str(c.dir / f"h2f_{name}")
        r = _cli(cli_base(c, s) + ["-h2f", ",".join(CLI_H2F), "-eff", outs[name] + ".dbslmm"], c.dir)
        assert r.returncode == 0, r.stderr
    for hh in CLI_H2F:
        check_cli_file(c, f"{outs['bad']}_h2f{hh}.dbslmm.txt", f"{outs['clean']}_h2f{hh}.dbslmm.txt",
                       CLI_H * float(hh), f"-h2f {hh}")
