"""The PCG route (pcg.hip, run_pcg in route_pcg.hip) through everything downstream of the solve: sharded
contexts, units plans, copy-split units, the variance's forced factorisation re-solve
(pcg_pending_var), route changes on one plan and the drop-in CLI on its production route.  The
route's own numerics are test_pcg.py's subject; here every problem has the flagship prior shift
(n_obs = 100000, sigma_s = 0.5 / 1e6: d = 1 / (sigma_s n_obs) = 20), so the auto rule takes the
PCG route with no solver option, and every test asserts plan.workload()["pcg_route"], so that none
can pass on the other route.

Bars: parity with the oracle's direct solve per block, max |dbeta| / max |beta_block| <= 1e-10
(the stopping rule bounds the relative 2-norm error of a block and copy by
1e-12, so the max-norm error by sqrt(m) 1e-12 <= 3.4e-11 at m = 1103); the variance within
test_variance.TOL (1e-8 per block column) of the literal formulas; "bit for bit" wherever a
block's path is a function of the block and the number of copies alone (DESIGN.md sections 3.6
and 6: fixed reduction orders) -- sharding, units plans, repeated runs and runs after a route
change may not move a bit."""
import os
import subprocess

import numpy as np
import pytest

import oracle as O
import ref_numpy as R
from _common import BLOCKS_EUR1, ROOT, TD, blockwise, pcg_case
from test_variance import TOL, _colwise, synth_oracle

DEVS = [0, 0, 0]
F3 = (0.8, 1.0, 1.2)
BAR = 1e-10
N_OBS, SIGMA = 100000, 0.5 / 1e6
MONO, EMPTY = 1, 5                    # the monomorphic variant's block; PCG_SIZES' empty block
VARIANTS = {"plain": {}, "lmm": dict(lmm=True), "miss": dict(miss_block=2), "mono": dict(mono_block=MONO),
            "nref301": dict(n_ref=301)}


def _sig(prob, factors=F3):
    return [prob.sigma_s * f for f in factors]


def _route(plan, want):
    got = plan.workload()["pcg_route"]
    assert got == want, (got, want)


def _same(a, b):
    """(beta_s, beta_l, status) triples, or lists of them: equal bit for bit, NaNs included"""
    if isinstance(a, list):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            _same(x, y)
        return
    for u, v in zip(a, b):
        np.testing.assert_array_equal(u, v)


_ORACLE = {}


def _oracle(name, prob, sigma):
    """The oracle's direct fp64 solve at sigma, computed once per (problem name, sigma)."""
    key = (name, float(sigma), float(prob.tau))
    if key not in _ORACLE:
        O.use_blas(True)
        bs, bl, _, _ = O.est(prob.bed, prob.n_ref, prob.n_obs, sigma, prob.s_ptr, prob.s_pos, prob.z_s,
                             prob.l_ptr, prob.l_pos, prob.z_l, tau=prob.tau, method="direct", threads=8)
        _ORACLE[key] = (bs, bl)
    return _ORACLE[key]


def _m(prob):
    return np.diff(prob.s_ptr) + (np.diff(prob.l_ptr) if prob.l_ptr is not None else 0)


def _status_ok(prob, st, mono=None):
    from dbslmm_amd import BLOCK_EMPTY, BLOCK_MONOMORPHIC, BLOCK_OK
    want = np.where(_m(prob) > 0, BLOCK_OK, BLOCK_EMPTY)
    if mono is not None:
        want[mono] = BLOCK_MONOMORPHIC
    np.testing.assert_array_equal(st, want)


# ------------------------------------------------------------------ CPU: the builder and the rule
def test_shared_problem_has_the_flagship_shift_and_every_block_kind():
    """d = 20 exactly as the flagship configurations; one block of each kind; the variants touch
    only what they name."""
    c = pcg_case()
    p = c.prob
    assert 1.0 / (p.sigma_s * p.n_obs) == pytest.approx(20.0, rel=1e-15) and "solver" not in p.opts
    m, ml = _m(p), np.diff(p.l_ptr)
    assert m.tolist() == [70, 600, 200, 1030, 1100, 0, 40] and ml.tolist() == [0, 0, 2, 0, 3, 0, 0]
    assert m[3] > 1024 and m[4] > 1024 and 0 < m[6] < 64 and m[EMPTY] == 0
    assert c.ts_pos.size == p.n_s and c.tl_pos.size == p.n_l and 0 < c.ind.sum() < c.ind.size
    q = pcg_case(lmm=True).prob
    assert q.l_ptr is None and q.n_s == p.n_s + p.n_l
    assert pcg_case(n_ref=301).prob.n_ref % 4 == 1
    a, b = pcg_case(miss_block=2).prob.bed, p.bed
    assert np.count_nonzero(a != b) == 1
    z = pcg_case(zero_blocks=(0, 2)).prob
    assert np.all(z.z_s[z.s_ptr[0]:z.s_ptr[1]] == 0) and np.all(z.z_l[z.l_ptr[2]:z.l_ptr[3]] == 0)
    assert np.all(z.z_s[z.s_ptr[1]:z.s_ptr[2]] != 0)


FIVE = (0.6, 0.8, 1.0, 1.2, 1.4)      # more copies than pcg::kMaxNC = 4


def five_copies_case():
    """5 copies under solver = 2 with the default h2f mode (rule_cases' problem): the
    factorisation route, whose copies other than the base iterate on the base copy's factor."""
    prob = pcg_case(sizes=(70, 300, 200, 1030, 0, 40), n_large=(0, 0, 2, 1, 0, 0), solver=2).prob
    return prob, [SIGMA * f for f in FIVE]


def rule_cases():
    """(name, problem, sigmas, expected pcg_route) at the edges of the route rule (pcg_route in
    route_pcg.hip, problem_pcg_route in multi.hip).  d = 1 / (sigma n) is exactly 2.0 in fp64 at
    n = 2^16, sigma = 2^-17 (both powers of two: the product 0.5 and its reciprocal are exact);
    the next fp64 sigma gives d = 2 - 2^-51 < 2.  The 5-copy case here factors every copy
    (h2f_mode = 1, the CLI's --h2f-merged); the default h2f mode is five_copies_case."""
    n2 = 65536
    s2 = 1.0 / (2.0 * n2)
    assert 1.0 / (s2 * n2) == 2.0 and 1.0 / (np.nextafter(s2, 1.0) * n2) < 2.0
    mk = lambda **kw: pcg_case(sizes=(70, 300, 200, 1030, 0, 40), n_large=(0, 0, 2, 1, 0, 0), **kw).prob
    lm = lambda **kw: pcg_case(sizes=(70, 300, 200, 1030, 0, 40), n_large=(0,) * 6, lmm=True, **kw).prob
    return [
        ("d2", mk(n_obs=n2, sigma_s=s2), [s2], 1),
        ("d2_next", mk(n_obs=n2, sigma_s=float(np.nextafter(s2, 1.0))), [float(np.nextafter(s2, 1.0))], 0),
        ("five_copies_forced_merged", mk(solver=2, h2f_mode=1), [SIGMA * f for f in FIVE], 0),
        ("four_copies", mk(), [SIGMA * f for f in (0.6, 0.8, 1.0, 1.2)], 1),
        ("tau1_large_forced", mk(tau=1.0, solver=2), [SIGMA], 0),
        ("tau1_large_auto", mk(tau=1.0), [SIGMA], 0),
        ("tau1_lmm", lm(tau=1.0), [SIGMA], 1),
        ("one_copy_below_merged", mk(h2f_mode=1), [SIGMA, SIGMA * 11.0], 0),
    ]


def check_shard_rule(prob, sigmas, route, world=3):
    """dist.shard_units_problem decides as the plan does: on the factorisation route its plan is
    shard_units' (the factorisation model), on the PCG route every block sits whole on one device,
    placed by the PCG model -- for these problems another placement than the factorisation
    model's."""
    from dbslmm_amd.dist import shard_units, shard_units_problem
    m = _m(prob)
    ud, ms = shard_units_problem(prob, sigmas, world)
    fd, fms = shard_units(m, prob.n_ref, world, len(sigmas))
    assert ud.shape == (prob.num_block, len(sigmas)) and np.all((ud >= 0) == (m > 0)[:, None])
    if route == 0:
        np.testing.assert_array_equal(ud, fd)
        np.testing.assert_array_equal(ms, fms)
    else:
        assert np.all(ud == ud[:, :1])
        assert not np.array_equal(ms, fms)           # the PCG model's step, not the factorisation's
    return ud


def test_shard_plan_follows_the_route_rule_at_its_edges():
    """Host only: d exactly 2 (PCG), the next fp64 sigma (factorisation), more than kMaxNC = 4
    copies under solver = 2, tau = 1 with and without large SNPs, one copy of several below the
    threshold.  On _split_problem at three copies the factorisation model splits the dominant
    block by copy and the PCG model keeps it whole, so the two decisions show in the plan."""
    from test_dist import _split_problem
    for name, prob, sig, route in rule_cases():
        check_shard_rule(prob, sig, route)
    check_shard_rule(*five_copies_case(), 0)
    prob, m = _split_problem()
    lo = check_shard_rule(prob, _sig(prob), 0)
    assert len(set(lo[1].tolist())) == 3
    hi = check_shard_rule(prob, [SIGMA * f for f in F3], 1)
    assert len(set(hi[1].tolist())) == 1


# ------------------------------------------------------------------ 1. sharded = one device
@pytest.mark.gpu
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_sharded_pcg_equals_one_device_bit_for_bit(variant):
    """Context([0, 0, 0]) against Context(0): DBSLMMFIT.est, run() + sync() + download(), and
    run_multi of 1, 3 and 4 copies twice in a row -- betas and statuses equal, the NaNs of the
    monomorphic block included.  Every device gets blocks, shard_info() is column 0 of
    shard_units_problem's plan and every block sits whole on one device (a
    block's path depends on the block and the number of copies alone)."""
    from dbslmm_amd import DBSLMMFIT, Context, Plan
    from dbslmm_amd.dist import shard_units_problem
    prob = pcg_case(**VARIANTS[variant]).prob
    mono = MONO if variant == "mono" else None
    m = _m(prob)
    one, many = Plan(Context(0), prob), Plan(Context(DEVS), prob)
    info = many.shard_info()
    ud, _ = shard_units_problem(prob, [prob.sigma_s], 3)
    np.testing.assert_array_equal(info, ud[:, 0])
    assert np.all((info == -1) == (m == 0)) and set(info[m > 0].tolist()) == {0, 1, 2}
    ud3, _ = shard_units_problem(prob, _sig(prob), 3)
    assert np.all(ud3 == ud3[:, :1])
    e1, e3 = DBSLMMFIT(0).est(prob), DBSLMMFIT(DEVS).est(prob)
    _same(e1, e3)
    for p in (one, many):
        p.run()
        p.sync()
        _route(p, 1)
    d1 = one.download()
    _same(d1, many.download())
    _same(d1, e1)
    _status_ok(prob, d1[2], mono)
    if mono is not None:
        assert np.all(np.isnan(d1[0][prob.s_ptr[mono]:prob.s_ptr[mono + 1]]))
        assert np.isfinite(d1[0]).sum() == prob.n_s - (prob.s_ptr[mono + 1] - prob.s_ptr[mono])
    else:
        assert np.all(np.isfinite(d1[0])) and np.all(np.isfinite(d1[1]))
    for factors in ((1.0,), F3, (0.5, 0.8, 1.0, 1.3)):
        sig = _sig(prob, factors)
        ref = one.run_multi(sig)
        _route(one, 1)
        for _ in range(2):
            _same(many.run_multi(sig), ref)
            _route(many, 1)
        _same(one.run_multi(sig), ref)
        for r in ref:
            _status_ok(prob, r[2], mono)
    one.close()
    many.close()


# ------------------------------------------------------------------ 2. units plans
@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["plain", "mono"])
def test_units_plans_on_the_pcg_route_fill_the_one_device_result(variant):
    """The torchrun ranks' path: one units plan per device index of shard_units_problem's
    three-device plan, each filling its units of shared arrays; together bit for bit the
    one-device result (statuses of the blocks with SNPs: a units plan leaves the others alone)."""
    from dbslmm_amd import Context, Plan
    from dbslmm_amd.dist import shard_units_problem
    prob = pcg_case(**VARIANTS[variant]).prob
    sig = _sig(prob)
    ud, _ = shard_units_problem(prob, sig, 3)
    assert np.all(ud == ud[:, :1]) and set(ud[_m(prob) > 0, 0].tolist()) == {0, 1, 2}
    one = Plan(Context(0), prob)
    ref = one.run_multi(sig)
    _route(one, 1)
    bs, bl = np.full((3, prob.n_s), -7.25), np.full((3, prob.n_l), -7.25)
    st = np.full((3, prob.num_block), -99, dtype=np.int32)
    ctx = Context(0)
    for d in range(3):
        u = Plan.units(ctx, prob, ud, d)
        u.run_multi(sig, out=(bs, bl, st))
        _route(u, 1)
        u.close()
    full = _m(prob) > 0
    for c in range(3):
        np.testing.assert_array_equal(bs[c], ref[c][0])
        np.testing.assert_array_equal(bl[c], ref[c][1])
        np.testing.assert_array_equal(st[c][full], ref[c][2][full])
    one.close()


# ------------------------------------------------------------------ 3. more devices than blocks
@pytest.mark.gpu
def test_more_devices_than_blocks_on_the_pcg_route():
    """One block, Context([0, 0]): the idle device stays harmless; identical to one device."""
    from dbslmm_amd import DBSLMMFIT, Context, Plan
    prob = pcg_case(sizes=(300,), n_large=(2,)).prob
    _same(DBSLMMFIT(0).est(prob), DBSLMMFIT([0, 0]).est(prob))
    one, two = Plan(Context(0), prob), Plan(Context([0, 0]), prob)
    sig = _sig(prob)
    ref = one.run_multi(sig)
    _same(two.run_multi(sig), ref)
    _route(one, 1)
    _route(two, 1)
    assert sorted(two.shard_info().tolist()) == [0]
    rs, rl = _oracle("one_block", prob, sig[-1])
    assert blockwise(prob, ref[-1][:2], (rs, rl)) <= BAR
    one.close()
    two.close()


# ------------------------------------------------------------------ 4. copy-split units on PCG
@pytest.mark.gpu
def test_copy_split_units_run_on_the_pcg_route():
    """shard_copies = 3 at a sigma_s on the factorisation route (test_dist._split_problem: the
    1600-SNP block's copies go to three devices), then run_multi with three sigmas of d >= 2: the
    route is decided per run, so every job iterates.  The whole blocks equal the one-device run of
    the same sigmas bit for bit.  The split block is solved copy by copy (one Krylov sequence
    each) where one device runs its copies together, so its copies are held to the parity bar
    against the oracle's direct solve, with the one-device statuses; the difference from the
    one-device run is printed (measured: see DESIGN.md section 4)."""
    from test_dist import _split_problem
    from dbslmm_amd import Context, Plan
    prob, m = _split_problem()
    assert 1.0 / (prob.sigma_s * prob.n_obs) < 2.0
    sig = [SIGMA * f for f in F3]
    assert all(1.0 / (s * prob.n_obs) >= 2.0 for s in sig)
    one = Plan(Context(0), prob)
    single = one.run_multi(sig)
    _route(one, 1)
    prob.opts["shard_copies"] = 3
    many = Plan(Context(DEVS), prob)
    got = many.run_multi(sig)
    _route(many, 1)
    sl, ll = np.r_[prob.s_ptr[1]:prob.s_ptr[2]], np.r_[prob.l_ptr[1]:prob.l_ptr[2]]
    keep_s, keep_l = np.setdiff1d(np.arange(prob.n_s), sl), np.setdiff1d(np.arange(prob.n_l), ll)
    for c in range(3):
        np.testing.assert_array_equal(got[c][0][keep_s], single[c][0][keep_s])
        np.testing.assert_array_equal(got[c][1][keep_l], single[c][1][keep_l])
        np.testing.assert_array_equal(got[c][2], single[c][2])
        assert np.all(got[c][2][m > 0] == 0)
        g = np.concatenate([got[c][0][sl], got[c][1][ll]])
        o = np.concatenate([single[c][0][sl], single[c][1][ll]])
        print(f"split block, copy {c}: |units - one device| / max = {np.max(np.abs(g - o)) / np.max(np.abs(o)):.3e}")
        rs, rl = _oracle("split", prob, sig[c])
        e_units, e_one = blockwise(prob, got[c][:2], (rs, rl)), blockwise(prob, single[c][:2], (rs, rl))
        print(f"copy {c}: worst block vs oracle: units {e_units:.3e}, one device {e_one:.3e}")
        assert e_units <= BAR and e_one <= BAR, (c, e_units, e_one)
    _same(many.run_multi(sig), got)                      # and again: the same bits
    one.close()
    many.close()


# ------------------------------------------------------------------ 5. variance after a PCG run
_VAR_ORACLE = {}


def _var_oracle(name, c, sigma):
    key = (name, float(sigma))
    if key not in _VAR_ORACLE:
        _VAR_ORACLE[key] = synth_oracle(c.prob, c.tbed, c.ind, c.ts_pos, c.tl_pos, sigma=sigma)
    return _VAR_ORACLE[key]


def _variance(plan, c):
    return plan.variance(c.tbed, c.ind, c.ts_pos, c.tl_pos)


@pytest.mark.gpu
@pytest.mark.parametrize("start", ["run", "multi3"])
@pytest.mark.parametrize("variant", ["plain", "mono"])
def test_variance_after_a_pcg_run_resolves_by_factorisation(variant, start):
    """A PCG run leaves no factor, so variance() first re-solves the last sigma on the
    factorisation route (variance_factor: pcg_pending_var, force_factor).  From run() + sync() and
    from a run_multi whose last sigma is neither the largest nor the smallest: (a) within TOL of
    the literal formulas at the last sigma, (b) bit for bit the variance of a fresh solver = 1 plan
    at that sigma (the re-solve is that route's run), (c) the monomorphic block's column NaN,
    (d) the empty block's column 0, (e) download() afterwards gives the last sigma's betas (the
    re-solve's: within the parity bar of the oracle, the statuses the PCG run reported), (f) a
    second variance() returns the same array and re-solves nothing."""
    from dbslmm_amd import Context, Plan
    c = pcg_case(**VARIANTS[variant])
    prob = c.prob
    mono = MONO if variant == "mono" else None
    plan = Plan(Context(0), prob)
    if start == "run":
        plan.run()
        plan.sync()
        last = prob.sigma_s
        st_pcg = plan.download()[2]
    else:
        sig = _sig(prob, (0.8, 1.2, 1.0))
        st_pcg = plan.run_multi(sig)[-1][2]
        last = sig[-1]
    _route(plan, 1)
    runs = plan.workload()
    got = _variance(plan, c)
    _route(plan, 0)                                      # the re-solve was the latest run
    ref = _var_oracle(variant, c, last)
    keep = [b for b in range(prob.num_block) if b != mono]
    assert got.shape == ref.shape and np.all(np.isfinite(got[:, keep]))
    err = _colwise(got[:, keep], ref[:, keep])
    print(f"variance after PCG ({variant}, {start}): worst column error {err:.3e}")
    assert err < TOL                                                             # (a)
    if mono is not None:
        assert np.all(np.isnan(got[:, mono]))                                    # (c)
    assert np.all(got[:, EMPTY] == 0)                                            # (d)
    after = plan.download()                                                      # (e)
    rs, rl = _oracle(variant, prob, last)
    skip = () if mono is None else (mono,)
    e = blockwise(prob, after[:2], (rs, rl), skip=skip)
    assert e <= BAR, e
    np.testing.assert_array_equal(after[2], st_pcg)
    _status_ok(prob, after[2], mono)
    again = _variance(plan, c)                                                   # (f)
    np.testing.assert_array_equal(again, got)
    _route(plan, 0)
    _same(plan.download(), after)
    plan.close()
    fresh = pcg_case(sigma_s=last, solver=1, **VARIANTS[variant])                # (b)
    fp = Plan(Context(0), fresh.prob)
    fp.run()
    fp.sync()
    _route(fp, 0)
    np.testing.assert_array_equal(_variance(fp, fresh), got)
    _same(fp.download(), after)
    fp.close()
    assert runs["pcg_route"] == 1


# ------------------------------------------------------------------ 6. sharded variance after PCG
@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["plain", "miss"])
def test_sharded_variance_after_pcg_matches_one_device(variant):
    """run_multi on the PCG route, then variance, on the device lists 0, [0, 0] and [0, 0, 0]:
    every shard re-solves its last sigma by factorisation before any shard's variance starts
    (mp_variance); the variance arrays and the betas are equal bit for bit across the lists, and
    the variance is within TOL of the literal formulas."""
    from dbslmm_amd import Context, Plan
    c = pcg_case(**VARIANTS[variant])
    prob = c.prob
    sig = _sig(prob)
    out, betas = [], []
    for dev in (0, [0, 0], [0, 0, 0]):
        plan = Plan(Context(dev), prob)
        betas.append(plan.run_multi(sig))
        _route(plan, 1)
        out.append(_variance(plan, c))
        out.append(_variance(plan, c))                   # (a second call: nothing pending any more)
        plan.close()
    for o in out[1:]:
        np.testing.assert_array_equal(out[0], o)
    for b in betas[1:]:
        _same(betas[0], b)
    err = _colwise(out[0], _var_oracle(variant, c, sig[-1]))
    print(f"sharded variance after PCG ({variant}): worst column error {err:.3e}")
    assert err < TOL


# ------------------------------------------------------------------ 7. route changes on one plan
def _fresh(prob, call):
    from dbslmm_amd import Context, Plan
    plan = Plan(Context(0), prob)
    out = call(plan)
    plan.close()
    return out


def _run_dl(plan):
    plan.run()
    plan.sync()
    return plan.download()


@pytest.mark.gpu
def test_route_alternates_pcg_factorisation_pcg():
    """What h2f tuning does when its sigmas cross the threshold: PCG run_multi(3), set_sigma to
    d = 0.5 and run() (factorisation), PCG run_multi(3) again -- each the bits of the same call on
    a fresh plan."""
    from dbslmm_amd import Context, Plan
    prob = pcg_case().prob
    sig = _sig(prob)
    low = 1.0 / (0.5 * prob.n_obs)
    ref3 = _fresh(prob, lambda p: p.run_multi(sig))

    def low_run(p):
        p.set_sigma(low)
        return _run_dl(p)
    ref_low = _fresh(prob, low_run)
    plan = Plan(Context(0), prob)
    _same(plan.run_multi(sig), ref3)
    _route(plan, 1)
    _same(low_run(plan), ref_low)
    _route(plan, 0)
    _same(plan.run_multi(sig), ref3)
    _route(plan, 1)
    rs, rl = _oracle("plain", prob, low)
    assert blockwise(prob, ref_low[:2], (rs, rl)) <= BAR
    plan.close()


@pytest.mark.gpu
def test_route_sequence_with_variance_and_copy_counts():
    """On the missing-call variant (its flags are read once, after the plan's first PCG run):
    PCG run_multi(3), variance(), PCG run_multi(3), PCG run_multi(1), run_multi of 5 copies (more
    than kMaxNC: the factorisation), PCG run_multi(3) -- each call the bits of the same call on a
    fresh plan."""
    from dbslmm_amd import Context, Plan
    c = pcg_case(miss_block=2)
    prob = c.prob
    s3, s1 = _sig(prob), _sig(prob, (1.1,))
    s5 = _sig(prob, (0.6, 0.8, 1.0, 1.2, 1.4))
    ref3 = _fresh(prob, lambda p: p.run_multi(s3))
    ref1 = _fresh(prob, lambda p: p.run_multi(s1))
    ref5 = _fresh(prob, lambda p: p.run_multi(s5))
    refv = _fresh(prob, lambda p: (p.run_multi(s3), _variance(p, c))[1])
    plan = Plan(Context(0), prob)
    for call, ref, route in ((s3, ref3, 1), (None, refv, 0), (s3, ref3, 1), (s1, ref1, 1), (s5, ref5, 0),
                             (s3, ref3, 1)):
        if call is None:
            np.testing.assert_array_equal(_variance(plan, c), ref)
        else:
            _same(plan.run_multi(call), ref)
        _route(plan, route)
    _same([plan.download()], ref3[-1:])
    plan.close()
    for k, s in enumerate(s5):     # the 5-copy run is right, not only repeatable (its h2f copies: pcg_tol)
        assert blockwise(prob, ref5[k][:2], _oracle("miss", prob, s)) <= BAR, k
    for k, s in enumerate(s3):
        assert blockwise(prob, ref3[k][:2], _oracle("miss", prob, s)) <= BAR, k


@pytest.mark.gpu
def test_one_plan_takes_every_reallocation_path():
    """One plan's life through every place that frees and re-allocates its device buffers: PCG
    run_multi(3) (pcg_layout), PCG run_multi(2) (pcg_layout rebuilt for another copy count),
    run_multi of 5 copies (the factorisation: ensure_copies grows the per-copy buffers and the block
    matrices, the first merged work list and Chebyshev coefficients), run_multi of 6 copies (the
    merged work list replaced, a longer coefficient vector: one more copy group), variance(),
    close() -- each call the bits of the same call on a fresh plan."""
    from dbslmm_amd import Context, Plan
    c = pcg_case()
    prob = c.prob
    s3, s2 = _sig(prob), _sig(prob, (0.9, 1.1))
    s5, s6 = _sig(prob, FIVE), _sig(prob, FIVE + (1.6,))
    cheb = {}

    def multi(sig):
        def call(p):
            out = p.run_multi(sig)
            cheb[len(sig)] = p.workload()
            return out
        return call
    refs = [_fresh(prob, multi(s)) for s in (s3, s2, s5, s6)]
    refv = _fresh(prob, lambda p: (p.run_multi(s6), _variance(p, c))[1])
    # the fresh runs took the paths this test is about: both many-copy runs iterate their other
    # copies on the base copy's factor, the second with more copy groups (a longer coefficient vector)
    assert cheb[5]["cheb_base"] >= 0 and cheb[6]["cheb_base"] >= 0
    assert 0 < cheb[5]["cheb_iters"] < cheb[6]["cheb_iters"], (cheb[5]["cheb_iters"], cheb[6]["cheb_iters"])
    plan = Plan(Context(0), prob)
    for sig, ref, route in zip((s3, s2, s5, s6), refs, (1, 1, 0, 0)):
        _same(plan.run_multi(sig), ref)
        _route(plan, route)
        assert plan.workload()["cheb_iters"] == cheb[len(sig)]["cheb_iters"]
    np.testing.assert_array_equal(_variance(plan, c), refv)
    plan.close()


@pytest.mark.gpu
def test_runs_without_sync_and_queries_on_a_pending_run():
    """A PCG run stays pending until something waits for it: run() twice without sync() and then
    download(); run() then variance(); run() then block_iters() -- each the result of the
    synchronised sequence on a fresh plan.  With timing on, a PCG run and a factorisation run
    before one sync() are reported as 2 runs with finite non-negative spans."""
    from dbslmm_amd import Context, Plan
    c = pcg_case()
    prob = c.prob
    ref = _fresh(prob, _run_dl)
    refv = _fresh(prob, lambda p: (_run_dl(p), _variance(p, c))[1])
    refi = _fresh(prob, lambda p: (_run_dl(p), p.block_iters())[1])
    assert np.all((refi > 0) == (_m(prob) > 0))
    ctx = Context(0)
    plan = Plan(ctx, prob)
    plan.run()
    plan.run()
    _same(plan.download(), ref)
    _route(plan, 1)
    plan.close()
    plan = Plan(ctx, prob)
    plan.run()
    np.testing.assert_array_equal(_variance(plan, c), refv)
    _route(plan, 0)
    plan.close()
    plan = Plan(ctx, prob)
    plan.run()
    np.testing.assert_array_equal(plan.block_iters(), refi)
    _route(plan, 1)
    _same(plan.download(), ref)
    # timing across the two routes
    plan.enable_timing(True)
    plan.run()
    plan.set_sigma(1.0 / (0.5 * prob.n_obs))
    plan.run()
    plan.sync()
    _route(plan, 0)
    ms, n = plan.kernel_ms()
    assert n == 2 and np.all(np.isfinite(ms)) and np.all(ms >= 0) and ms.sum() > 0, (n, ms)
    plan.close()


# ------------------------------------------------------------------ 8. the CLI's production route
CLI = os.path.join(ROOT, "dbslmm_amd", "bin", "dbslmm")
CLI_N, CLI_NSNP, CLI_H = 100000, 1000000, 0.5


def _cli(args, cwd):
    return subprocess.run([CLI] + args, capture_output=True, text=True, cwd=str(cwd), timeout=300)


def _cli_panel(tmp_path):
    """A one-chromosome synth.write_plink panel with large SNPs, its host-side oracle rows and
    the block of every output row (large rows first, then small, as the writer)."""
    from dbslmm_amd import synth
    from test_cli import _oracle_host
    panel = synth.simulate(4000, 300, pop="EUR", chroms=[1], seed=11, large_every=4)
    f = synth.write_plink(panel, str(tmp_path / "p"))
    bim = R.read_bim(f["ref"], panel.n_ref, True)
    blocks, _, _, info_s, info_l, _ = _oracle_host(f, bim, 0.2)
    assert len(info_l) >= 3 and len(info_s) > 3000
    base = ["-s", f["s"], "-l", f["l"], "-r", f["ref"], "-b", f["b"], "-n", str(CLI_N), "-nsnp", str(CLI_NSNP),
            "-mafMax", "0.2", "--precise-out"]
    row_block = np.array([e["block"] for e in info_l + info_s])
    return panel, base, len(blocks), info_s, info_l, row_block


def _rows(path):
    rows = [x.split() for x in open(path).read().splitlines() if x.strip()]
    return [(x[0], x[1], x[4]) for x in rows], np.array([float(x[2]) for x in rows])


def _rows_blockwise(got, ref, row_block):
    worst = 0.0
    for b in np.unique(row_block):
        k = row_block == b
        err = float(np.max(np.abs(got[k] - ref[k])) / np.max(np.abs(ref[k])))
        assert np.isfinite(err), b
        worst = max(worst, err)
    return worst


def _assert_cli_shift(h=CLI_H, factors=(1.0,)):
    for f in factors:
        assert CLI_NSNP / (h * f * CLI_N) >= 2.0         # d = 1 / (sigma_s n), sigma_s = h f / nsnp


@pytest.mark.gpu
def test_cli_production_route_matches_oracle_and_its_shards(tmp_path):
    """dbslmm with -n 100000 -nsnp 1000000 -h 0.5 (d = 20: the auto rule's PCG route, asserted
    through a Python plan of the same sigma, n_obs and tau): --precise-out rows in the oracle's
    order with its SNP / allele / flag columns, betas within the parity bar per LD block of
    R.est(..., method="chol") at 0.5 / 1e6; --gpu-ids 0,0,0 writes the same file byte for byte."""
    from dbslmm_amd import Context, Plan, synth
    _assert_cli_shift()
    panel, base, nb, info_s, info_l, row_block = _cli_panel(tmp_path)
    prob = synth.make_problem(panel)
    prob.n_obs, prob.sigma_s = CLI_N, CLI_H / CLI_NSNP
    assert prob.tau == 0.8
    plan = Plan(Context(0), prob)
    plan.run()
    plan.sync()
    _route(plan, 1)
    plan.close()
    res = R.est(panel.bed, panel.n_ref, CLI_N, CLI_H / CLI_NSNP, nb, info_s, info_l, tau=0.8, method="chol")
    exp = [x.split() for x in R.format_eff(res)]
    outs = []
    for extra, name in (([], "one"), (["--gpu-ids", "0,0,0"], "three")):
        eff = str(tmp_path / name)
        r = _cli(base + ["-h", str(CLI_H), "-eff", eff] + extra, tmp_path)
        assert r.returncode == 0, r.stderr
        outs.append(open(eff + ".txt").read())
    assert "Sharding the LD blocks over 3 GPUs" in r.stdout
    assert outs[0] == outs[1]
    keys, got = _rows(str(tmp_path / "one.txt"))
    assert keys == [(x[0], x[1], x[4]) for x in exp] and len(keys) == len(info_s) + len(info_l)
    err = _rows_blockwise(got, np.concatenate([res.beta_l, res.beta_s]), row_block)
    print(f"CLI on the PCG route: worst block vs oracle {err:.3e}")
    assert err <= BAR


@pytest.mark.gpu
def test_cli_h2f_on_the_production_route_matches_separate_runs(tmp_path):
    """-h2f 0.8,1,1.2 at d >= 2 for every factor: each output has the rows of a separate run at
    that h, its betas within the parity bar per LD block (one multi-shift sequence serves the
    copies of a block without large SNPs, so the bits may differ from a one-copy run)."""
    factors = ("0.8", "1", "1.2")
    _assert_cli_shift(factors=[float(x) for x in factors])
    _, base, _, _, _, row_block = _cli_panel(tmp_path)
    prefix = str(tmp_path / "chr1")
    r = _cli(base + ["-h", str(CLI_H), "-h2f", ",".join(factors), "-eff", prefix + ".dbslmm"], tmp_path)
    assert r.returncode == 0, r.stderr
    for hh in factors:
        single = str(tmp_path / f"single{hh}")
        r = _cli(base + ["-h", repr(CLI_H * float(hh)), "-eff", single], tmp_path)
        assert r.returncode == 0, r.stderr
        kt, vt = _rows(f"{prefix}_h2f{hh}.dbslmm.txt")
        kr, vr = _rows(single + ".txt")
        assert kt == kr
        err = _rows_blockwise(vt, vr, row_block)
        print(f"CLI -h2f {hh} vs a separate run: worst block {err:.3e}")
        assert err <= BAR, hh


@pytest.mark.gpu
def test_cli_variance_on_the_production_route(tmp_path):
    """-dat_str / -test_indicator_file after a solve at d = 20 on test_dat (the helpers of
    test_variance.test_cli_writes_variance_txt): run_multi streams the PCG results out, then
    dbslmm_plan_variance re-solves by factorisation.  variance.txt within 1e-8 per column of the
    restatement, and identical between one GPU and --gpu-ids 0,0."""
    from test_cli import REF, SUMM, split_summary
    from test_variance import read_arma_ascii, td_oracle, td_variance_problem
    _assert_cli_shift()
    v = td_variance_problem(False, drop_test_mono=True, nsnp=CLI_NSNP)
    v["n_obs"] = CLI_N
    assert v["sigma"] == CLI_H / CLI_NSNP
    D = td_oracle(v)
    summ = str(tmp_path / "summ.txt")
    with open(SUMM) as f, open(summ, "w") as o:
        for line in f:
            if line.split("\t")[1] not in v["dropped"]:
                o.write(line)
    s, l = split_summary(tmp_path, summ)
    ind = str(tmp_path / "ind.txt")
    open(ind, "w").write("".join(f"{x}\n" for x in v["ind"]))
    outs = []
    for name, extra in (("one", []), ("two", ["--gpu-ids", "0,0"])):
        d = tmp_path / name
        d.mkdir()
        r = _cli(["-s", s, "-l", l, "-r", REF, "-b", BLOCKS_EUR1, "-n", str(CLI_N), "-nsnp", str(CLI_NSNP), "-h",
                  str(CLI_H), "-mafMax", "0.2", "-eff", str(d / "o"), "-dat_str", os.path.join(TD, "test_chr1"),
                  "-test_indicator_file", ind] + extra, d)
        assert r.returncode == 0, r.stderr
        outs.append([open(d / x).read() for x in ("variance.txt", "o.txt")])
    assert outs[0] == outs[1]
    got = read_arma_ascii(str(tmp_path / "one" / "variance.txt"))
    assert got.shape == D.shape and np.array_equal(np.isnan(got), np.isnan(D))
    fin = np.isfinite(D)
    assert fin.any()
    err = _colwise(np.where(fin, got, 0.0), np.where(fin, D, 0.0))
    print(f"CLI variance.txt after the PCG solve: worst column error {err:.3e}")
    assert err < TOL
