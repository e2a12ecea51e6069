"""The h2f iterations on the base copy's factor, per block and at their route edges
(dbslmm_chol_cheb; dbslmm_cheb_init / dbslmm_trsv_fwd / dbslmm_trsv_bwd / dbslmm_cg_update and the
fused dbslmm_trsv_cheb; dbslmm_tcheb; the host-side cheb_plan: DESIGN.md 3.3 / 3.4).

One panel (n_ref = 1280, missing calls) with the blocks E_BLOCKS = (m, m_large): the one-wave /
one-workgroup hand-over (63 / 64: the Gram epilogue writes every copy at 63 and only the base copy
from 64), dbslmm_chol_cheb at its LDS limit (511, ld = 512), blocks whose update delta P_s is zero
(128, 128) or one coordinate (480, 479), the z row alone in its tile (64, 128), an empty block, and
tiled blocks of 8 - 9 tile rows beside the ones of 10 and 17 - 18.  d_b = 1 / (sigma n) = 0.1: the
auto rule stays on the factorisation route.

Reference: the oracle's direct solve of every sigma (Case.oracle), per block on the block's own
scale (blockwise).  Bars: 1e-10 for a factored copy (test_preconditions_from_the_reference_alone:
kappa(M_c) <= 250, so m eps kappa <= 3e-11), CHEB_TOL for an iterated copy, and at the wide
spectra 10 x CHEB_TOL (Chebyshev) / 2 x CHEB_TOL (CG), as test_h2f_cheb.py's
test_cheb_error_within_target / test_cg_error_within_target.

tau = 1 (test_tau_one_copies_are_ok): CG's stopping bound of a block with large SNPs is
cheb_tol (1 - tau) |x| = 0 there, so the block runs the whole a priori count; a copy that did is
within the target by that count's own bound and reports OK -- only a cap that pcg_maxit cut below
the count reports DBSLMM_BLOCK_NOT_CONVERGED (test_h2f_cheb.py::test_cg_cap_reports_not_converged).

A base factor that is not positive definite needs tau > 1 (test_chol_edges.py's docstring), where
cheb_plan declines and every copy is factored: test_not_pd_block_beside_iteration_panel checks that
route on this panel (status 2 and NaN in every copy, every other block untouched bit for bit).  A
failed base status inherited by ITERATED copies is test_h2f_cheb.py's monomorphic block (status 3).

Measured on the MI355X, worst per block: h2f 0.8 / 1 / 1.2 Chebyshev 2.7e-10, CG 6.4e-11, the base
copy 5.0e-14; base positions and groups 3.3e-10; wide spectra Chebyshev 2.8e-10 (bar 1e-8), CG
5.6e-10 (bar 2e-9); tau = 1 CG 2.1e-10, Chebyshev 4.2e-10; beside the NOT_PD block 2.1e-13
("h2f iterations per block", with the three defects this module found: the status 4
false alarm at tau = 1, a missing barrier in dbslmm_tcheb's start, cheb_plan's count without the 2
of its bound).
"""
import functools

import numpy as np
import pytest

from _common import CHEB_TOL, blockwise
from test_chol_edges import build_case, gpu_multi, gpu_run, same

E_NREF, E_MISS, E_SEED, E_SIGMA = 1280, 0.002, 11, 1e-4          # d_b = 1 / (1e-4 x 100000) = 0.1
E_BLOCKS = [(63, 1), (64, 1), (65, 0), (96, 2), (128, 128), (200, 0), (330, 3), (480, 479), (511, 2), (0, 0),
            (600, 2), (1030, 0), (1100, 3)]
E_SIZES = [m for m, _ in E_BLOCKS]
E_EMPTY = E_SIZES.index(0)
E_DUP_TAU, E_DUP_BLOCK, E_DUP = 1.05, E_BLOCKS.index((330, 3)), (328, 329)   # two of the three large SNPs
H2F = (0.8, 1.0, 1.2)
POSITIONS = [(1.0, 0.8, 1.2), (0.8, 1.2, 1.0), (1.2, 0.8), (0.7, 0.9, 1.1, 1.3), (1.0, 1.0, 1.0), (0.8, 1.0, 1.0)]
WIDE = [(0.05, 1.0), (1.0, 0.02)]        # cheb_plan's counts: 31 and 50
TOO_WIDE = (0.01, 1.0)                   # 72 > 60: the merged factorisation
KAPPA_MAX = 250.0


@functools.lru_cache(maxsize=None)
def case_e(tau=0.8, lmm=False, dup=False, emptied=False):
    blocks = [(m, ml, E_DUP if dup and b == E_DUP_BLOCK else None) for b, (m, ml) in enumerate(E_BLOCKS)]
    return build_case(blocks, n_ref=E_NREF, tau=tau, sigma_s=E_SIGMA, miss_rate=E_MISS, seed=E_SEED, lmm=lmm,
                      empty=(E_DUP_BLOCK,) if emptied else ())


def sigmas(factors):
    return [E_SIGMA * f for f in factors]


# every (case, h2f factor) the GPU tests below solve
USED = {
    "tau0.8": (dict(), sorted({f for t in [H2F] + POSITIONS + WIDE + [TOO_WIDE] for f in t})),
    "tau1": (dict(tau=1.0), sorted(H2F)),
    "tau1_lmm": (dict(tau=1.0, lmm=True), sorted(H2F)),
    "dup": (dict(tau=E_DUP_TAU, dup=True), sorted(H2F)),
}


# ----------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("name", list(USED))
def test_preconditions_from_the_reference_alone(name):
    """From the oracle and NumPy only, for every sigma the GPU tests use: the oracle's direct solve
    succeeds on every healthy block (and fails on the duplicated one alone), and kappa(M_c) <=
    KAPPA_MAX, from which the direct-solve bar 1e-10 per block follows (m eps kappa <= 1100 x
    1.1e-16 x 250 = 3e-11).  The tau = 1.05 case is held to m eps kappa < 1e-10 per block instead:
    its kappa exceeds KAPPA_MAX (see below)."""
    kw, factors = USED[name]
    c = case_e(**kw)
    assert [c.blocks[b][0] for b in c.keep] == [m for m in E_SIZES if m > 0]
    assert c.fail == ([E_DUP_BLOCK] if kw.get("dup") else [])
    worst, worst_bound = (0.0, None, None), 0.0
    for f in factors:
        sg = E_SIGMA * f
        st = c.oracle(sg)[2]
        assert np.flatnonzero(st != 0).tolist() == [b for b in c.keep if c.fails(b, sg)] == c.fail, (name, f, st)
        for b in c.healthy:
            ev = np.linalg.eigvalsh(c.joint(b, sg))
            assert ev[0] > 0.0, (name, f, c.blocks[b], ev[0])
            kappa = float(ev[-1] / ev[0])
            worst = max(worst, (kappa, c.blocks[b][:2], f))
            bound = c.blocks[b][0] * 2.0 ** -53 * kappa
            worst_bound = max(worst_bound, bound)
            if kw.get("dup"):
                # tau = 1.05 shifts every eigenvalue of the large SNPs' part down by 0.05: kappa reaches
                # 802 at (480, 479) and 746 at (1100, 3), above KAPPA_MAX, and the bar still follows
                # (m eps kappa <= 9.2e-11 at (1100, 3), h2f 1.2; 6.2e-11 for the base sigma)
                assert bound < 1e-10, (name, f, c.blocks[b], kappa, bound)
            else:
                assert kappa <= KAPPA_MAX, (name, f, c.blocks[b], kappa)
        if kw.get("dup"):      # indefinite by 1 - tau = -0.05 in every copy (test_chol_edges.py's docstring)
            assert c.kind(E_DUP_BLOCK) == "l"
            assert np.linalg.eigvalsh(c.joint(E_DUP_BLOCK, sg))[0] <= 1.0 - E_DUP_TAU + 1e-9
    print(f"{name}: worst kappa(M_c) {worst[0]:.1f} at block {worst[1]}, h2f factor {worst[2]}; "
          f"worst m eps kappa {worst_bound:.2e}")


def test_cases_share_rows_and_z():
    """Every variant is the same panel rows and z: the LMM-only case moves the large SNPs among the
    small ones, the emptied case drops one block from the CSR and keeps the others' rows."""
    a, l = case_e(tau=1.0), case_e(tau=1.0, lmm=True)
    assert l.prob.l_ptr is None and l.prob.n_s == a.prob.n_s + a.prob.n_l == sum(E_SIZES)
    assert E_EMPTY not in a.keep and len(a.keep) == len(E_BLOCKS) - 1
    np.testing.assert_array_equal(a.prob.bed, l.prob.bed)
    d, e = case_e(tau=E_DUP_TAU, dup=True), case_e(tau=E_DUP_TAU, dup=True, emptied=True)
    assert e.fail == [] and e.healthy == d.healthy
    for b in d.healthy:
        for x, y in ((d.prob.s_pos, e.prob.s_pos), (d.prob.z_s, e.prob.z_s)):
            np.testing.assert_array_equal(x[d.rows(b)[0]], y[e.rows(b)[0]])


def test_a_priori_counts_of_the_wide_cases():
    """cheb_plan's bound 2 q^K |ext| <= cheb_tol on [1, 1 + ext] widened by 1e-6 each way, ext =
    (d_c - d_b) / (d_b + 1 - tau): K = 31 and 50 iterate, 72 exceeds the limit of 60.  (Without the
    2 of the bound: 30, 48 and 70.)"""
    for (factors, want, without) in ((WIDE[0], 31, 30), (WIDE[1], 50, 48), (TOO_WIDE, 72, 70)):
        other = min(factors)
        ext = (0.1 / other - 0.1) / (0.1 + 1.0 - 0.8)
        kap = (1.0 + ext) * (1.0 + 1e-6) / (1.0 - 1e-6)
        q = (np.sqrt(kap) - 1.0) / (np.sqrt(kap) + 1.0)
        assert int(np.ceil(np.log(CHEB_TOL / (2.0 * ext)) / np.log(q))) == want, factors
        assert int(np.ceil(np.log(CHEB_TOL / ext) / np.log(q))) == without, factors
        assert (30 <= without <= want <= 60) == (factors != TOO_WIDE) and (factors != TOO_WIDE or without > 60)


# ----------------------------------------------------------------------------- GPU plumbing
DISPATCH = {
    "default": dict(),                                       # tiled from 384: 64 .. 330 on dbslmm_chol_cheb
    "single512": dict(tiled_min=512),                        # 480 and 511 on dbslmm_chol_cheb too
    "tiled64": dict(tiled_min=64),
    "whole": dict(tiled_min=64, lead_min=1000, sub_split=2),  # 1030, 1100 lead; the rest on dbslmm_tcheb
}
ITER = {"cheb": dict(h2f_iter=1), "cg": dict(h2f_iter=2), "fused": dict(h2f_iter=1, cheb_fused=1)}
ROUTES = [(d, i) for d in DISPATCH for i in ("cheb", "cg")] + [("tiled64", "fused")]
TWO = [(d, i) for d in ("default", "tiled64") for i in ("cheb", "cg")]


def _ids(routes):
    return [f"{d}-{i}" for d, i in routes]


def class_counts(c, dispatch):
    """(blocks_tiled, blocks_large) of the blocks case c keeps."""
    tmin = DISPATCH[dispatch].get("tiled_min", 384)      # (a block of >= 512 SNPs: the default stays 384)
    sizes = [c.blocks[b][0] for b in c.keep]
    n_tiled = sum(1 for m in sizes if m >= tmin)
    return n_tiled, sum(1 for m in sizes if m >= 64) - n_tiled


_RUNS, _FRESH = {}, {}


def multi_e(key, dispatch, it, factors, **opts):
    """run_multi of case_e(**key) on one route, once: (copies, workload)."""
    k = (tuple(sorted(key.items())), dispatch, it, tuple(factors), tuple(sorted(opts.items())))
    if k not in _RUNS:
        c = case_e(**key)
        o = dict(DISPATCH[dispatch], **opts)
        if it is not None:
            o.update(ITER[it])
        _RUNS[k] = gpu_multi(c.variant(**o), sigmas(factors))
        wl = _RUNS[k][1]
        assert wl["pcg_route"] == 0
        assert (wl["blocks_tiled"], wl["blocks_large"]) == class_counts(c, dispatch), (dispatch, wl)
    return _RUNS[k]


def fresh_e(key, dispatch, factor):
    """A single-sigma run on a fresh plan with the same dispatch, once.  solver = 1: the route
    run_multi took (alone, h2f 0.01 has d = 10 and the auto rule would solve it by PCG)."""
    k = (tuple(sorted(key.items())), dispatch, factor)
    if k not in _FRESH:
        _FRESH[k] = gpu_run(case_e(**key).variant(sigma_s=E_SIGMA * factor, solver=1, **DISPATCH[dispatch]))
        assert _FRESH[k][3]["pcg_route"] == 0
    return _FRESH[k]


def worst_block(c, res, ref):
    """(block, max-norm error, 2-norm error) of the block with the largest max-norm error, each
    relative to the block's reference."""
    out = (None, 0.0, 0.0)
    for b in c.healthy:
        g, r = c.of(res, b), c.of(ref, b)
        e = float(np.max(np.abs(g - r)) / np.max(np.abs(r)))
        if not e <= out[1]:
            out = (c.blocks[b][:2], e, float(np.linalg.norm(g - r) / np.linalg.norm(r)))
    return out


def expected(c):
    st = np.zeros(len(c.blocks), dtype=np.int32)
    st[[b for b in range(len(c.blocks)) if b not in c.keep]] = 1
    return st.tolist()


def check_copies(c, key, dispatch, factors, multi, wl, what, bar=CHEB_TOL, base_fresh=True):
    """The per-block bars of every copy against the oracle; the base copy (and every copy of the
    same sigma) at the direct solve's bar, the base copy bit for bit a fresh solve."""
    sig = sigmas(factors)
    base = int(np.argsort(sig, kind="stable")[len(sig) // 2])
    assert wl["cheb_base"] == base, (what, wl["cheb_base"])
    worst = 0.0
    for k, sg in enumerate(sig):
        assert multi[k][2].tolist() == expected(c), (what, k, multi[k][2])
        assert np.all(np.isfinite(multi[k][0])) and np.all(np.isfinite(multi[k][1])), (what, k)
        ref = c.oracle(sg)
        err = blockwise(c.prob, multi[k][:2], ref[:2])
        blk, e_max, e_2 = worst_block(c, multi[k], ref)
        print(f"{what} copy {k} (h2f {factors[k]}{', base' if k == base else ''}): worst block {blk} "
              f"max-norm {e_max:.3e}, 2-norm {e_2:.3e}")
        assert err < (1e-10 if sg == sig[base] else bar), (what, k, blk, err)
        if sg != sig[base]:
            worst = max(worst, err)
    if base_fresh:
        same(multi[base], fresh_e(key, dispatch, factors[base]), f"{what}: the base copy")
    return worst


# ----------------------------------------------------------------------------- GPU tests
@pytest.mark.gpu
@pytest.mark.parametrize("dispatch,it", ROUTES, ids=_ids(ROUTES))
def test_copies_per_block_against_direct_solve(dispatch, it):
    c = case_e()
    multi, wl = multi_e({}, dispatch, it, H2F)
    assert 0 < wl["cheb_iters"] <= 60
    worst = check_copies(c, {}, dispatch, H2F, multi, wl, f"{dispatch} {it}")
    print(f"{dispatch} {it}: iterated copies, worst per-block error {worst:.3e} ({wl['cheb_iters']} iterations)")


@pytest.mark.gpu
def test_whole_block_rest_group_iterates_by_chebyshev():
    """sub_split = 2: the rest group's copies come from dbslmm_tcheb whatever h2f_iter says (bit
    for bit the Chebyshev run's), the lead blocks' from the tile items (CG differs from Chebyshev
    in the last bits at least)."""
    c = case_e()
    cheb, cg = multi_e({}, "whole", "cheb", H2F)[0], multi_e({}, "whole", "cg", H2F)[0]
    lead = [b for b in c.keep if c.blocks[b][0] >= 1000]
    assert [c.blocks[b][0] for b in lead] == [1030, 1100]
    for k in (0, 2):
        for b in c.keep:
            if b not in lead:
                np.testing.assert_array_equal(c.of(cg[k], b), c.of(cheb[k], b), err_msg=f"copy {k} block {b}")
        assert any(not np.array_equal(c.of(cg[k], b), c.of(cheb[k], b)) for b in lead), k


@pytest.mark.gpu
@pytest.mark.parametrize("factors", POSITIONS, ids=[",".join(map(str, f)) for f in POSITIONS])
@pytest.mark.parametrize("dispatch,it", TWO, ids=_ids(TWO))
def test_base_position_and_groups(dispatch, it, factors):
    """The base copy first, last and in the middle of three, first of two, a 2 + 1 split of the
    copy groups (four copies), and copies of the base's own sigma (delta = 0: check_copies holds
    them to the direct solve's bar)."""
    c = case_e()
    multi, wl = multi_e({}, dispatch, it, factors)
    assert wl["cheb_iters"] > 0
    worst = check_copies(c, {}, dispatch, factors, multi, wl, f"{dispatch} {it} {factors}")
    print(f"{dispatch} {it} {factors}: base {int(wl['cheb_base'])}, worst per-block error of the iterated copies "
          f"{worst:.3e}")


@pytest.mark.gpu
@pytest.mark.parametrize("factors", WIDE, ids=[",".join(map(str, f)) for f in WIDE])
@pytest.mark.parametrize("dispatch,it", TWO, ids=_ids(TWO))
def test_wide_spectra_iterate_within_target(dispatch, it, factors):
    """Spectra of M_b^-1 M_c up to [1, 17.3]: 31 and 50 iterations by cheb_plan's formula."""
    c = case_e()
    multi, wl = multi_e({}, dispatch, it, factors)
    assert wl["cheb_base"] >= 0
    assert 30 <= wl["cheb_iters"] <= 60, wl["cheb_iters"]
    bar = 10 * CHEB_TOL if it == "cheb" else 2 * CHEB_TOL
    worst = check_copies(c, {}, dispatch, factors, multi, wl, f"{dispatch} {it} {factors}", bar=bar)
    print(f"{dispatch} {it} {factors}: {int(wl['cheb_iters'])} iterations, worst per-block error {worst:.3e} "
          f"(bar {bar:.0e})")


@pytest.mark.gpu
@pytest.mark.parametrize("dispatch,it", TWO, ids=_ids(TWO))
def test_too_wide_falls_back_to_factorisation(dispatch, it):
    multi, wl = multi_e({}, dispatch, it, TOO_WIDE)
    assert wl["cheb_base"] == -1 and wl["cheb_iters"] == 0
    c = case_e()
    for k, f in enumerate(TOO_WIDE):
        same(multi[k], fresh_e({}, dispatch, f), f"{dispatch} {it}: copy {k} of the merged factorisation")
        assert multi[k][2].tolist() == expected(c)
        assert blockwise(c.prob, multi[k][:2], c.oracle(E_SIGMA * f)[:2]) < 1e-10


@pytest.mark.gpu
@pytest.mark.parametrize("lmm", [False, True], ids=["large", "lmm"])
@pytest.mark.parametrize("it", [None, "cheb"], ids=["defaults", "cheb"])
@pytest.mark.parametrize("dispatch", ["default", "tiled64"])
def test_tau_one_copies_are_ok(dispatch, it, lmm):
    """tau = 1, the Manual's setting.  Before the status was gated on a lowered cap, CG (the
    default) reported status 4 for every iterated copy of every block of >= 64 SNPs with a large
    SNP here: its stopping bound is 0."""
    key = dict(tau=1.0, lmm=lmm)
    c = case_e(**key)
    multi, wl = multi_e(key, dispatch, it, H2F)
    assert wl["cheb_iters"] > 0
    worst = check_copies(c, key, dispatch, H2F, multi, wl, f"tau 1 {dispatch} {it or 'defaults'} lmm {lmm}")
    print(f"tau 1 {dispatch} {it or 'defaults'} lmm {lmm}: worst per-block error {worst:.3e}")
    if it is None:
        again, _ = gpu_multi(c.variant(**DISPATCH[dispatch]), sigmas(H2F))
        for k in range(len(H2F)):
            same(again[k], multi[k], f"tau 1 {dispatch}: CG copy {k} on a second run")


@pytest.mark.gpu
@pytest.mark.parametrize("dispatch", ["default", "tiled64"])
def test_not_pd_block_beside_iteration_panel(dispatch):
    from dbslmm_amd import BLOCK_NOT_PD
    key = dict(tau=E_DUP_TAU, dup=True)
    c, e = case_e(**key), case_e(emptied=True, **key)
    multi, wl = multi_e(key, dispatch, None, H2F)
    alone, _ = multi_e(dict(emptied=True, **key), dispatch, None, H2F)
    assert wl["cheb_iters"] == 0              # tau > 1: every copy factored
    want = np.array(expected(c))
    want[E_DUP_BLOCK] = BLOCK_NOT_PD
    for k, f in enumerate(H2F):
        assert multi[k][2].tolist() == want.tolist(), (k, multi[k][2])
        assert np.all(np.isnan(c.of(multi[k], E_DUP_BLOCK))), k
        err = blockwise(c.prob, multi[k][:2], c.oracle(E_SIGMA * f)[:2], skip=[E_DUP_BLOCK])
        print(f"NOT_PD {dispatch} copy {k}: worst healthy block {err:.3e}")
        assert err < (1e-10 if k == 1 else CHEB_TOL), (k, err)
        for b in c.healthy:
            assert np.all(np.isfinite(c.of(multi[k], b))), (k, b)
            np.testing.assert_array_equal(c.of(multi[k], b), e.of(alone[k], b), err_msg=f"copy {k} block {b}")
    same(multi[1], fresh_e(key, dispatch, 1.0), "the base sigma vs a fresh plan")
