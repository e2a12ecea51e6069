"""The panel image's row table (kernels.hip: dbslmm_bed_repitch reduces each row's exact integer
dosage sum, sum of squares and missing-call count while it builds the image) and everything that
now derives its per-row statistics from it: dbslmm_slot_stats in the plans' runs (both routes),
bed_maf, read_snp_std, and the table's lifetime next to the image bytes it belongs to.

Panels of tests 1 and 2 are built here from explicit 2-bit PLINK codes; the reference of the table
is a NumPy unpack of the same bytes."""
import functools

import numpy as np
import pytest

import oracle as O
from _common import normwise
from test_rawbed_gram import CLASSES, _all_equal, _panel, _rows_problem, _wide_panel
from test_tiled import _oracle

pytestmark = pytest.mark.gpu

# a row shorter than one 16-byte chunk; both sides of the 64-individual chunk edge; odd bytes per
# row (file rows at every byte alignment); both sides of the 256 and 1024 stage edges; 65 chunks
# (a lane takes a second pass)
N_REFS = [5, 63, 64, 65, 250, 257, 1021, 1024, 4099]
N_ROWS = 37                      # not a multiple of the 4 waves per workgroup
N_RANDOM = N_ROWS - 5
FILLS = (1, 0, 3)                # pad bits of every row's last byte: 01 (missing), 00 (dosage 2), 11
# PLINK code (low bit first): 00 -> dosage 2, 10 -> 1, 11 -> 0, 01 -> missing
C_TWO, C_MISS, C_ONE, C_ZERO = 0, 1, 2, 3


@pytest.fixture(scope="module")
def ctx():
    from dbslmm_amd import Context
    c = Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _codes(n_ref, miss):
    """(N_ROWS, n_ref) 2-bit codes: N_RANDOM random rows (the first half of them made polymorphic
    by a fixed dosage-2 and dosage-0 call, so that they have a standard deviation), then rows that
    are all 00, all 11, all missing, and with one missing call at individual 0 / n_ref - 1 only."""
    rng = np.random.default_rng(1000 * n_ref + int(1000 * miss))
    c = rng.choice(np.array([C_TWO, C_ONE, C_ZERO], dtype=np.uint8), size=(N_ROWS, n_ref), p=[0.2, 0.4, 0.4])
    c[:N_RANDOM][rng.random((N_RANDOM, n_ref)) < miss] = C_MISS
    c[:N_RANDOM // 2, 1] = C_TWO
    c[:N_RANDOM // 2, 2] = C_ZERO
    c[N_RANDOM + 0] = C_TWO
    c[N_RANDOM + 1] = C_ZERO
    c[N_RANDOM + 2] = C_MISS
    c[N_RANDOM + 3][c[N_RANDOM + 3] == C_MISS] = C_ONE
    c[N_RANDOM + 3, 0] = C_MISS
    c[N_RANDOM + 3, 1:3] = (C_TWO, C_ZERO)
    c[N_RANDOM + 4][c[N_RANDOM + 4] == C_MISS] = C_ONE
    c[N_RANDOM + 4, n_ref - 1] = C_MISS
    c[N_RANDOM + 4, 1:3] = (C_TWO, C_ZERO)
    c.setflags(write=False)
    return c


def _bed(codes, fill):
    """the .bed image (magic + rows of ceil(n_ref / 4) bytes) with every pad field = fill"""
    m, n = codes.shape
    nb = (n + 3) // 4
    c = np.full((m, 4 * nb), fill, dtype=np.uint8)
    c[:, :n] = codes
    c4 = c.reshape(m, nb, 4)
    rows = c4[:, :, 0] | (c4[:, :, 1] << 2) | (c4[:, :, 2] << 4) | (c4[:, :, 3] << 6)
    return np.concatenate([np.array([0x6C, 0x1B, 0x01], dtype=np.uint8), rows.astype(np.uint8).ravel()])


def _exact(bed, n_ref, n_rows):
    """NumPy unpack of the image's bytes -> exact (sum, sumsq, nmiss) per row"""
    nb = (n_ref + 3) // 4
    rows = bed[3:3 + n_rows * nb].reshape(n_rows, nb)
    c = ((rows[:, :, None] >> np.array([0, 2, 4, 6], dtype=np.uint8)) & 3).reshape(n_rows, 4 * nb)[:, :n_ref]
    two, one, mis = (c == C_TWO).sum(1), (c == C_ONE).sum(1), (c == C_MISS).sum(1)
    return np.stack([2 * two + one, 4 * two + one, mis], axis=1).astype(np.int32)


# rows with a finite standard deviation: the polymorphic random rows and the two single-missing rows
STD_ROWS = list(range(N_RANDOM // 2)) + [N_RANDOM + 3, N_RANDOM + 4]


@pytest.mark.parametrize("miss", [0.0, 0.07])
@pytest.mark.parametrize("n_ref", N_REFS)
def test_table_exact(ctx, n_ref, miss):
    """1. dbslmm_bed_row_stats equals the exact integers, whatever the pad bits hold."""
    codes = _codes(n_ref, miss)
    tabs = []
    for fill in FILLS:
        bed = _bed(codes, fill)
        if n_ref % 4:
            assert np.all(bed[3:].reshape(N_ROWS, -1)[:, -1] >> (2 * (n_ref % 4)) == (fill * 0x55) >> (2 * (n_ref % 4)))
        got = ctx.row_stats(bed, n_ref, N_ROWS)
        assert got.shape == (N_ROWS, 3) and got.dtype == np.int32
        np.testing.assert_array_equal(got, _exact(bed, n_ref, N_ROWS))
        tabs.append(got)
    np.testing.assert_array_equal(tabs[0], tabs[1])
    np.testing.assert_array_equal(tabs[0], tabs[2])
    want = tabs[0]
    assert want[N_RANDOM + 0].tolist() == [2 * n_ref, 4 * n_ref, 0]
    assert want[N_RANDOM + 1].tolist() == [0, 0, 0]
    assert want[N_RANDOM + 2].tolist() == [0, 0, n_ref]
    assert want[N_RANDOM + 3, 2] == 1 and want[N_RANDOM + 4, 2] == 1
    if miss > 0 and n_ref >= 63:
        assert want[:N_RANDOM, 2].sum() > 0


@pytest.mark.parametrize("miss", [0.0, 0.07])
@pytest.mark.parametrize("n_ref", N_REFS)
def test_consumers(ctx, n_ref, miss):
    """2. bed_maf bit for bit the oracle's MAF pass; read_snp_std within the bounds of
    test_gpu.py::test_read_snp_std_matches_oracle (columns 1e-12, MAF 1e-14)."""
    from dbslmm_amd import bed_maf, read_snp_std
    codes = _codes(n_ref, miss)
    idv = np.ones(n_ref, dtype=np.int32)
    for fill in FILLS:
        bed = _bed(codes, fill)
        np.testing.assert_array_equal(bed_maf(ctx, bed, n_ref, N_ROWS), O.bed_maf(bed, n_ref, N_ROWS))
        X, maf = read_snp_std(ctx, bed, n_ref, STD_ROWS)
        for j, r in enumerate(STD_ROWS):
            g, m = O.read_snp_im(bed, r, idv)
            np.testing.assert_allclose(X[:, j], O.normalize(g), rtol=0, atol=1e-12)
            assert abs(maf[j] - m) < 1e-14


# ------------------------------------------------------------------------------------------------
# 3. solves
# ------------------------------------------------------------------------------------------------
SIGMA_F = (0.5, 1.0, 2.0)


@functools.lru_cache(maxsize=None)
def _panel_oracle_sigma(n_ref, miss, f):
    from dbslmm_amd import synth
    prob = synth.make_problem(_panel(n_ref, miss))
    prob.sigma_s *= f
    return _oracle(prob)


def _plan_runs(ctx, prob, sigmas=None, **opts):
    """one plan, run twice -> the first result (the second must equal it bit for bit)"""
    from dbslmm_amd import Plan
    keep = dict(prob.opts)
    prob.opts.update(opts)
    try:
        plan = Plan(ctx, prob)
        outs = []
        for _ in range(2):
            if sigmas is None:
                plan.run()
                plan.sync()
                outs.append([plan.download()])
            else:
                outs.append([tuple(a.copy() for a in r) for r in plan.run_multi(sigmas)])
        route = plan.workload()["pcg_route"]
        plan.close()
    finally:
        prob.opts.clear()
        prob.opts.update(keep)
    for a, b in zip(outs[0], outs[1]):
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)
    return outs[0], route


def _solve_all_ways(ctx, prob, refs):
    """factorisation route (3 Gram classes), forced PCG route (3 classes; single and 3 sigmas);
    refs[f] = oracle (beta, status) at sigma_s * f.  Returns the factorisation result."""
    sig = [prob.sigma_s * f for f in SIGMA_F]
    fac, pcg1, pcg3 = [], [], []
    for big, huge in CLASSES:
        kw = dict(gram_big_min=big, gram_huge_min=min(huge, 2 ** 31 - 1))
        out, route = _plan_runs(ctx, prob, solver=1, **kw)
        assert route == 0
        fac.append(out[0])
        out, route = _plan_runs(ctx, prob, solver=2, **kw)
        assert route == 1
        pcg1.append(out[0])
        out, route = _plan_runs(ctx, prob, sigmas=sig, solver=2, **kw)
        assert route == 1
        pcg3.append([x for r in out for x in r])
    _all_equal(fac)
    _all_equal(pcg1)
    _all_equal(pcg3)
    ref1, _ = refs[1.0]
    for name, res in (("factor", fac[0]), ("pcg", pcg1[0])):
        err = normwise(np.concatenate(res[:2]), ref1)
        print(f"{name}: normwise {err:.3e}")
        assert err < 1e-10
    np.testing.assert_array_equal(pcg1[0][2], fac[0][2])
    for i, f in enumerate(SIGMA_F):
        ref, _ = refs[f]
        err = normwise(np.concatenate(pcg3[0][3 * i:3 * i + 2]), ref)
        print(f"pcg x3, sigma x {f}: normwise {err:.3e}")
        assert err < 1e-10
        np.testing.assert_array_equal(pcg3[0][3 * i + 2], fac[0][2])
    return fac[0]


@pytest.mark.parametrize("miss", [0.0, 0.01])
@pytest.mark.parametrize("n_ref", [257, 1024])
def test_solves(ctx, n_ref, miss):
    from dbslmm_amd import synth
    prob = synth.make_problem(_panel(n_ref, miss))
    _solve_all_ways(ctx, prob, {f: _panel_oracle_sigma(n_ref, miss, f) for f in SIGMA_F})


def test_solves_scattered_rows(ctx):
    """Rows in descending order, image row 71 in both blocks, padding slots in both blocks."""
    sizes = [130, 70]
    rows = list(range(200, 70, -1)) + list(range(71, 1, -1))
    assert rows.count(71) == 2 and all(s % 32 != 31 for s in sizes)
    p = _wide_panel(257, 1843)
    d, BlockProblem = _rows_problem(257, sizes, rows)
    prob = BlockProblem(bed=p.bed, **d)
    refs = {}
    for f in SIGMA_F:
        prob.sigma_s = d["sigma_s"] * f
        refs[f] = _oracle(prob)
    prob.sigma_s = d["sigma_s"]
    res = _solve_all_ways(ctx, prob, refs)
    assert np.all(res[2] == 0)


def test_one_missing_call(ctx):
    """Two blocks; one call of one slot of block 0 is missing: block 0 takes the missing-call path
    (status and beta against the oracle), block 1 is what it was without the missing call."""
    from dbslmm_amd import DBSLMMFIT
    n_ref, sizes = 257, [40, 50]
    p = _panel(n_ref, 0.0)
    d, BlockProblem = _rows_problem(n_ref, sizes, np.arange(sum(sizes)))
    nb = (n_ref + 3) // 4
    row, ind = 10, 100
    bed = p.bed.copy()
    at, sh = 3 + row * nb + ind // 4, 2 * (ind % 4)
    bed[at] = (bed[at] & ~np.uint8(3 << sh)) | np.uint8(C_MISS << sh)
    tab0, tab1 = ctx.row_stats(p.bed, n_ref, sum(sizes)), ctx.row_stats(bed, n_ref, sum(sizes))
    assert tab0[:, 2].sum() == 0 and tab1[:, 2].sum() == 1 and tab1[row, 2] == 1
    fit = DBSLMMFIT(0)
    clean = fit.est(BlockProblem(bed=p.bed, **d))
    for solver in (1, 2):
        prob = BlockProblem(bed=bed, opts={"solver": solver}, **d)
        got = fit.est(prob)
        ref, st = _oracle(prob)
        err = normwise(np.concatenate(got[:2]), ref)
        print(f"solver {solver}: normwise {err:.3e}")
        assert err < 1e-10
        np.testing.assert_array_equal(got[2], st)
    prob = BlockProblem(bed=bed, **d)
    got = fit.est(prob)
    in0_s = np.arange(d["s_ptr"][0], d["s_ptr"][1])
    in1_s = np.arange(d["s_ptr"][1], d["s_ptr"][2])
    in1_l = np.arange(d["l_ptr"][1], d["l_ptr"][2])
    np.testing.assert_array_equal(got[0][in1_s], clean[0][in1_s])
    np.testing.assert_array_equal(got[1][in1_l], clean[1][in1_l])
    assert np.any(got[0][in0_s] != clean[0][in0_s])


# ------------------------------------------------------------------------------------------------
# 4. lifetime
# ------------------------------------------------------------------------------------------------
def _fresh(prob):
    from dbslmm_amd import Context, Plan
    c = Context(0)
    plan = Plan(c, prob)
    plan.run()
    plan.sync()
    out = plan.download()
    plan.close()
    c.close()
    return out


@pytest.mark.parametrize("other", [(257, 0.01), (1024, 0.0)])
def test_table_lives_with_its_image(other):
    """Plan A keeps the cached image and table of panel A after the context has cached panel B
    (same n_ref / another n_ref) and created plan B from it."""
    from dbslmm_amd import Context, Plan, synth
    pa, pb = _panel(257, 0.0), _panel(*other)
    prob_a, prob_b = synth.make_problem(pa), synth.make_problem(pb)
    want_a, want_b = _fresh(prob_a), _fresh(prob_b)
    c = Context(0)
    c.cache_bed(prob_a.bed)
    plan_a = Plan(c, prob_a)
    c.cache_bed(prob_b.bed)
    plan_b = Plan(c, prob_b)
    np.testing.assert_array_equal(c.row_stats(prob_b.bed, pb.n_ref, pb.m), _exact(pb.bed, pb.n_ref, pb.m))
    for plan, want in ((plan_a, want_a), (plan_b, want_b), (plan_a, want_a)):
        plan.run()
        plan.sync()
        for x, y in zip(plan.download(), want):
            np.testing.assert_array_equal(x, y)
    plan_a.close()
    plan_b.close()
    c.close()


def test_two_sub_contexts():
    """Context([0, 0]): each sub-context's image carries its own table."""
    from dbslmm_amd import DBSLMMFIT, synth
    prob = synth.make_problem(_panel(257, 0.01))
    one = DBSLMMFIT(0).est(prob)
    two = DBSLMMFIT([0, 0]).est(prob)
    for x, y in zip(one, two):
        np.testing.assert_array_equal(x, y)
