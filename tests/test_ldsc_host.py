"""LD scores and LD score regression without a GPU: the oracle's self-checks (tests/_ldsc_ref.py), the
preconditions of the GPU cases of tests/test_ldsc.py, the stand-alone sanitizer program over
ldsc_layout.hpp and ldsc_fit.hpp, dbslmm_ldsc_fit (host only) against the NumPy rule, and the CLI's
--ldsc arguments through --dry-run."""
import os
import subprocess

import numpy as np
import pytest

import _clump_ref as CR
import _ldsc_ref as LR
from _common import BLOCKS_EUR1, ROOT, TD, load_bed
from test_sanitizers import BIN, _built, _clean, _run

SUMM = os.path.join(TD, "summary_gemma_chr1.assoc.txt")
REF = os.path.join(TD, "ref_chr1")
CLI = os.path.join(ROOT, "dbslmm_amd", "bin", "dbslmm")


# ------------------------------------------------------------------------------------------------
# the oracle
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hand():
    """9 rows over 203 individuals: 3 monomorphic, 4 all missing, 5 without variance among its calls"""
    rng = np.random.default_rng(0)
    X = rng.integers(-1, 3, size=(9, 203)).astype(np.int8)
    X[3] = 2
    X[4] = -1
    X[5, X[5] >= 0] = 1
    return X


def test_oracle_is_the_row_sum_of_squared_correlations(hand):
    """unbiased = 0 under a covering window: the row sums of corrcoef(mean-imputed rows)^2 to 1e-12;
    a NaN row gets NaN and its neighbours lose nothing but its term"""
    X = hand
    chrom, bp = np.ones(9), 100 * np.arange(9)
    ref = LR.ld_scores_ref(X, chrom, bp, 10_000, False, 203)
    ok = [0, 1, 2, 6, 7, 8]
    xs = np.where(X < 0, np.nan, X).astype(np.float64)
    mu = np.nanmean(xs[ok], axis=1, keepdims=True)
    want = (np.corrcoef(np.where(np.isnan(xs[ok]), mu, xs[ok])) ** 2).sum(axis=1)
    assert np.max(np.abs(ref["l2"][ok].astype(np.float64) - want)) < 1e-12
    assert np.all(np.isnan(ref["l2"][[3, 4, 5]])) and np.all(ref["nan_row"][[3, 4, 5]])
    assert np.all(ref["n_window"] == 9) and np.all(ref["n_terms"][ok] == 6)
    alone = LR.ld_scores_ref(X[ok], chrom[ok], bp[ok], 10_000, False, 203)
    assert float(np.max(np.abs(alone["l2"] - ref["l2"][ok]))) < 1e-17   # the NaN rows added nothing
    # ldsc's adjustment, term by term
    adj = LR.ld_scores_ref(X, chrom, bp, 10_000, True, 203)
    r2 = ref["r2"][np.ix_(ok, ok)].astype(np.float64)
    assert np.max(np.abs(adj["l2"][ok].astype(np.float64) - (r2 - (1 - r2) / 201).sum(axis=1))) < 1e-12


def test_oracle_window_edges(hand):
    """a pair at exactly window_bp is in, at window_bp + 1 out; equal bp on two chromosomes never
    meet; window 0 keeps the rows at one position"""
    X = hand[[0, 1, 2, 6, 7, 8]]
    r2 = CR.r2_longdouble(X).astype(np.float64)
    bp = np.array([0, 500, 1000, 1001, 1001, 3000])
    chrom = np.array([1, 1, 1, 1, 2, 1])
    ref = LR.ld_scores_ref(X, chrom, bp, 500, False, 203)
    np.testing.assert_array_equal(ref["n_window"], [2, 3, 3, 2, 1, 1])
    want = [1 + r2[0, 1], 1 + r2[1, 0] + r2[1, 2], 1 + r2[2, 1] + r2[2, 3], 1 + r2[3, 2], 1, 1]
    assert np.max(np.abs(ref["l2"].astype(np.float64) - want)) < 1e-15
    np.testing.assert_array_equal(LR.ld_scores_ref(X, chrom, bp, 499, False, 203)["n_window"], [1, 1, 2, 2, 1, 1])
    ref0 = LR.ld_scores_ref(X, np.ones(6), bp, 0, False, 203)
    np.testing.assert_array_equal(ref0["n_window"], [1, 1, 1, 2, 2, 1])
    assert abs(float(ref0["l2"][3]) - (1 + r2[3, 4])) < 1e-15
    # caller order does not matter
    perm = np.array([4, 0, 5, 2, 1, 3])
    shuf = LR.ld_scores_ref(X[perm], chrom[perm], bp[perm], 500, False, 203)
    np.testing.assert_array_equal(shuf["n_window"], ref["n_window"][perm])
    assert np.max(np.abs((shuf["l2"] - ref["l2"][perm]).astype(np.float64))) < 1e-15


def test_test_dat_has_the_properties_the_gpu_case_claims():
    """723 .bim rows on one chromosome in bp order, no missing call, no NaN row, 722 of the 996 summary
    SNPs in the .bim; at 50 kb n_window is 32 / 239 / 289 (min / median / max) and the band reaches two
    tile columns of 128 past the diagonal; at 1000 kb every row sees all 723"""
    td = LR.test_dat_inputs(SUMM, REF)
    X = CR.decode(load_bed(REF + ".bed"), 400, np.arange(723))
    assert len(td["snp"]) == 723 and X.shape == (723, 400) and np.all(X >= 0)
    assert set(td["chrom"]) == {0} and np.all(np.diff(td["bp"]) >= 0)
    assert td["n_summ"] == 996 and int((td["summ_of"] >= 0).sum()) == 722
    assert np.all(X.min(axis=1) < X.max(axis=1))                     # every row varies: no NaN row
    W = LR.window_matrix(td["chrom"], td["bp"], 50_000)
    nw = W.sum(axis=1)
    assert (int(nw.min()), int(np.median(nw)), int(nw.max())) == (32, 239, 289)
    i, j = np.nonzero(W)
    assert int(np.max(np.abs(i // 128 - j // 128))) == 2             # tiles (I, I + 2): three columns wide
    assert np.all(LR.window_matrix(td["chrom"], td["bp"], 1_000_000).sum(axis=1) == 723)


def test_gpu_window_cases_have_the_band_widths_they_claim():
    from test_ldsc import WINDOW_CASES, _band_width
    for name, (chrom, bp, window_bp, width) in WINDOW_CASES.items():
        assert _band_width(chrom, bp, window_bp) == width, name
    chrom, bp, w, _ = WINDOW_CASES["one column, gaps wider than the window"]
    assert np.max(np.diff(np.sort(bp))) > w


def test_gpu_ragged_cases_have_the_reaches_they_claim():
    """the ragged band of tests/test_ldsc.py from the oracle's position order and window matrix alone:
    the tile rows reach 0, 1, 2 and 3 tile columns past the diagonal, neither rising nor falling
    throughout; distinct positions (the shuffled call has one position order); a gap wider than the
    window and none of its pairs in any window; dense and sparse stretches; the rows with missing calls
    cover a whole tile row and leave others untouched; the second case changes chromosome inside a tile
    and no window crosses the change"""
    from test_ldsc import RAGGED_CASES, RAGGED_MISSING, RAGGED_N, RAGGED_WINDOW, tile_row_reach
    for name, (chrom, bp, reach) in RAGGED_CASES.items():
        got = tile_row_reach(chrom, bp, RAGGED_WINDOW)
        assert got == reach, (name, got)
        d = np.diff(got)
        assert (d > 0).any() and (d < 0).any(), name
        assert len(chrom) == RAGGED_N == 900 and len(got) == 8
        order = LR.position_order(chrom, bp)
        np.testing.assert_array_equal(order, np.arange(RAGGED_N))          # caller order = position order
        assert len({(int(c), int(b)) for c, b in zip(chrom, bp)}) == RAGGED_N
        nw = LR.window_matrix(chrom, bp, RAGGED_WINDOW).sum(axis=1)
        assert nw.min() < 80 and nw.max() > 400, (name, nw.min(), nw.max())  # sparse and dense stretches
    chrom, bp, reach = RAGGED_CASES["one chromosome"]
    assert set(reach) == {0, 1, 2, 3}
    gap = int(np.argmax(np.diff(bp)))
    assert bp[gap + 1] - bp[gap] > RAGGED_WINDOW and gap // 128 == (gap + 1) // 128   # the gap inside tile row 4
    assert not LR.window_matrix(chrom, bp, RAGGED_WINDOW)[:gap + 1, gap + 1:].any()
    chrom, bp, _ = RAGGED_CASES["two chromosomes, the change inside a tile"]
    change = int(np.flatnonzero(np.diff(chrom))[0]) + 1
    assert len(np.flatnonzero(np.diff(chrom))) == 1 and change % 128 != 0
    assert not LR.window_matrix(chrom, bp, RAGGED_WINDOW)[:change, change:].any()
    assert bp[chrom == 2].min() < bp[chrom == 1].max()               # the bp ranges of the two overlap
    lo, hi = RAGGED_MISSING
    assert hi - lo >= 128 and any(lo <= 128 * I and 128 * (I + 1) <= hi for I in range(8))
    assert lo // 128 > 0 and (hi - 1) // 128 < 5                     # tile rows 0, 1, 5, 6, 7 hold no missing call


def test_ldsc_layout_and_fit_under_asan_ubsan():
    """tests/host/ldsc_check.cpp: the 128-band layout from first principles and ldsc_fit.hpp on a fixed
    data set, under ASan + UBSan (a stand-alone program: no preloaded runtime)"""
    exe = _built(os.path.join(ROOT, "dbslmm_amd", "csrc"), "../bin/ldsc_asan", os.path.join(BIN, "ldsc_asan"))
    r = _run(exe, [])
    assert _clean(r), r.stderr[-3000:]
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stderr[-3000:]


# ------------------------------------------------------------------------------------------------
# the regression (host only)
# ------------------------------------------------------------------------------------------------
def _fixed_data():
    j = np.arange(61)
    l = 1 + ((j * 37) % 101) / 4.0
    N = 40000.0 + ((j * 7919) % 10000)
    return (1 + N * 0.4 * l / 1e5) * (0.2 + ((j * 53) % 17) / 4.0), N, l


def test_fixed_data_set_values_of_the_host_check():
    """the values tests/host/ldsc_check.cpp holds are the NumPy rule's on the same data"""
    chi2, N, l = _fixed_data()
    r = LR.ldsc_fit_ref(chi2, N, l, 1e5, n_blocks=7)
    np.testing.assert_allclose([r["h2"], r["h2_se"], r["intercept"], r["intercept_se"], r["mean_chi2"]],
                               [1.1868932222403816, 0.42493426955392644, 1.2359638193077034, 1.4667763580301476,
                                7.507473225409836], rtol=1e-12)
    r = LR.ldsc_fit_ref(chi2, N, l, 1e5, intercept=1.0, n_blocks=7)
    np.testing.assert_allclose([r["h2"], r["h2_se"]], [1.294347355001953, 0.14570548674778613], rtol=1e-12)
    r = LR.ldsc_fit_ref(chi2, N, l, 1e5, n_blocks=7, chisq_max=5.0)
    assert r["n"] == 25
    np.testing.assert_allclose([r["h2"], r["intercept"]], [0.1704796896413038, 2.0528521285892105], rtol=1e-12)


KEYS = ("h2", "h2_se", "intercept", "intercept_se", "mean_chi2")


@pytest.mark.parametrize("n", [3, 199, 200, 201, 5000])
@pytest.mark.parametrize("intercept", [None, 1.05])
def test_ldsc_fit_equals_the_numpy_rule(n, intercept):
    """dbslmm_ldsc_fit through ctypes against ldsc_fit_ref, 200 blocks: both form the same block normal
    equations, so only the summation order differs.  rtol 1e-8 on estimates and SEs, four decades above
    the kappa n u expected of these 2 x 2 systems; the worst observed is printed (DESIGN.md section 3.9
    records it: below 1e-10)."""
    from dbslmm_amd import ldsc_h2
    rng = np.random.default_rng(100 + n)
    chi2, N, l = (v[:n] for v in LR.simulate(rng))
    got = ldsc_h2(chi2, N, l, 1e5, intercept=intercept, n_blocks=200)
    ref = LR.ldsc_fit_ref(chi2, N, l, 1e5, intercept=intercept, n_blocks=200)
    assert got["status"] == ref["status"] and got["n"] == ref["n"] == n
    if n == 3 and intercept is None:                                 # fewer SNPs than twice the parameters
        assert got["status"] == 1 and np.isnan(got["h2"]) and np.isnan(got["h2_se"])
        return
    assert got["status"] == 0
    rel = [abs(got[k] - ref[k]) / abs(ref[k]) for k in KEYS if ref[k] != 0]
    print(f"ldsc_fit n {n} intercept {intercept}: worst relative difference {max(rel):.3g}")
    for k in KEYS:
        np.testing.assert_allclose(got[k], ref[k], rtol=1e-8, atol=0, err_msg=k)
    if intercept is not None:
        assert got["intercept"] == intercept and got["intercept_se"] == 0.0


def test_ldsc_fit_statuses_and_options():
    from dbslmm_amd import DbslmmError, ldsc_h2
    rng = np.random.default_rng(7)
    chi2, N, l = (v[:500] for v in LR.simulate(rng))
    # singular: every x equal with a free intercept; fine with a fixed one
    r = ldsc_h2(chi2, 45000.0, np.full(500, 12.5), 1e5)
    assert r["status"] == 2 and np.isnan(r["h2"]) and LR.ldsc_fit_ref(chi2, 45000.0, np.full(500, 12.5), 1e5)["status"] == 2
    assert ldsc_h2(chi2, 45000.0, np.full(500, 12.5), 1e5, intercept=1.0)["status"] == 0
    # too few
    assert ldsc_h2(chi2[:1], N[:1], l[:1], 1e5, intercept=1.0)["status"] == 1
    assert ldsc_h2(chi2[:0], N[:0], l[:0], 1e5)["status"] == 1
    # the chi2 filter drops SNPs before anything else; off by default
    cut = float(np.quantile(chi2, 0.9))
    a, b = ldsc_h2(chi2, N, l, 1e5, chisq_max=cut), LR.ldsc_fit_ref(chi2, N, l, 1e5, chisq_max=cut)
    assert a["n"] == b["n"] == int((chi2 <= cut).sum()) < 500
    np.testing.assert_allclose(a["h2"], b["h2"], rtol=1e-8)
    assert ldsc_h2(chi2, N, l, 1e5)["n"] == 500
    # 0 blocks = 200; fewer blocks change the SE only
    assert ldsc_h2(chi2, N, l, 1e5, n_blocks=0) == ldsc_h2(chi2, N, l, 1e5, n_blocks=200)
    c = ldsc_h2(chi2, N, l, 1e5, n_blocks=10)
    assert c["h2"] == pytest.approx(ldsc_h2(chi2, N, l, 1e5)["h2"], rel=1e-12) and c["h2_se"] != ldsc_h2(chi2, N, l, 1e5)["h2_se"]
    for bad in (dict(m=0.0), dict(n_blocks=1), dict(n_blocks=-3), dict(chisq_max=-1.0)):
        kw = dict(m=1e5)
        kw.update(bad)
        with pytest.raises(DbslmmError):
            ldsc_h2(chi2, N, l, **kw)


def test_ldsc_fit_recovers_the_simulated_heritability():
    """independent chi2 with E = a + N h2 l / M, M = 1e5, N in [4e4, 5e4), l = 1 + Gamma(2, 20), h2 = 0.4,
    a = 1.05, seed 1, four trials, both modes: within 4 SE of the truth (the NumPy rule alone stays
    within 1.6 SE on these inputs)"""
    from dbslmm_amd import ldsc_h2
    rng = np.random.default_rng(1)
    for trial in range(4):
        chi2, N, l = LR.simulate(rng)
        free = ldsc_h2(chi2, N, l, 1e5)
        fixed = ldsc_h2(chi2, N, l, 1e5, intercept=1.05)
        print(f"trial {trial}: free h2 {free['h2']:.4f} ({free['h2_se']:.4f}) a {free['intercept']:.4f} "
              f"({free['intercept_se']:.4f}); fixed h2 {fixed['h2']:.4f} ({fixed['h2_se']:.4f})")
        assert free["status"] == 0 and fixed["status"] == 0
        assert abs(free["h2"] - 0.4) <= 4 * free["h2_se"]
        assert abs(free["intercept"] - 1.05) <= 4 * free["intercept_se"]
        assert abs(fixed["h2"] - 0.4) <= 4 * fixed["h2_se"]
        assert 0 < fixed["h2_se"] < free["h2_se"] < 0.1


# ------------------------------------------------------------------------------------------------
# CLI arguments (host only: --dry-run)
# ------------------------------------------------------------------------------------------------
BASE = ["--ldsc", "--summary", SUMM, "-r", REF, "--dry-run"]


def _cli(args, cwd):
    return subprocess.run([CLI] + args, capture_output=True, text=True, cwd=str(cwd), timeout=300)


def test_cli_ldsc_dry_run_counts_rows_and_regression_snps(tmp_path):
    r = _cli(BASE + ["--out", str(tmp_path / "o")], tmp_path)
    assert r.returncode == 0, r.stderr
    assert "dry-run: 723 rows, 722 regression SNPs; stops before the LD scores" in r.stdout, r.stdout
    assert not os.listdir(str(tmp_path))
    r = _cli(["--ldsc", "--summary", SUMM + "," + SUMM, "-r", REF + "," + REF, "--dry-run", "--out", str(tmp_path / "o"),
              "--intercept", "1", "--ld-wind-kb", "50", "--chisq-max", "80"], tmp_path)
    assert r.returncode == 0 and "dry-run: 1446 rows, 1444 regression SNPs" in r.stdout, (r.stdout, r.stderr)


@pytest.mark.parametrize("args,msg", [
    (BASE + ["--out", "o", "-s", SUMM], "no -s / -l / -b"),
    (BASE + ["--out", "o", "-l", SUMM], "no -s / -l / -b"),
    (BASE + ["--out", "o", "-b", BLOCKS_EUR1], "no -s / -l / -b"),
    (BASE, "--ldsc needs --out"),
    (["--ldsc", "--summary", SUMM + "," + SUMM, "-r", REF, "--out", "o", "--dry-run"], "the same number of files"),
    (BASE + ["--out", "o", "--ld-wind-kb", "-1"], "--ld-wind-kb must not be negative"),
    (BASE + ["--out", "o", "--intercept", "fre"], "--intercept must be `free` or a number"),
    (BASE + ["--out", "o", "--intercept", "1.0x"], "--intercept must be `free` or a number"),
    (["--ldsc", "--summary", "/nonexistent", "-r", REF, "--out", "o", "--dry-run"], "dose not exist"),
    (["--ldsc", "--summary", SUMM, "-r", "/nonexistent", "--out", "o", "--dry-run"], "dose not exist"),
])
def test_cli_ldsc_argument_errors(args, msg, tmp_path):
    r = _cli(args, tmp_path)
    assert r.returncode == 1 and msg in r.stderr, (r.returncode, r.stderr)


def test_cli_ldsc_host_path_under_asan_ubsan(tmp_path):
    """the host side of --ldsc (list parsing, the n_obs column, the row matching) in the sanitizer
    build of the CLI, a stand-alone program"""
    exe = _built(os.path.join(ROOT, "dbslmm_amd", "csrc"), "sanitize", os.path.join(BIN, "dbslmm_asan"))
    r = _run(exe, BASE + ["--out", str(tmp_path / "o")], cwd=str(tmp_path))
    assert _clean(r), r.stderr[-3000:]
    assert r.returncode == 0 and "dry-run: 723 rows, 722 regression SNPs" in r.stdout, (r.returncode, r.stderr[-2000:])
    r = _run(exe, BASE + ["--out", str(tmp_path / "o"), "--intercept", "x"], cwd=str(tmp_path))
    assert _clean(r) and r.returncode == 1, r.stderr[-3000:]
