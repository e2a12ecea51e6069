"""The association scan without a GPU: the NumPy restatement (tests/_assoc_ref.py) pinned against
scipy.stats.linregress and numpy.linalg.lstsq, the Student t tail against scipy, the host finish
(dbslmm_assoc_stat_host) on every status, the stand-alone sanitizer program over assoc_layout.hpp and
assoc_fit.hpp, and the CLI's --assoc arguments through --dry-run."""
import os

import numpy as np
import pytest
import scipy.stats

import _assoc_ref as AR
from _common import ROOT
from test_sanitizers import BIN, _built, _clean, _run

CSRC = os.path.join(ROOT, "dbslmm_amd", "csrc")


def random_panel(rng, n_rows, n_total, miss=0.0):
    g = rng.integers(0, 3, size=(n_rows, n_total)).astype(np.int8)
    m = rng.random((n_rows, n_total)) < miss
    return g, m


# ------------------------------------------------------------------------------------------------
# the restatement itself
# ------------------------------------------------------------------------------------------------
def test_restatement_is_linregress_without_covariates():
    """c = 1, no missing call: slope, stderr and p-value of scipy.stats.linregress to 1e-10."""
    rng = np.random.default_rng(1)
    n = 211
    g, m = random_panel(rng, 12, n)
    y = 0.3 * g[0] + rng.standard_normal(n)
    ref = AR.scan(AR.encode(g), n, y)
    assert np.all(ref["status"] == AR.OK) and ref["df"] == n - 2
    for j in range(12):
        lr = scipy.stats.linregress(g[j].astype(np.float64), y)
        assert abs(ref["beta"][0, j] - lr.slope) <= 1e-10 * abs(lr.slope)
        assert abs(ref["se"][0, j] - lr.stderr) <= 1e-10 * lr.stderr
        assert abs(ref["p"][0, j] - lr.pvalue) <= 1e-10 * lr.pvalue


def test_restatement_is_least_squares_with_covariates_and_missing_calls():
    """Covariates, keep holes, NaN phenotypes and 5 % missing calls: the coefficient of the mean-imputed
    column in numpy.linalg.lstsq on [1 | covar | x] and the classical standard error
    sqrt(s2 (X^T X)^-1_xx), s2 = rss / (n - c - 1), to 1e-10; both orders of summation and both dtypes."""
    rng = np.random.default_rng(2)
    n_total = 300
    g, m = random_panel(rng, 10, n_total, 0.05)
    w = rng.standard_normal((n_total, 3))
    y = np.stack([0.2 * g[1] + w @ [0.5, -1.0, 0.25] + rng.standard_normal(n_total), rng.standard_normal(n_total)], axis=1)
    y[17, 0] = np.nan
    keep = np.ones(n_total, dtype=np.uint8)
    keep[[0, 5, 63, 64, 250]] = 0
    bed = AR.encode(g, m)
    for dtype in (np.float64, np.longdouble):
        for grouped in (False, True):
            ref = AR.scan(bed, n_total, y, w, keep, dtype=dtype, grouped=grouped)
            s = ref["design"]["sel"]
            assert len(s) == n_total - 6 and np.all(ref["status"] == AR.OK)
            for j in range(10):
                x = np.where(m[j, s], np.nan, g[j, s].astype(np.float64))
                x = np.where(np.isnan(x), np.nanmean(x), x)
                X = np.column_stack([np.ones(len(s)), w[s], x])
                for q in range(2):
                    coef, rss = np.linalg.lstsq(X, y[s, q], rcond=None)[:2]
                    s2 = rss[0] / (len(s) - 4 - 1)
                    se = np.sqrt(s2 * np.linalg.inv(X.T @ X)[-1, -1])
                    assert abs(float(ref["beta"][q, j]) - coef[-1]) <= 1e-10 * abs(coef[-1])
                    assert abs(float(ref["se"][q, j]) - se) <= 1e-10 * se
                    pv = 2 * scipy.stats.t.sf(abs(coef[-1] / se), len(s) - 5)
                    assert abs(float(ref["p"][q, j]) - pv) <= 1e-9 * pv   # (p moves ~|T| times as fast as T)
                assert ref["n_mis"][j] == np.sum(m[j, s]) and ref["n_obs"][j] == len(s) - np.sum(m[j, s])


def test_restatement_codes_round_trip():
    """encode / decode: all four codes, the pad bits of a row's last byte zero, no dosage read from them."""
    rng = np.random.default_rng(3)
    g, m = random_panel(rng, 5, 7, 0.2)
    bed = AR.encode(g, m)
    assert bed.size == 3 + 5 * 2 and np.all(bed[3:].reshape(5, 2)[:, 1] >> 6 == 0)
    g2, m2 = AR.decode(bed, 7)
    assert np.array_equal(m2, m) and np.array_equal(g2, np.where(m, 0, g))
    g3, _ = AR.decode(bed, 7, [4, 0, 4])
    assert np.array_equal(g3, g2[[4, 0, 4]])


# ------------------------------------------------------------------------------------------------
# the library's host functions
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("df", [1, 2, 5, 30, 1e3, 1e5])
def test_student_t_two_sided_matches_scipy(df):
    from dbslmm_amd import student_t_two_sided
    for t in (0, 1e-8, 0.5, 2, 10, 40):
        want = 2 * scipy.stats.t.sf(t, df)
        for sign in (1, -1):
            got = student_t_two_sided(sign * t, df)
            assert got == want or abs(got - want) <= 1e-10 * want, (df, t, got, want)


def test_student_t_two_sided_non_finite_is_nan():
    from dbslmm_amd import student_t_two_sided
    for t, df in ((np.nan, 5), (np.inf, 5), (-np.inf, 5), (1, np.nan), (1, np.inf), (1, 0), (1, -3)):
        assert np.isnan(student_t_two_sided(t, df)), (t, df)


def test_assoc_stat_host_every_status():
    """The finish on caller-supplied counts and products: OK rows equal the restatement (the same
    fp64 operations: 16 ulp), a row without a call, the integer monomorphic test on all-0, all-1, all-2
    rows and an all-2 row with missing calls, and a row equal to a covariate is COLLINEAR."""
    from dbslmm_amd import assoc_stat_host
    rng = np.random.default_rng(4)
    n_total = 120
    g, m = random_panel(rng, 12, n_total, 0.05)
    w = rng.standard_normal((n_total, 2))
    g[2], g[3], g[4], g[5] = 0, 1, 2, 2
    m[2] = m[3] = m[4] = False
    m[5] = rng.random(n_total) < 0.3
    m[6] = True
    m[7] = False
    w[:, 1] = g[7]                                    # row 7 is a covariate
    y = rng.standard_normal((n_total, 2)) + 0.3 * g[0][:, None]
    ref = AR.scan(AR.encode(g, m), n_total, y, w)
    want = np.zeros(12, dtype=np.int32)
    want[[2, 3, 4, 5]] = AR.MONOMORPHIC
    want[6] = AR.NO_CALL
    want[7] = AR.COLLINEAR
    assert np.array_equal(ref["status"], want)
    s = ref["design"]["in_s"]
    n1, n2 = np.sum((ref["g"] == 1) & s, axis=1), np.sum((ref["g"] == 2) & s, axis=1)
    with np.errstate(all="ignore"):
        mu = (n1 + 2 * n2) / (ref["design"]["n"] - ref["n_mis"])
    t = ref["prod_d"] + np.where(np.isfinite(mu), mu, 0)[:, None] * ref["prod_m"]
    got = assoc_stat_host(ref["design"]["n"], 3, n1, n2, ref["n_mis"], t, ref["design"]["yy"])
    assert np.array_equal(got["status"], want) and np.array_equal(got["n_obs"], ref["n_obs"])
    assert np.array_equal(got["af"], ref["af"], equal_nan=True)
    assert got["af"][2] == 0 and got["af"][3] == 0.5 and got["af"][4] == 1 and got["af"][5] == 1 and np.isnan(got["af"][6])
    ok = want == AR.OK
    for k in ("beta", "se", "tstat"):
        assert np.all(np.isnan(got[k][:, ~ok]))
        assert np.max(np.abs(got[k][:, ok] / ref[k][:, ok] - 1)) <= 16 * 2.0 ** -52, k
    assert np.all(np.isnan(got["p"][:, ~ok]))
    assert np.max(np.abs(got["p"][:, ok] / ref["p"][:, ok] - 1)) <= 1e-10
    from dbslmm_amd import student_t_two_sided
    assert all(got["p"][q, j] == student_t_two_sided(got["tstat"][q, j], ref["df"]) for q in range(2) for j in np.flatnonzero(ok))


def test_assoc_stat_host_bad_arguments():
    from dbslmm_amd import DbslmmError, assoc_stat_host
    one = np.ones(1, dtype=np.int32)
    with pytest.raises(DbslmmError):
        assoc_stat_host(3, 2, one, one, one, np.zeros((1, 2)), [1.0])      # df = 0
    with pytest.raises(ValueError):
        assoc_stat_host(30, 2, one, one, one, np.zeros((1, 3)), [1.0])     # t: one column too many


# ------------------------------------------------------------------------------------------------
# sanitizers
# ------------------------------------------------------------------------------------------------
def test_assoc_host_check_under_asan_ubsan():
    exe = _built(CSRC, "sanitize", os.path.join(BIN, "assoc_asan"))
    r = _run(exe, [])
    assert _clean(r) and r.returncode == 0 and "assoc_check: ok" in r.stdout, r.stderr[-3000:]


def write_panel(tmp_path, name="train", n_total=40, n_rows=12, seed=5, pheno=True):
    rng = np.random.default_rng(seed)
    g, m = random_panel(rng, n_rows, n_total, 0.02)
    prefix = str(tmp_path / name)
    AR.encode(g, m).tofile(prefix + ".bed")
    y = rng.standard_normal(n_total)
    with open(prefix + ".fam", "w") as f:
        for i in range(n_total):
            f.write(f"F{i} I{i} 0 0 1 {y[i] if pheno and i != 3 else -9}\n")
    with open(prefix + ".bim", "w") as f:
        for j in range(n_rows):
            f.write(f"1\trs{j}\t0\t{1000 + 10 * j}\tA\tG\n")
    with open(prefix + ".pheno", "w") as f:
        for i in range(n_total - 1, 1, -1):                      # another order, two individuals absent
            f.write(f"F{i} I{i} {y[i]} {'NA' if i == 9 else -y[i]}\n")
    w = rng.standard_normal((n_total, 2))
    with open(prefix + ".covar", "w") as f:
        for i in range(n_total):
            f.write(f"F{i} I{i} {w[i, 0]} {w[i, 1]}\n")
    with open(prefix + ".dupcovar", "w") as f:
        for i in range(n_total):
            f.write(f"F{i} I{i} {w[i, 0]} {2 * w[i, 0] + 1}\n")
    with open(prefix + ".keep", "w") as f:
        for i in range(n_total):
            f.write("0\n" if i % 7 == 0 else "1\n")
    with open(prefix + ".keep5", "w") as f:
        for i in range(n_total):
            f.write("1\n" if i in (4, 5, 6, 8) else "0\n")   # n = 4 with c = 3: df = 0
    return prefix


def test_cli_assoc_dry_run_under_asan_ubsan(tmp_path):
    """--assoc --dry-run: the parsing, the matching by FID + IID and the QR, with the sample it prints."""
    exe = _built(CSRC, "sanitize", os.path.join(BIN, "dbslmm_asan"))
    pre = write_panel(tmp_path)
    out = str(tmp_path / "o")
    r = _run(exe, ["--assoc", "-r", pre, "--out", out, "--dry-run"])
    assert _clean(r) and r.returncode == 0 and "dry-run: n 39 c 1 P 1" in r.stdout, r.stdout + r.stderr[-3000:]
    # 38 lines in --pheno, one NA in its column 2, 6 of 40 not kept (0 and 35 of them already absent / 7 .. 28)
    r = _run(exe, ["--assoc", "-r", pre, "--out", out, "--pheno", pre + ".pheno", "--pheno-col", "1,2", "--covar",
                   pre + ".covar", "--keep", pre + ".keep", "--dry-run"])
    keep = [i for i in range(40) if i % 7 and i >= 2 and i != 9]
    assert _clean(r) and r.returncode == 0 and f"dry-run: n {len(keep)} c 3 P 2" in r.stdout, r.stdout + r.stderr[-3000:]
    r = _run(exe, ["--assoc", "-r", pre + "," + pre, "--out", out, "--dry-run"])
    assert _clean(r) and r.returncode == 0 and "24 rows" in r.stdout, r.stdout + r.stderr[-3000:]
    assert not os.path.exists(out + ".assoc.txt")


def test_cli_assoc_argument_errors_under_asan_ubsan(tmp_path):
    exe = _built(CSRC, "sanitize", os.path.join(BIN, "dbslmm_asan"))
    pre = write_panel(tmp_path)
    other = write_panel(tmp_path, "other", n_total=41)
    out = str(tmp_path / "o")
    for args, word in (
            (["--assoc", "-r", pre, "--dry-run"], "--out"),
            (["--assoc", "--out", out, "--dry-run"], "-r"),
            (["--assoc", "-r", pre, "--out", out, "--pheno", pre + ".pheno", "--pheno-col", "3", "--dry-run"], "--pheno-col"),
            (["--assoc", "-r", pre, "--out", out, "--pheno-col", "2", "--dry-run"], "--pheno-col"),
            (["--assoc", "-r", pre, "--out", out, "--pheno", pre + ".pheno", "--pheno-col", "x", "--dry-run"], "--pheno-col"),
            (["--assoc", "-r", pre, "--out", out, "--covar", pre + ".covar", "--keep", pre + ".keep5", "--dry-run"], "n - c - 1"),
            (["--assoc", "-r", pre, "--out", out, "--covar", pre + ".dupcovar", "--dry-run"], "rank"),
            (["--assoc", "-r", pre, "--out", out, "--keep", other + ".keep", "--dry-run"], "--keep"),
            (["--assoc", "-r", pre + "," + other, "--out", out, "--dry-run"], ".fam"),
            (["--assoc", "-r", pre, "--out", out, "--pheno", str(tmp_path / "none"), "--dry-run"], "exist"),
            (["--assoc", "-r", str(tmp_path / "none"), "--out", out, "--dry-run"], "exist"),
            (["--assoc", "-r", pre, "--out", out, "--maf-min", "0.7", "--dry-run"], "--maf-min"),
            (["--assoc", "-r", pre, "--out", out, "--miss-max", "-1", "--dry-run"], "--miss-max"),
            (["--assoc", "-r", pre, "--out", out, "-s", "x", "--dry-run"], "--assoc takes")):
        r = _run(exe, args)
        assert _clean(r), r.stderr[-3000:]
        assert r.returncode != 0 and word in r.stdout + r.stderr, (args, r.stdout, r.stderr[-500:])
