"""Clumping without a GPU: the oracle's self-checks (tests/_clump_ref.py), the preconditions of the
GPU cases of tests/test_clump.py worked out from the exact integers, the stand-alone sanitizer
program over clump_layout.hpp, and the CLI's argument errors through --dry-run."""
import os
import subprocess

import numpy as np
import pytest

import _clump_ref as CR
from _common import BLOCKS_EUR1, ROOT, TD, load_bed
from test_sanitizers import BIN, _built, _clean, _run

SUMM = os.path.join(TD, "summary_gemma_chr1.assoc.txt")
REF = os.path.join(TD, "ref_chr1")
CLI = os.path.join(ROOT, "dbslmm_amd", "bin", "dbslmm")


@pytest.fixture(scope="module")
def td():
    bed = load_bed(REF + ".bed")
    c = CR.summary_candidates(SUMM, REF + ".bim", 1e-6)
    X = CR.decode(bed, 400, c["row"])
    return c, X, CR.pair_integers(X)


def test_oracle_r2_is_the_squared_correlation_of_the_imputed_dosages():
    """r2 from the exact integers against numpy's corrcoef of the mean-imputed rows (fp64: 1e-12),
    NaN for rows without variance or observed call; encode / decode round trip at n % 4 != 0"""
    rng = np.random.default_rng(0)
    X = rng.integers(-1, 3, size=(9, 203)).astype(np.int8)
    X[3] = 2
    X[4] = -1
    X[5, X[5] >= 0] = 1
    np.testing.assert_array_equal(CR.decode(CR.encode(X), 203, np.arange(9)), X)
    r2 = CR.r2_longdouble(X).astype(np.float64)
    xs = np.where(X < 0, np.nan, X).astype(np.float64)
    ok = [0, 1, 2, 6, 7, 8]
    mu = np.nanmean(xs[ok], axis=1, keepdims=True)
    ref = np.corrcoef(np.where(np.isnan(xs[ok]), mu, xs[ok])) ** 2
    assert np.max(np.abs(r2[np.ix_(ok, ok)] - ref)) < 1e-12
    for r in (3, 4, 5):
        assert np.all(np.isnan(r2[r])) and np.all(np.isnan(r2[:, r]))
    Nm, den = CR.pair_integers(X)
    assert not CR.ge_threshold(Nm, den, 1e-300)[3].any()          # NaN compares false
    assert CR.ge_threshold(Nm, den, 1.0)[0, 0]                     # r2 = 1 exactly is >= 1


def test_oracle_on_test_dat(td):
    """444 candidates at pth 1e-6; the brute-force walk without a window equals the windowed one when
    the window covers the 300 kb span; a 50 kb window differs (a real band); deterministic; margins as
    measured (4.0e-5 at 0.2, 1.1e-4 at 0.1)."""
    c, X, pi = td
    assert len(c["snp"]) == 444 and np.all(X >= 0)
    assert int(c["bp"].max() - c["bp"].min()) < 1_000_000
    assert np.all(np.diff(np.abs(c["z"])) <= 0) and np.all(c["p"] <= 1e-6)
    for t, n_index in ((0.2, 27), (0.1, 20)):
        a, ma = CR.clump_ref(X, c["chrom"], c["bp"], t, 1_000_000, pairs_int=pi)
        b, mb = CR.clump_ref(X, c["chrom"], c["bp"], t, 1_000_000, brute=True, pairs_int=pi)
        np.testing.assert_array_equal(a, b)
        assert ma == mb and ma >= 1e-9
        assert int((a == np.arange(444)).sum()) == n_index
        again, _ = CR.clump_ref(X, c["chrom"], c["bp"], t, 1_000_000, pairs_int=pi)
        np.testing.assert_array_equal(a, again)
        assert np.all(a[a] == a) and np.all(a <= np.arange(444))  # absorbed by an earlier index SNP
    assert abs(CR.clump_ref(X, c["chrom"], c["bp"], 0.2, 1_000_000, pairs_int=pi)[1] - 4.0e-5) < 1e-6
    narrow, mn = CR.clump_ref(X, c["chrom"], c["bp"], 0.2, 50_000, pairs_int=pi)
    wide, _ = CR.clump_ref(X, c["chrom"], c["bp"], 0.2, 1_000_000, pairs_int=pi)
    assert mn >= 1e-9 and not np.array_equal(narrow, wide)


def test_priority_ties_break_by_summary_line(td):
    """candidates sharing |z| with another keep their summary order, and the order matters: walking
    the tied candidates in reverse changes the index set"""
    c, X, pi = td
    az = np.abs(c["z"])
    tied = np.flatnonzero(np.concatenate([[False], az[1:] == az[:-1]]))
    assert len(tied) >= 2
    for k in tied:
        assert c["line"][k - 1] < c["line"][k]
    base, _ = CR.clump_ref(X, c["chrom"], c["bp"], 0.2, 1_000_000, pairs_int=pi)
    # the same candidates with every run of equal |z| reversed
    perm = np.arange(444)
    k = 0
    while k < 444:
        e = k
        while e + 1 < 444 and az[e + 1] == az[k]:
            e += 1
        perm[k:e + 1] = perm[k:e + 1][::-1]
        k = e + 1
    rev, _ = CR.clump_ref(X[perm], c["chrom"][perm], c["bp"][perm], 0.2, 1_000_000)
    assert {c["snp"][i] for i in np.flatnonzero(base == np.arange(444))} != \
           {c["snp"][perm[i]] for i in np.flatnonzero(rev == np.arange(444))}


def test_absorption_is_not_transitive():
    """a hand-built panel: A - B and B - C are linked, A - C is not; in the order A, B, C the walk gives
    index SNPs A and C, in the order B, A, C only B"""
    # A and C are uncorrelated patterns over four groups of 10 individuals, B their mean:
    # r2(A, B) = r2(B, C) = 0.5, r2(A, C) = 0
    n = 40
    a = np.repeat(np.array([2, 2, 0, 0], dtype=np.int8), 10)
    c = np.repeat(np.array([2, 0, 2, 0], dtype=np.int8), 10)
    b = np.repeat(np.array([2, 1, 1, 0], dtype=np.int8), 10)
    X = np.stack([a, b, c])
    r2 = CR.r2_longdouble(X).astype(np.float64)
    assert r2[0, 1] >= 0.2 and r2[1, 2] >= 0.2 and r2[0, 2] < 0.2, r2
    chrom, bp = np.ones(3), np.array([100, 200, 300])
    idx, _ = CR.clump_ref(X, chrom, bp, 0.2, 1000)
    np.testing.assert_array_equal(idx, [0, 0, 2])
    idx, _ = CR.clump_ref(X[[1, 0, 2]], chrom, bp[[1, 0, 2]], 0.2, 1000)
    np.testing.assert_array_equal(idx, [0, 0, 0])
    idx, _ = CR.clump_ref(X, chrom, bp, 0.2, 50)                   # out of the window: three index SNPs
    np.testing.assert_array_equal(idx, [0, 1, 2])
    idx, _ = CR.clump_ref(X, np.array([1, 2, 1]), bp, 0.2, 1000)   # B on another chromosome
    np.testing.assert_array_equal(idx, [0, 1, 2])
    assert n == X.shape[1]


def test_synthetic_case_has_the_properties_it_claims():
    """the synthetic list of tests/test_clump.py: margin >= 1e-9, equal bp on two chromosomes, a band
    at least three tile columns wide, an empty stretch, priority unrelated to position, the chain"""
    from test_clump import SYN_WINDOW_KB, synthetic_candidates, synthetic_oracle
    _, X, rows, chrom, bp = synthetic_candidates()
    ref, margin = synthetic_oracle()
    assert margin >= 1e-9, margin
    assert set(bp[chrom == 2]) <= set(bp[chrom == 1])
    order = np.array(sorted(range(len(bp)), key=lambda k: (chrom[k], bp[k], k)))
    pos = np.empty(len(bp), dtype=np.int64)
    pos[order] = np.arange(len(bp))
    w = SYN_WINDOW_KB * 1000
    reach = max(int(pos[j] // 32 - pos[i] // 32) for i in range(len(bp)) for j in range(len(bp))
                if chrom[i] == chrom[j] and 0 < bp[j] - bp[i] <= w)
    assert reach >= 3
    c1 = np.sort(bp[chrom == 1])
    assert np.max(np.diff(c1)) > w                                  # the empty stretch
    assert abs(np.corrcoef(pos, np.arange(len(bp)))[0, 1]) < 0.2    # priority unrelated to position
    r2 = CR.r2_longdouble(X[:3]).astype(np.float64)
    assert r2[0, 1] >= 0.2 and r2[1, 2] >= 0.2 and r2[0, 2] < 0.2, r2
    assert list(ref[:3]) == [0, 0, 2]
    n_index = int((ref == np.arange(len(ref))).sum())
    assert 20 < n_index < len(ref) - 20                             # the walk absorbs and keeps plenty
    assert np.any(X < 0)


def test_clump_layout_under_asan_ubsan():
    """tests/host/clump_check.cpp: the band tile list, its indices and clump_greedy from first
    principles, under ASan + UBSan (a stand-alone program: no preloaded runtime)"""
    exe = _built(os.path.join(ROOT, "dbslmm_amd", "csrc"), "../bin/clump_asan", os.path.join(BIN, "clump_asan"))
    r = _run(exe, [])
    assert _clean(r), r.stderr[-3000:]
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stderr[-3000:]


# ------------------------------------------------------------------------------------------------
# CLI arguments (host only: --dry-run)
# ------------------------------------------------------------------------------------------------
BASE = ["-r", REF, "-b", BLOCKS_EUR1, "-n", "2400", "-nsnp", "996", "-h", "0.5", "-mafMax", "1", "--dry-run"]


def _cli(args, cwd):
    return subprocess.run([CLI] + args, capture_output=True, text=True, cwd=str(cwd), timeout=300)


@pytest.mark.parametrize("extra,msg", [
    (["--summary", SUMM, "--pth", "1e-6", "-s", SUMM], "--summary replaces -s / -l"),
    (["--summary", SUMM, "--pth", "1e-6", "-l", SUMM], "--summary replaces -s / -l"),
    (["--summary", SUMM], "--summary needs --pth"),
    (["--summary", SUMM, "--pth", "0"], "--pth must be in (0, 1]"),
    (["--summary", SUMM, "--pth", "1e-6", "--clump-r2", "1.5"], "--clump-r2 must be in (0, 1]"),
    (["--summary", "/nonexistent", "--pth", "1e-6"], "dose not exist"),
    (["-s", SUMM, "--pth", "1e-6"], "--pth needs --summary"),
])
def test_cli_summary_argument_errors(extra, msg, tmp_path):
    r = _cli(extra + BASE + ["-eff", str(tmp_path / "o")], tmp_path)
    assert r.returncode == 1 and msg in r.stderr, (r.returncode, r.stderr)


def test_cli_summary_host_path_under_asan_ubsan(tmp_path):
    """the host side of --summary (the .bim reader's chr / bp fields, p-values, the candidate sort)
    in the sanitizer build of the CLI, a stand-alone program"""
    exe = _built(os.path.join(ROOT, "dbslmm_amd", "csrc"), "sanitize", os.path.join(BIN, "dbslmm_asan"))
    r = _run(exe, ["--summary", SUMM, "--pth", "1e-6"] + BASE + ["-eff", str(tmp_path / "o")], cwd=str(tmp_path))
    assert _clean(r), r.stderr[-3000:]
    assert r.returncode == 0 and "dry-run: 444 candidates" in r.stdout, (r.returncode, r.stderr[-2000:])


def test_cli_summary_dry_run_stops_before_the_clump(tmp_path):
    """--dry-run parses, counts the candidates (as the oracle does) and says that it stops before the
    clump; nothing is written"""
    r = _cli(["--summary", SUMM, "--pth", "1e-6"] + BASE + ["-eff", str(tmp_path / "o")], tmp_path)
    assert r.returncode == 0, r.stderr
    n = len(CR.summary_candidates(SUMM, REF + ".bim", 1e-6)["snp"])
    assert f"dry-run: {n} candidates at pth 1e-06; stops before the clump" in r.stdout, r.stdout
    assert not os.path.exists(str(tmp_path / "o") + ".clumped.txt")
    r = _cli(["--summary", SUMM, "--pth", "1e-300"] + BASE + ["-eff", str(tmp_path / "o")], tmp_path)
    assert r.returncode == 0 and "dry-run: 0 candidates" in r.stdout
