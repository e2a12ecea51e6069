"""`dbslmm --assoc` on the GPU: a training panel written by the test (300 individuals x 600 SNPs on one
chromosome, 1 % missing calls, two covariates, the .fam phenotype simulated as X beta + W gamma + e
from 5 causal rows, one planted monomorphic row) goes in, GEMMA's 11 columns come out, and the file
feeds `--summary / --pth` and `--ldsc` on the same panel with no other program in between."""
import os
import subprocess

import numpy as np
import pytest

import _assoc_ref as AR
from _common import ROOT

gpu = pytest.mark.gpu
CLI = os.path.join(ROOT, "dbslmm_amd", "bin", "dbslmm")
N, M = 300, 600
CAUSAL = (40, 150, 290, 410, 555)
MONO = 77


def run(args, cwd):
    return subprocess.run([CLI] + args, capture_output=True, text=True, cwd=cwd, timeout=300)


@pytest.fixture(scope="module")
def panel(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("assoc_cli"))
    rng = np.random.default_rng(11)
    g = rng.binomial(2, rng.uniform(0.2, 0.5, size=(M, 1)), size=(M, N)).astype(np.int8)
    m = rng.random((M, N)) < 0.01
    g[MONO], m[MONO] = 0, False
    w = rng.standard_normal((N, 2))
    y = g[list(CAUSAL)].T @ np.array([1.0, -1.0, 1.2, -0.9, 1.1]) + w @ [0.5, -0.7] + rng.standard_normal(N)
    y2 = rng.standard_normal(N)
    pre = os.path.join(d, "train")
    AR.encode(g, m).tofile(pre + ".bed")
    with open(pre + ".fam", "w") as f:
        for i in range(N):
            f.write(f"F{i} I{i} 0 0 1 {float(y[i])!r}\n")
    with open(pre + ".bim", "w") as f:
        for j in range(M):
            f.write(f"1\trs{j}\t0\t{1000 + 100 * j}\tA\tG\n")
    with open(pre + ".covar", "w") as f:
        for i in range(N):
            f.write(f"F{i} I{i} {float(w[i, 0])!r} {float(w[i, 1])!r}\n")
    with open(pre + ".pheno", "w") as f:
        for i in range(N):
            f.write(f"F{i} I{i} {float(y[i])!r} {float(y2[i])!r}\n")
    with open(pre + ".blocks", "w") as f:
        f.write("chr\tstart\tstop\n")
        for lo in range(0, 70000, 10000):
            f.write(f"chr1\t{lo}\t{lo + 10000}\n")
    return dict(dir=d, pre=pre, bed=AR.encode(g, m), y=y, y2=y2, w=w)


@pytest.fixture(scope="module")
def scan(panel):
    from dbslmm_amd import Context, assoc
    return assoc(Context(0), panel["bed"], N, np.column_stack([panel["y"], panel["y2"]]), panel["w"])


def read_assoc(path, header=False):
    lines = open(path).read().splitlines()
    if header:
        assert lines[0].split("\t") == "chr rs ps n_mis n_obs allele1 allele0 af beta se p_wald".split()
        lines = lines[1:]
    rows = [l.split("\t") for l in lines]
    assert all(len(r) == 11 for r in rows)
    return rows


def check_rows(rows, ref, q, precise):
    ok = np.flatnonzero(ref["status"] == 0)
    assert [r[1] for r in rows] == [f"rs{j}" for j in ok]
    for r, j in zip(rows, ok):
        assert r[0] == "1" and int(r[2]) == 1000 + 100 * j and r[5] == "A" and r[6] == "G"
        assert int(r[3]) == ref["n_mis"][j] and int(r[4]) == ref["n_obs"][j]
        want = (ref["af"][j], ref["beta"][q, j], ref["se"][q, j], ref["p"][q, j])
        got = [float(x) for x in r[7:]]
        if precise:
            assert tuple(got) == want, (j, got, want)
        else:
            assert abs(got[0] - want[0]) <= 5.0001e-4                      # %.3f
            assert all(abs(a - b) <= 5.0001e-7 * abs(b) for a, b in zip(got[1:], want[1:])), (j, got, want)   # %e


def held_to_the_reference(got, ref, ok, yard, what):
    """The bars of test_assoc.py: integers, status and af exact; beta (normwise per trait), se and T
    (elementwise) within max(32 x yardstick, 2^-48).  got may lack tstat (the file does not hold it)."""
    for k in ("n_mis", "n_obs", "status"):
        assert np.array_equal(got[k], ref[k]), (what, k)
    assert np.array_equal(np.isnan(got["af"]), np.isnan(ref["af"])), what
    assert np.array_equal(got["af"][ok].view(np.uint64), ref["af"][ok].view(np.uint64)), what
    keys = [k for k in ("beta", "se", "tstat") if k in got]
    dev = AR.deviation(got, ref, ok, keys)
    print(f"assoc cli {what}: yardstick beta {yard['beta']:.2e} se {yard['se']:.2e} T {yard['tstat']:.2e}; "
          + " ".join(f"{k} {dev[k]:.2e}" for k in keys) + f"; OK rows {int(ok.sum())}")
    for k in keys:
        assert np.all(np.isfinite(got[k][:, ok])) and dev[k] <= max(32 * yard[k], 2.0 ** -48), (what, k, dev[k], yard[k])


@gpu
def test_the_library_scan_of_the_panel_is_the_references(panel, scan):
    """The `scan` the CLI is compared with, held to tests/_assoc_ref.py on the module's 600 x 300 panel (38
    tiles in 10 workgroups, three finish blocks) with the bars of test_assoc.py; the preconditions
    (n_obs >= c + 2 and xPx / ssx >= 1e-3 on every OK row) are asserted from the reference first."""
    ref, ok, yard = AR.measured(panel["bed"], N, np.column_stack([panel["y"], panel["y2"]]), panel["w"])
    assert ref["status"][MONO] == AR.MONOMORPHIC and ok.sum() == M - 1
    held_to_the_reference(scan, ref, ok, yard, "600 x 300")
    assert np.all(np.isnan(scan["beta"][:, ~ok]))


def file_scan(paths, n_rows, names):
    """The outputs a set of --precise-out files (one per trait) holds, in the layout of `assoc`: rows absent
    from the files have status -1 and NaN."""
    P = len(paths)
    out = dict(n_mis=np.zeros(n_rows, dtype=np.int32), n_obs=np.zeros(n_rows, dtype=np.int32),
               status=np.full(n_rows, -1, dtype=np.int32), af=np.full(n_rows, np.nan),
               beta=np.full((P, n_rows), np.nan), se=np.full((P, n_rows), np.nan), p=np.full((P, n_rows), np.nan))
    at = {s: j for j, s in enumerate(names)}
    for q, path in enumerate(paths):
        for r in read_assoc(path):
            j = at[r[1]]
            assert q == 0 or (out["n_mis"][j], out["n_obs"][j], out["af"][j]) == (int(r[3]), int(r[4]), float(r[7]))
            out["n_mis"][j], out["n_obs"][j], out["status"][j], out["af"][j] = int(r[3]), int(r[4]), 0, float(r[7])
            out["beta"][q, j], out["se"][q, j], out["p"][q, j] = float(r[8]), float(r[9]), float(r[10])
    return out


@gpu
def test_assoc_two_panels_are_written_one_after_the_other(panel):
    """-r A,B with B a second panel of the same individuals (100 other rows, one monomorphic): A's lines, then
    B's, each half the single-panel run's line for line; .assoc.skipped lists both panels' rows in order;
    and B's half holds the reference's integers, af, beta and se."""
    d = panel["dir"]
    mb, mono_b = 100, 31
    rng = np.random.default_rng(12)
    g = rng.binomial(2, rng.uniform(0.2, 0.5, size=(mb, 1)), size=(mb, N)).astype(np.int8)
    m = rng.random((mb, N)) < 0.02
    g[mono_b], m[mono_b] = 2, rng.random(N) < 0.1
    pre_b = os.path.join(d, "second")
    bed_b = AR.encode(g, m)
    bed_b.tofile(pre_b + ".bed")
    with open(pre_b + ".fam", "w") as f:
        f.write(open(panel["pre"] + ".fam").read())
    with open(pre_b + ".bim", "w") as f:
        for j in range(mb):
            f.write(f"2\tsb{j}\t0\t{500 + 10 * j}\tC\tT\n")
    lines, skipped = {}, {}
    for key, r_arg in (("a", panel["pre"]), ("b", pre_b), ("ab", panel["pre"] + "," + pre_b)):
        out = os.path.join(d, "two_" + key)
        r = run(["--assoc", "-r", r_arg, "--out", out, "--covar", panel["pre"] + ".covar", "--precise-out"], d)
        assert r.returncode == 0, r.stdout + r.stderr
        lines[key] = open(out + ".assoc.txt").read().splitlines()
        skipped[key] = open(out + ".assoc.skipped").read().splitlines()
    assert len(lines["a"]) == M - 1 and len(lines["b"]) == mb - 1
    assert lines["ab"] == lines["a"] + lines["b"]
    assert skipped["ab"] == skipped["a"] + skipped["b"] == [f"rs{MONO}\tmonomorphic", f"sb{mono_b}\tmonomorphic"]
    ref, ok, yard = AR.measured(bed_b, N, panel["y"], panel["w"])
    names = [f"sb{j}" for j in range(mb)]
    got = file_scan([os.path.join(d, "two_b.assoc.txt")], mb, names)
    assert np.array_equal(got["status"] == 0, ok) and ref["status"][mono_b] == AR.MONOMORPHIC
    for k in ("n_mis", "n_obs"):
        got[k][~ok] = ref[k][~ok]                               # (skipped rows are not in the file)
    got["status"][~ok] = ref["status"][~ok]
    got["af"][~ok] = ref["af"][~ok]
    held_to_the_reference(got, ref, ok, yard, "second panel, 100 x 300")


@gpu
def test_assoc_sample_selection_reaches_the_scan(panel):
    """--keep, and --pheno with one NA, one -9, one individual without a line and one duplicate line (the
    first wins), with --covar: the printed n is the reference's, and the --precise-out files hold the
    integers and af of tests/_assoc_ref.py on the corresponding keep / NaN arrays, beta and se within the
    bars of test_assoc.py."""
    d = panel["dir"]
    rng = np.random.default_rng(13)
    keep = (rng.random(N) < 0.9).astype(np.uint8)
    keep[[0, 15, 16, 63, 64, 255, 256, N - 1]] = (0, 1, 0, 0, 1, 0, 1, 0)
    i_na, i_m9, i_absent, i_dup = (int(i) for i in np.flatnonzero(keep)[[10, 40, 90, 150]])
    Y = np.column_stack([panel["y"], panel["y2"]])
    with open(os.path.join(d, "sel.keep"), "w") as f:
        for i in range(N):
            f.write(f"{int(keep[i])}\n")
    with open(os.path.join(d, "sel.pheno"), "w") as f:
        for i in range(N):
            v = [repr(float(Y[i, 0])), repr(float(Y[i, 1]))]
            if i == i_absent:
                continue
            if i == i_na:
                v[0] = "NA"
            if i == i_m9:
                v[1] = "-9"
            f.write(f"F{i} I{i} {v[0]} {v[1]}\n")
        f.write(f"F{i_dup} I{i_dup} 99.5 NA\n")                 # a second line of i_dup, after its first: ignored
    Yn = Y.copy()
    Yn[i_na, 0] = Yn[i_m9, 1] = np.nan
    Yn[i_absent] = np.nan
    ref, ok, yard = AR.measured(panel["bed"], N, Yn, panel["w"], keep)
    n = ref["design"]["n"]
    assert n == int(keep.sum()) - 3
    out = os.path.join(d, "sel")
    r = run(["--assoc", "-r", panel["pre"], "--out", out, "--covar", panel["pre"] + ".covar", "--keep",
             os.path.join(d, "sel.keep"), "--pheno", os.path.join(d, "sel.pheno"), "--pheno-col", "1,2", "--precise-out"], d)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"assoc: n {n} of {N} individuals, c 3, P 2, {M} rows" in r.stdout, r.stdout
    got = file_scan([f"{out}.{q + 1}.assoc.txt" for q in (0, 1)], M, [f"rs{j}" for j in range(M)])
    assert np.array_equal(got["status"] == 0, ok)
    want = [f"rs{j}\t" + {AR.NO_CALL: "no_call", AR.MONOMORPHIC: "monomorphic", AR.COLLINEAR: "collinear"}[int(ref["status"][j])]
            for j in np.flatnonzero(~ok)]
    assert open(out + ".assoc.skipped").read().splitlines() == want and f"rs{MONO}\tmonomorphic" in want
    for k in ("n_mis", "n_obs", "status", "af"):
        got[k][~ok] = ref[k][~ok]                               # (skipped rows are not in the files)
    held_to_the_reference(got, ref, ok, yard, "keep + pheno + covar")


@gpu
def test_assoc_writes_gemmas_columns(panel, scan):
    out = os.path.join(panel["dir"], "a")
    r = run(["--assoc", "-r", panel["pre"], "--out", out, "--covar", panel["pre"] + ".covar"], panel["dir"])
    assert r.returncode == 0, r.stdout + r.stderr
    assert scan["status"][MONO] == 2 and np.sum(scan["status"] != 0) == 1
    check_rows(read_assoc(out + ".assoc.txt"), scan, 0, False)
    assert open(out + ".assoc.skipped").read().splitlines() == [f"rs{MONO}\tmonomorphic"]
    # the causal rows carry the smallest p-values
    p = {r[1]: float(r[10]) for r in read_assoc(out + ".assoc.txt")}
    assert set(sorted(p, key=p.get)[:5]) == {f"rs{j}" for j in CAUSAL}


@gpu
def test_assoc_precise_header_two_traits_and_filters(panel, scan):
    out = os.path.join(panel["dir"], "b")
    r = run(["--assoc", "-r", panel["pre"], "--out", out, "--covar", panel["pre"] + ".covar", "--pheno",
             panel["pre"] + ".pheno", "--pheno-col", "1,2", "--precise-out", "--assoc-header"], panel["dir"])
    assert r.returncode == 0, r.stdout + r.stderr
    assert not os.path.exists(out + ".assoc.txt")
    for q in (0, 1):
        path = f"{out}.{q + 1}.assoc.txt"
        assert len(open(path).read().splitlines()) == M - 1 + 1          # exactly one more line: the header
        check_rows(read_assoc(path, header=True), scan, q, True)
    # the filters: folded af and missing fraction, each skipped row with its reason
    out = os.path.join(panel["dir"], "c")
    r = run(["--assoc", "-r", panel["pre"], "--out", out, "--covar", panel["pre"] + ".covar", "--maf-min", "0.3",
             "--miss-max", "0.015"], panel["dir"])
    assert r.returncode == 0, r.stdout + r.stderr
    maf = np.minimum(scan["af"], 1 - scan["af"])
    want = {}
    for j in range(M):
        if scan["status"][j] != 0:
            want[f"rs{j}"] = "monomorphic"
        elif maf[j] < 0.3:
            want[f"rs{j}"] = "maf"
        elif scan["n_mis"][j] / N > 0.015:
            want[f"rs{j}"] = "missing"
    got = dict(l.split("\t") for l in open(out + ".assoc.skipped").read().splitlines())
    assert got == want and {"maf", "missing", "monomorphic"} <= set(want.values())
    assert [r[1] for r in read_assoc(out + ".assoc.txt")] == [f"rs{j}" for j in range(M) if f"rs{j}" not in want]


@gpu
def test_assoc_file_feeds_the_summary_run_and_ldsc(panel):
    d = panel["dir"]
    out = os.path.join(d, "r")
    r = run(["--assoc", "-r", panel["pre"], "--out", out, "--covar", panel["pre"] + ".covar"], d)
    assert r.returncode == 0, r.stdout + r.stderr
    summ = out + ".assoc.txt"
    n_lines = len(open(summ).read().splitlines())
    assert n_lines == M - 1
    eff = os.path.join(d, "eff")
    r = run(["--summary", summ, "--pth", "1e-4", "-r", panel["pre"], "-b", panel["pre"] + ".blocks", "-n", str(N), "-nsnp",
             str(n_lines), "-h", "0.5", "-mafMax", "1", "-eff", eff], d)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [l.split() for l in open(eff + ".txt").read().splitlines()]
    assert len(rows) == n_lines and len({x[0] for x in rows}) == n_lines       # one line per matched SNP
    large = {x[0] for x in rows if x[4] == "1"}
    assert {f"rs{j}" for j in CAUSAL} <= large and len(large) < 30
    assert all(np.isfinite(float(x[2])) for x in rows)
    l = os.path.join(d, "l")
    r = run(["--ldsc", "--summary", summ, "-r", panel["pre"], "--out", l], d)
    assert r.returncode == 0, r.stdout + r.stderr
    h2 = dict(x.split()[:2] for x in open(l + ".h2.txt").read().splitlines())
    assert np.isfinite(float(h2["h2"]))
