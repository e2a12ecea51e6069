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
