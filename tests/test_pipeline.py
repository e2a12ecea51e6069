"""The one-binary pipeline on a three-chromosome panel: `dbslmm --ldsc` (h2) and `dbslmm --summary /
--pth` (clump, split, solve) against the oracle composed in tests/_pipeline_ref.py, whose docstring
describes the panel and the summary.  What only test_dat covered before: candidate selection by erfc,
the |z| priority with ties by summary line, chromosome codes by first appearance, the hand-off of the
index SNPs into match_ref / add_block, .badsnps flag 1 for a rejected index SNP, the per-line N, the
first-summary-line rule, nan rows of the .l2.ldscore and M_5_50 with missing calls.

No tolerance is set here: the clump is compared whole (the oracle's margin >= MIN_MARGIN is asserted
first, from exact integers), effect files byte for byte against the split run and at the 1e-10
normwise bar of test_cli_filters_multichrom_match_oracle against the reference's direct solve, LD
scores at l2_bar + the file's %.10g, the regression at the rtol 1e-6 of test_cli_ldsc_on_test_dat.
The CPU tests assert the panel's properties from the oracle alone."""
import math
import os

import numpy as np
import pytest

import _clump_ref as CR
import _ldsc_ref as LR
import _pipeline_ref as PR
import ref_numpy as R
from test_cli import run
from test_clump import MIN_MARGIN
from test_ldsc import _h2_file, l2_bar

gpu = pytest.mark.gpu
LD = np.longdouble
CLUMPS = {"default": ([], 0.2, 1000.0), "r2 0.5, 250 kb": (["--clump-r2", "0.5", "--clump-kb", "250"], 0.5, 250.0)}


@pytest.fixture(scope="module")
def P(tmp_path_factory):
    return PR.build_panel(str(tmp_path_factory.mktemp("panel")))


_cache = {}


def summary_oracle(P, name="default", pth=PR.PTH):
    key = (id(P), name, pth)
    if key not in _cache:
        _cache[key] = PR.SummaryOracle(P, pth, CLUMPS[name][1], CLUMPS[name][2])
    return _cache[key]


def ldsc_oracle(P):
    key = (id(P), "ldsc")
    if key not in _cache:
        _cache[key] = PR.LdscOracle(P, l2_bar)
    return _cache[key]


def solve_args(P, h="0.5"):
    return ["-r", P.ref, "-b", P.blocks, "-n", str(PR.N_OBS), "-nsnp", str(P.n_lines), "-h", h, "-mafMax", "0.2",
            "--precise-out"]


def chains(S):
    """(A, B, C): A an index SNP that absorbed B, C a later index SNP linked to B and not to A"""
    out = []
    for B in range(len(S.index_of)):
        A = int(S.index_of[B])
        if A != B:
            out += [(A, B, int(C)) for C in np.flatnonzero(S.link[B]) if S.index_of[C] == C and C > A and not S.link[A, C]]
    return out


# ------------------------------------------------------------------------------------------------
# CPU: the panel is what the GPU cases need
# ------------------------------------------------------------------------------------------------
def test_panel_and_summary_have_the_properties_they_claim(P):
    X, chrom = P.X, P.chrom
    assert X.shape == (P.n_rows, PR.N_REF) and 2300 < P.n_rows <= 2400
    assert PR.N_REF % 4 != 0 and -(-PR.N_REF // 256) * 256 == 768                # pad bits; kpad 768: three K stages
    assert list(dict.fromkeys(chrom)) == [19, 20, 21]
    nmiss = (X < 0).sum(axis=1)
    with_missing = np.flatnonzero(nmiss > 0)
    c21 = np.flatnonzero(chrom == 21)
    assert np.all(nmiss[chrom == 19] == 0) and np.mean(nmiss[chrom == 20] > 0) > 0.99
    in21 = [r for r in with_missing if chrom[r] == 21 and r != P.allmiss]
    assert 90 <= len(in21) <= 100 and max(in21) - min(in21) < 100 and min(in21) > c21[0] + 128 and max(in21) < c21[-1] - 128
    rate = (X[chrom == 20] < 0).mean()
    assert 0.008 < rate < 0.012
    assert np.all(X[P.mono] == 2) and np.all(X[P.allmiss] == -1) and chrom[P.mono] == 19 and chrom[P.allmiss] == 21
    bim = [l.split("\t") for l in open(P.ref + ".bim").read().splitlines()]
    ids = [b[1] for b in bim]
    assert len(bim) == P.n_rows and 3 <= len(ids) - len(set(ids)) <= 6           # duplicate .bim ids
    # the block file: the reference's blocks of the three chromosomes without one in the middle of chromosome 20
    blocks = R.read_block(P.blocks)
    b20 = [b for b in blocks if b[0] == "chr20"]
    assert (f"chr{P.removed[0]}", P.removed[1], P.removed[2]) not in blocks and P.removed[0] == 20
    assert b20[0][1] < P.removed[1] and P.removed[2] < b20[-1][2]
    # the summary
    lines = [l.split("\t") for l in open(P.summ).read().splitlines()]
    assert len(lines) == P.n_lines == P.n_rows + 1 and all(len(l) == 11 for l in lines)
    first = {}
    for b in bim:
        first.setdefault(b[1], b)
    n = len(lines)
    swapped = sum(l[1] in first and (l[5], l[6]) == (first[l[1]][5], first[l[1]][4]) for l in lines)
    wrong_a2 = sum(l[1] in first and l[5] == first[l[1]][4] and l[6] != first[l[1]][5] for l in lines)
    absent = [l for l in lines if l[1] not in first]
    assert 0.02 * n < swapped < 0.04 * n and 0.005 * n < wrong_a2 < 0.02 * n and 0.005 * n < len(absent) < 0.02 * n
    N = np.array([int(l[4]) for l in lines])
    assert int((N == 0).sum()) == 1 and N[P.zero_n] == 0 and np.all((N[N > 0] >= 90000) & (N[N > 0] < 100000))
    assert len(set(N)) > 2000
    np.testing.assert_allclose([float(l[9]) for l, nn in zip(lines, N) if nn > 0], 1 / np.sqrt(N[N > 0]), rtol=1e-6)
    summ = R.read_summ(P.summ)
    assert any(math.erfc(abs(s.z) / math.sqrt(2)) <= PR.PTH for s in summ if s.snp not in first)   # an absent id with p <= pth
    a, b = P.tie
    assert b == a + 1 and lines[a][8:10] == lines[b][8:10] and lines[a][1] != lines[b][1]
    d0, d1 = P.dup
    assert lines[d0][1] == lines[d1][1] and [l[1] for l in lines].count(lines[d0][1]) == 2
    assert lines[d0][8] != lines[d1][8] and lines[d0][4] != lines[d1][4]            # which line counts matters
    # no MAF on the M_5_50 threshold
    import oracle as O
    maf = O.bed_maf(P.bed, PR.N_REF, P.n_rows)
    assert not np.any(np.abs(maf - 0.05) < 1e-9)


@pytest.mark.parametrize("name", list(CLUMPS))
def test_the_oracles_clump_has_the_properties_the_gpu_cases_claim(P, name):
    S = summary_oracle(P, name)
    c = S.cand
    n = len(c["snp"])
    assert n >= 100 and S.margin >= MIN_MARGIN, (n, S.margin)
    assert np.all(np.diff(np.abs(c["z"])) <= 0) and np.all(c["p"] <= PR.PTH)
    assert set(c["chrom"][S.index]) == {0, 1, 2}                                  # an index SNP on every chromosome
    # raw and four-product tiles each decide an in-window candidate pair
    fp = PR.clump_tiles_four_product((S.Xc < 0).sum(axis=1), c["chrom"], c["bp"])
    assert (fp & S.window).any() and (~fp & S.window).any()
    # the tie: neighbours in priority, the earlier summary line first
    k = [i for i in range(n) if c["line"][i] in P.tie]
    assert len(k) == 2 and k[1] == k[0] + 1 and abs(c["z"][k[0]]) == abs(c["z"][k[1]]) and c["line"][k[0]] < c["line"][k[1]]
    Nm, den = CR.pair_integers(S.Xc[k])
    assert CR.ge_threshold(Nm, den, 0.2)[0, 1]                                    # r2 of the tied rows >= 0.2
    assert S.index_of[k[0]] == k[0]
    # the hand-off: an index SNP match_ref rejects for its alleles, one outside every block of its chromosome
    blocks, inter_s, inter_l, info_s, info_l, bad = S.host(0.2)
    index_snps = [c["snp"][i] for i in S.index]
    assert P.swapped_causal in index_snps and f"{P.swapped_causal} 1" in bad
    assert P.absent_causal not in c["snp"]
    row_chr = {s: f"chr{ch}" for s, ch in zip(P.snp, P.chrom)}
    outside = [e["snp"] for e in inter_l if not any(b[0] == row_chr[e["snp"]] and b[1] <= e["ps"] < b[2] for b in blocks)]
    assert outside and all(P.removed[1] <= e["ps"] < P.removed[2] for e in inter_l if e["snp"] in outside)
    assert 0 < len(info_l) < len(inter_l) and 1000 < len(info_s) < len(inter_s)   # the scan stalls at the removed block
    assert sum(x.endswith(" 1") for x in bad) >= 1 and sum(x.endswith(" 0") for x in bad) > 50
    if name == "default":
        assert n - len(S.index) >= 40                                             # absorbed candidates
        assert S.index_of[k[1]] == k[0]                                           # the tie decides who is the index SNP
        assert len(chains(S)) >= 1
        wide = S.index
        assert wide != summary_oracle(P, "r2 0.5, 250 kb").index                  # the options change the answer
    print(f"{name}: {n} candidates, {len(S.index)} index SNPs, margin {S.margin:.2e}, {len(chains(S))} chains, "
          f"{len(info_l)} of {len(inter_l)} large and {len(info_s)} of {len(inter_s)} small SNPs in blocks")


def test_the_oracles_ld_scores_have_the_properties_the_gpu_case_claims(P):
    L = ldsc_oracle(P)
    assert sorted(np.flatnonzero(L.nan_row)) == sorted([P.mono, P.allmiss])
    assert L.uses_fp.sum() > 500 and (~L.uses_fp & ~L.nan_row).sum() > 500        # rows of both tile kinds
    ok = ~L.nan_row
    assert float(np.max(L.bar[ok] / L.l2[ok])) < 1e-9                             # the bar says something
    td = L.td
    assert list(dict.fromkeys(td["chrom"])) == [0, 1, 2] and np.all(np.diff(td["chrom"]) >= 0)
    # the regression set: the N = 0 line, the second line of the duplicated SNP and the NaN rows stay out
    lines = [l.split("\t") for l in open(P.summ).read().splitlines()]
    used = set(td["summ_of"][L.reg])
    assert P.zero_n not in used and P.dup[0] in used and P.dup[1] not in used
    assert L.named[P.mono] and L.named[P.allmiss] and int(L.named.sum()) == len(L.reg) + 2
    assert len({lines[s][4] for s in used}) > 2000                                # a sample size per line
    assert 0 < L.M < int(ok.sum())
    for kw in (dict(), dict(intercept=1.0), dict(chisq_max=30.0)):
        f = L.fit(**kw)
        assert f["status"] == 0 and (f["n"] == len(L.reg)) == ("chisq_max" not in kw), (kw, f)
    assert 0 < L.fit()["h2"] <= 1                      # the h2 of the free fit can go to -h as it is


def test_dry_runs_print_the_oracles_counts(P, tmp_path):
    S = summary_oracle(P)
    base = ["-r", P.ref, "-b", P.blocks, "-n", str(PR.N_OBS), "-nsnp", str(P.n_lines), "-h", "0.5", "-mafMax", "1",
            "--dry-run", "-eff", str(tmp_path / "o")]
    r = run(["--summary", P.summ, "--pth", "1e-6"] + base, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    assert f"dry-run: {len(S.cand['snp'])} candidates at pth 1e-06; stops before the clump" in r.stdout, r.stdout
    r = run(["--summary", P.summ, "--pth", "1e-300"] + base, cwd=str(tmp_path))
    assert r.returncode == 0 and "dry-run: 0 candidates" in r.stdout
    td = LR.test_dat_inputs(P.summ, P.ref)
    r = run(["--ldsc", "--summary", P.summ, "-r", P.ref, "--out", str(tmp_path / "l"), "--ld-wind-kb", str(PR.LD_WIND_KB),
             "--dry-run"], cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    n_reg = int((td["summ_of"] >= 0).sum())
    assert 2300 < n_reg < P.n_rows
    assert f"dry-run: {P.n_rows} rows, {n_reg} regression SNPs; stops before the LD scores" in r.stdout, r.stdout


# ------------------------------------------------------------------------------------------------
# GPU: dbslmm --summary
# ------------------------------------------------------------------------------------------------
def _eff(path):
    rows = [x.split() for x in open(path).read().splitlines()]
    return [(x[0], x[1], x[4]) for x in rows], np.array([float(x[2]) for x in rows])


def check_summary_run(P, S, tmp, extra, h="0.5", tag="a"):
    """one --summary run against the oracle S: the split run's bytes, the oracle's rows and betas, the
    clumped list, .badsnps and the count; returns the run's files' bytes"""
    tmp = str(tmp)
    assert S.margin >= MIN_MARGIN, S.margin
    common = solve_args(P, h)
    a = run(["--summary", P.summ, "--pth", "1e-6", "-eff", os.path.join(tmp, tag)] + extra + common, cwd=tmp)
    assert a.returncode == 0, a.stderr
    assert f"Using 1e-06, {len(S.index)} SNPs are regarded as fixed effect." in a.stdout, a.stdout
    s_path, l_path = S.split(tmp)
    b = run(["-s", s_path, "-l", l_path, "-eff", os.path.join(tmp, tag + "_split")] + common, cwd=tmp)
    assert b.returncode == 0, b.stderr
    files = {ext: open(os.path.join(tmp, tag + ext), "rb").read() for ext in (".txt", ".clumped.txt", ".badsnps")}
    assert len(files[".txt"]) > 0 and files[".txt"] == open(os.path.join(tmp, tag + "_split.txt"), "rb").read()
    # the reference's direct solve on the oracle's split
    blocks, inter_s, inter_l, info_s, info_l, bad = S.host(0.2)
    assert f"After filtering, {len(inter_s)} small effect SNPs are selected." in a.stdout
    assert f"After filtering, {len(inter_l)} large effect SNPs are selected." in a.stdout
    res = S.est(float(h))
    keys, got = _eff(os.path.join(tmp, tag + ".txt"))
    rows_e = [x.split() for x in R.format_eff(res)]
    assert len(rows_e) == len(info_s) + len(info_l) and keys == [(x[0], x[1], x[4]) for x in rows_e]
    ref = np.concatenate([res.beta_l, res.beta_s])
    worst = float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))
    print(f"--summary {extra} -h {h}: {len(S.index)} index SNPs, {len(keys)} rows, normwise |dbeta| {worst:.2e} (bar 1e-10)")
    assert worst <= 1e-10
    # <eff>.clumped.txt: the index SNPs in priority order
    c = S.cand
    lines = [l.split() for l in files[".clumped.txt"].decode().splitlines()]
    assert lines[0] == ["SNP", "CHR", "BP", "Z", "P", "N_ABSORBED"]
    assert [l[0] for l in lines[1:]] == [c["snp"][k] for k in S.index]
    assert [int(l[5]) for l in lines[1:]] == S.n_absorbed
    assert [int(l[2]) for l in lines[1:]] == [int(c["bp"][k]) for k in S.index]
    assert [l[1] for l in lines[1:]] == [str(P.chrom[c["row"][k]]) for k in S.index]
    tie = [i for i, k in enumerate(S.index) if c["line"][k] in P.tie]
    assert tie and c["line"][S.index[tie[0]]] == P.tie[0]               # the tie went to the earlier line
    # .badsnps: the oracle's, the rejected index SNP flagged 1
    got_bad = files[".badsnps"].decode().splitlines()
    assert got_bad == bad and f"{P.swapped_causal} 1" in got_bad
    return files


@gpu
@pytest.mark.parametrize("name", list(CLUMPS))
def test_cli_summary_on_three_chromosomes(P, name, tmp_path):
    check_summary_run(P, summary_oracle(P, name), tmp_path, CLUMPS[name][0])


@gpu
def test_cli_summary_without_a_significant_snp(P, tmp_path):
    """--pth 1e-300: no candidate, "no significant SNPs", the effect file of a -s run of the whole summary"""
    assert len(summary_oracle(P, pth=1e-300).cand["snp"]) == 0
    common = solve_args(P)
    a = run(["--summary", P.summ, "--pth", "1e-300", "-eff", str(tmp_path / "a")] + common, cwd=str(tmp_path))
    assert a.returncode == 0, a.stderr
    assert "Using 1e-300, no significant SNPs." in a.stdout and "regarded as fixed effect" not in a.stdout, a.stdout
    b = run(["-s", P.summ, "-eff", str(tmp_path / "b")] + common, cwd=str(tmp_path))
    assert b.returncode == 0, b.stderr
    ea = open(str(tmp_path / "a.txt"), "rb").read()
    assert len(ea) > 0 and ea == open(str(tmp_path / "b.txt"), "rb").read()
    assert open(str(tmp_path / "a.clumped.txt")).read().splitlines() == ["SNP CHR BP Z P N_ABSORBED"]
    assert open(str(tmp_path / "a.badsnps"), "rb").read() == open(str(tmp_path / "b.badsnps"), "rb").read()


@gpu
def test_cli_summary_gpu_ids_write_the_same_files(P, tmp_path):
    """--gpu-ids 0,0,0: the clump on the first context, the blocks sharded over three: the bytes of one device"""
    common = solve_args(P)
    out = []
    for extra, tag in (([], "one"), (["--gpu-ids", "0,0,0"], "three")):
        r = run(["--summary", P.summ, "--pth", "1e-6", "-eff", str(tmp_path / tag)] + extra + common, cwd=str(tmp_path))
        assert r.returncode == 0, r.stderr
        out.append([open(str(tmp_path / (tag + ext)), "rb").read() for ext in (".txt", ".clumped.txt", ".badsnps")])
    assert "Sharding the LD blocks over 3 GPUs" in r.stdout
    assert all(len(x) > 0 for x in out[0]) and out[0] == out[1]


# ------------------------------------------------------------------------------------------------
# GPU: dbslmm --ldsc, and its h2 fed to the solve
# ------------------------------------------------------------------------------------------------
def run_ldsc(P, tmp, extra, tag="o"):
    out = os.path.join(str(tmp), tag)
    r = run(["--ldsc", "--summary", P.summ, "-r", P.ref, "--out", out, "--ld-wind-kb", str(PR.LD_WIND_KB)] + extra,
            cwd=str(tmp))
    assert r.returncode == 0, r.stderr
    return out


LDSC_RUNS = {"free": ([], {}), "fixed": (["--intercept", "1"], dict(intercept=1.0)),
             "free, chisq-max": (["--chisq-max", "30"], dict(chisq_max=30.0)),
             "fixed, chisq-max": (["--intercept", "1", "--chisq-max", "30"], dict(intercept=1.0, chisq_max=30.0))}


@gpu
@pytest.mark.parametrize("name", list(LDSC_RUNS))
def test_cli_ldsc_on_three_chromosomes(P, name, tmp_path):
    L = ldsc_oracle(P)
    extra, kw = LDSC_RUNS[name]
    out = run_ldsc(P, tmp_path, extra)
    lines = [l.split("\t") for l in open(out + ".l2.ldscore").read().splitlines()]
    assert lines[0] == ["CHR", "SNP", "BP", "L2"] and len(lines) == 1 + P.n_rows
    assert [l[0] for l in lines[1:]] == [str(c) for c in P.chrom] and [l[1] for l in lines[1:]] == P.snp
    assert [int(l[2]) for l in lines[1:]] == list(P.bp)
    assert [l[3] == "nan" for l in lines[1:]] == list(L.nan_row)                  # nan exactly on the oracle's NaN rows
    got = np.array([float(l[3]) for l in lines[1:]])
    ok = ~L.nan_row
    err = np.abs(got.astype(LD) - L.l2)
    lim = L.bar + LD(1e-9) * np.abs(L.l2)
    worst = {k: float(np.max(err[s] / lim[s])) for k, s in (("raw", ok & ~L.uses_fp), ("four-product", ok & L.uses_fp))}
    print(f"--ldsc {name}: worst |got - ref| / (bar + 1e-9 l) {worst}")
    assert np.all(err[ok] <= lim[ok]), worst
    assert int(open(out + ".l2.M_5_50").read()) == L.M
    fit = L.fit(**kw)
    assert fit["status"] == 0
    h = _h2_file(out + ".h2.txt")
    np.testing.assert_allclose([float(v) for v in h["h2"]], [fit["h2"], fit["h2_se"]], rtol=1e-6)
    if "intercept" in kw:
        assert h["intercept"] == ["1", "fixed"]
    else:
        np.testing.assert_allclose([float(v) for v in h["intercept"]], [fit["intercept"], fit["intercept_se"]], rtol=1e-6)
    assert int(h["M"][0]) == L.M and int(h["n_snp"][0]) == fit["n"]
    assert (fit["n"] == len(L.reg)) == ("chisq_max" not in kw)
    np.testing.assert_allclose(float(h["mean_chi2"][0]), fit["mean_chi2"], rtol=1e-6)


@gpu
def test_cli_h2_of_ldsc_feeds_the_summary_run(P, tmp_path):
    """the chain a user runs: h2 of `--ldsc` as -h of `--summary`.  The text of the .h2.txt goes to -h; were
    the simulated value outside (0, 1] it would be clamped to it here (on this panel it is 0.043 and is
    not); the run is compared with the oracle at that h."""
    out = run_ldsc(P, tmp_path, [])
    text = _h2_file(out + ".h2.txt")["h2"][0]
    if 0 < float(text) <= 1:
        np.testing.assert_allclose(float(text), ldsc_oracle(P).fit()["h2"], rtol=1e-6)
    else:
        text = "1" if float(text) > 1 else "1e-4"
    check_summary_run(P, summary_oracle(P), tmp_path, [], h=text, tag="chain")
