"""Polygenic scores of a target panel from the solved betas (dbslmm_plan_score, Plan.score, tune_r2,
the CLI's --score).

Oracle: a NumPy restatement in this module.  For every SNP ref_numpy.read_snp_im gives the imputed
dosages of the selected individuals (missing -> the mean of the observed calls), then
  counts  score[c][t] = sum_j beta_jc w_j g'_tj
  std     score[c][t] = sum_j beta_jc w_j (g'_tj - mu'_j) / sd_j      (sd: N-1, over the selected)
with g' = 2 - g, mu' = 2 - mu for a flipped SNP, accumulated in np.longdouble.  A SNP is dropped for
copy c (contributes 0, counted) when its block's status is NOT_PD / MONOMORPHIC, beta w is not
finite, no selected call is observed, or (std) sd = 0 or n_test < 2.  The betas are those the same
GPU run returned, so only the scoring is under test.

Bar (derived, not measured), per individual and copy:
  |got - ref| <= 2 (M + 64) 2^-53 sum_j |a_jc| (|g_tj| + |mu_j|),   a = beta w (counts), beta w / sd (std)
M = the plan's SNPs: an FMA chain of M terms in any order plus the few roundings of a coefficient.
The bar must stay useful: every case checks bound <= 1e-11 max|score| (so the z-scores of the
non-driver SNPs are scaled down: a score of thousands of random-sign terms cancels to sqrt(M) of
its absolute sum and the bar of such a case would say little).  dropped must match exactly.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import ref_numpy as R
from _common import ROOT, TD, load_bed, pcg_case

LD = np.longdouble
CLI = os.path.join(ROOT, "dbslmm_amd", "bin", "dbslmm")
H2F = (0.8, 1.0, 1.2)


# ----------------------------------------------------------------------------- the restatement
class Panel:
    """The imputed dosages of the plan's SNPs (rows) over the selected individuals, compactly:
    code[j, t] in {0, 1, 2} or 255 (missing -> mu[j]); cnt = observed calls, const = sd is 0."""

    def __init__(self, tbed, n_total, indicator, rows):
        ind = np.ones(n_total, dtype=np.int32) if indicator is None else np.asarray(indicator, dtype=np.int32)
        assert ind.size == n_total
        sel = ind != 0
        self.n_test = int(sel.sum())
        nb = R.bytes_per_snp(n_total)
        M = len(rows)
        self.code = np.zeros((M, self.n_test), dtype=np.uint8)
        self.mu = np.zeros(M)
        self.cnt = np.zeros(M, dtype=np.int64)
        self.sd = np.ones(M, dtype=LD)
        self.const = np.zeros(M, dtype=bool)
        for j, r in enumerate(rows):
            g, _ = R.read_snp_im(tbed, int(r), ind)                       # imputed dosages
            miss = R.decode_codes(tbed[3 + int(r) * nb: 3 + (int(r) + 1) * nb], n_total)[sel] == 1
            self.cnt[j] = int((~miss).sum())
            if self.cnt[j] == 0:
                self.code[j] = 255                                        # (mu stays 0: the SNP is dropped)
                self.const[j] = True
                continue
            self.mu[j] = g[~miss].sum() / float(self.cnt[j])              # readSNPIm's imputation value
            assert not miss.any() or g[miss][0] == self.mu[j]
            self.code[j] = np.where(miss, 255, g).astype(np.uint8)
            gl = g.astype(LD)
            if self.n_test >= 2:
                self.sd[j] = np.sqrt(((gl - gl.mean()) ** 2).sum() / LD(self.n_test - 1))   # nomalizeVec
            self.const[j] = bool(np.all(g[~miss] == g[~miss][0])) or self.n_test < 2
            if self.const[j]:
                self.sd[j] = 1

    def ghat(self, j0, j1):
        c = self.code[j0:j1]
        return np.where(c == 255, self.mu[j0:j1, None], c.astype(np.float64))


def score_oracle(P, beta, ok, mode, w=None, flip=None, m_plan=None):
    """(ref[C, n_test] longdouble, dropped[C], bound[C, n_test]) for beta[C, M], ok[C, M] (the
    block's status lets the SNP count), per-SNP weights and flips."""
    beta = np.atleast_2d(np.asarray(beta, dtype=np.float64))
    C, M = beta.shape
    w = np.ones(M) if w is None else np.asarray(w, dtype=np.float64)
    flip = np.zeros(M, dtype=bool) if flip is None else np.asarray(flip) != 0
    with np.errstate(invalid="ignore", over="ignore"):
        bw = beta * w
    drop = ~np.asarray(ok, dtype=bool) | ~np.isfinite(bw) | (P.cnt == 0)[None, :]
    if mode == "std":
        drop = drop | (P.const | (P.n_test < 2))[None, :]
    a = np.where(drop, 0.0, bw).astype(LD)
    if mode == "std":
        a = a / P.sd[None, :]
    ref = np.zeros((C, P.n_test), dtype=LD)
    bsum = np.zeros((C, P.n_test), dtype=LD)
    for j0 in range(0, M, 256):
        j1 = min(M, j0 + 256)
        g = P.ghat(j0, j1).astype(LD)
        mu = P.mu[j0:j1].astype(LD)[:, None]
        f = flip[j0:j1, None]
        if mode == "std":
            x = np.where(f, (2 - g) - (2 - mu), g - mu)
        else:
            x = np.where(f, 2 - g, g)
        ref += a[:, j0:j1] @ x
        bsum += np.abs(a[:, j0:j1]) @ (np.abs(g) + np.abs(mu))
    bound = 2 * ((M if m_plan is None else m_plan) + 64) * LD(2.0) ** -53 * bsum
    return ref, drop.sum(axis=1).astype(np.int64), bound


def literal_scores(tbed, n_total, indicator, rows, beta, ok, mode, w, flip):
    """The same by a literal double loop over individuals and SNPs (plain Python floats)."""
    ind = np.ones(n_total, dtype=np.int32) if indicator is None else np.asarray(indicator)
    cols = [R.read_snp_im(tbed, int(r), ind)[0] for r in rows]
    n_test = int((ind != 0).sum())
    C, M = beta.shape
    out = np.zeros((C, n_test))
    dropped = np.zeros(C, dtype=np.int64)
    for c in range(C):
        for j in range(M):
            g = cols[j]
            bw = beta[c, j] * w[j]
            gone = (not ok[c, j]) or (not np.isfinite(bw)) or bool(np.all(np.isnan(g)))
            sd = 1.0
            if mode == "std" and not gone:
                sd = float(np.std(g, ddof=1)) if n_test >= 2 else 0.0
                gone = sd == 0.0
            if gone:
                dropped[c] += 1
        for t in range(n_test):
            acc = 0.0
            for j in range(M):
                g = cols[j]
                bw = beta[c, j] * w[j]
                if (not ok[c, j]) or (not np.isfinite(bw)) or bool(np.all(np.isnan(g))):
                    continue
                gt, mu = float(g[t]), float(np.mean(g))
                if flip[j]:
                    gt, mu = 2.0 - gt, 2.0 - mu
                if mode == "std":
                    sd = float(np.std(g, ddof=1)) if n_test >= 2 else 0.0
                    if sd == 0.0:
                        continue
                    acc += bw * (gt - mu) / sd
                else:
                    acc += bw * gt
            out[c, t] = acc
    return out, dropped


# ----------------------------------------------------------------------------- CPU tests
def test_restatement_equals_literal_double_loop_on_test_dat():
    from test_variance import td_indicator
    n_total = R.get_row(os.path.join(TD, "test_chr1.fam"))
    tbed = load_bed(os.path.join(TD, "test_chr1.bed"))
    ind = td_indicator(n_total)
    ind[40:] = 0                                       # (a literal Python loop: keep it to a few individuals)
    rng = np.random.default_rng(11)
    poly = [r for r in range((tbed.size - 3) // R.bytes_per_snp(n_total))
            if len(set(R.read_snp_im(tbed, r, ind)[0].tolist())) > 1]
    rows = rng.choice(poly, size=24, replace=False)
    tb = tbed.copy()
    nb = R.bytes_per_snp(n_total)
    tb[3 + rows[3] * nb: 3 + (rows[3] + 1) * nb] = 0x55            # every call missing: cnt = 0
    tb[3 + rows[5] * nb: 3 + (rows[5] + 1) * nb] = 0xAA            # every call heterozygous: sd = 0
    tb[3 + rows[7] * nb] = (tb[3 + rows[7] * nb] & 0xF0) | 0x05    # two missing calls: mean imputation
    beta = rng.standard_normal((2, 24))
    ok = np.ones((2, 24), dtype=bool)
    ok[1, 10:14] = False
    w = rng.uniform(0.5, 2.0, 24)
    w[2] = np.nan
    flip = rng.random(24) < 0.3
    flip[7] = True
    P = Panel(tb, n_total, ind, rows)
    assert P.cnt[3] == 0 and P.const[5] and P.cnt[7] < P.n_test
    for mode in ("counts", "std"):
        ref, dr, bound = score_oracle(P, beta, ok, mode, w, flip)
        lit, dl = literal_scores(tb, n_total, ind, rows, beta, ok, mode, w, flip)
        assert dr.tolist() == dl.tolist()
        assert dr.tolist() == ([2, 6] if mode == "counts" else [3, 7])
        assert np.all(np.abs(ref - lit) <= 1e-13 * np.abs(ref).max())
        assert np.all(bound > 0)


def test_tune_r2_equals_corrcoef_with_nans():
    from dbslmm_amd import tune_r2
    rng = np.random.default_rng(3)
    y = rng.standard_normal(57)
    sc = np.stack([0.2 * y + rng.standard_normal(57), 0.9 * y + rng.standard_normal(57), rng.standard_normal(57),
                   np.full(57, 1.5)])
    y[[4, 19, 33]] = np.nan
    ok = ~np.isnan(y)
    r2, best = tune_r2(sc, y)
    for c in range(3):
        assert abs(r2[c] - np.corrcoef(sc[c, ok], y[ok])[0, 1] ** 2) < 1e-14
    assert np.isnan(r2[3])                             # a constant score has no correlation
    assert best == int(np.argmax(r2[:3])) == 1
    with pytest.raises(ValueError):
        tune_r2(sc[:, :10], y)


def test_score_args_struct_matches_header():
    from dbslmm_amd import _lib
    src = open(os.path.join(ROOT, "include", "dbslmm_hip.h")).read()
    body = re.search(r"typedef struct dbslmm_score_args \{(.*?)\} dbslmm_score_args;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+);", body) == [f[0] for f in _lib.ScoreArgs._fields_]
    assert "dbslmm_plan_score" in _lib.EXPORTS
    assert (_lib.SCORE_COUNTS, _lib.SCORE_STD) == (0, 1)
    assert re.search(r"DBSLMM_SCORE_COUNTS = 0, DBSLMM_SCORE_STD = 1", src)


def test_cli_refuses_score_without_dat_str(tmp_path):
    r = subprocess.run([CLI, "-s", os.path.join(TD, "summary_gemma_chr1.assoc.txt"), "-r", os.path.join(TD, "ref_chr1"),
                        "-n", "2400", "-nsnp", "996", "-b", os.path.join(ROOT, "dbslmm_amd", "data", "block_data",
                                                                          "EUR", "chr1.bed"),
                        "-h", "0.5", "-t", "1", "-eff", str(tmp_path / "o"), "--score", str(tmp_path / "sc")],
                       capture_output=True, text=True)
    assert r.returncode != 0
    assert "--score" in r.stderr and "-dat_str" in r.stderr
    assert not os.path.exists(str(tmp_path / "sc") + ".score.txt")


# ----------------------------------------------------------------------------- GPU: cases
def _quiet(prob):
    """The z-scores of the non-driver SNPs scaled down (module docstring: a useful bar)."""
    prob.z_s[np.abs(prob.z_s) < 5.9] *= 0.02


_CASES = {}


def case(n_total=150, sel="ind", **kw):
    """pcg_case at n_total test individuals with selection sel: "all" (no indicator), "ones" (an
    explicit all-ones array), "ind" (pcg_case's 75 % indicator), "drop1" (all but one)."""
    c = pcg_case(n_total=n_total, **kw)
    _quiet(c.prob)
    c.n_total = n_total
    if sel in ("all", "ones"):
        c.ind = None if sel == "all" else np.ones(n_total, dtype=np.int32)
    elif sel == "drop1":
        c.ind = np.ones(n_total, dtype=np.int32)
        c.ind[n_total // 3] = 0
    c.rows = np.concatenate([c.ts_pos, c.tl_pos if c.tl_pos is not None else np.zeros(0, np.int32)])
    return c


def panel_of(c, tag=None):
    """The case's Panel, computed once per (panel, selection) and left unchanged."""
    key = tag or (c.n_total, None if c.ind is None else c.ind.tobytes(), c.rows.tobytes())
    if key not in _CASES:
        _CASES[key] = Panel(c.tbed, c.n_total, c.ind, c.rows)
    return _CASES[key]


def snp_block(prob):
    bs = np.repeat(np.arange(prob.num_block), np.diff(prob.s_ptr))
    bl = np.repeat(np.arange(prob.num_block), np.diff(prob.l_ptr)) if prob.l_ptr is not None else np.zeros(0, int)
    return np.concatenate([bs, bl]).astype(int)


def joint(prob, res):
    """run_multi's [(beta_s, beta_l, status)] -> beta[C, M], ok[C, M]."""
    from dbslmm_amd import BLOCK_MONOMORPHIC, BLOCK_NOT_PD
    blk = snp_block(prob)
    beta = np.stack([np.concatenate([r[0], r[1]]) for r in res])
    ok = np.stack([~np.isin(r[2][blk], (BLOCK_NOT_PD, BLOCK_MONOMORPHIC)) for r in res])
    return beta, ok


def sigmas(prob, f=H2F):
    return [prob.sigma_s * x for x in f]


def do_score(plan, c, **kw):
    return plan.score(c.tbed, c.ind, c.ts_pos, c.tl_pos, n_total=c.n_total, **kw)


def check(got, dropped, P, beta, ok, mode, w=None, flip=None, what="", useful=True):
    ref, dr, bound = score_oracle(P, beta, ok, mode, w, flip)
    assert got.shape == ref.shape, what
    assert np.all(np.isfinite(got)), what
    err = np.abs(got.astype(LD) - ref)
    ratio = float(np.max(err / np.maximum(bound, LD(1e-300))))
    use = float(bound.max() / np.abs(ref).max())
    print(f"score {what} {mode}: worst |got - ref| / bound = {ratio:.3g}, bound / max|score| = {use:.3g}")
    if dropped is not None:
        assert dropped.tolist() == dr.tolist(), what
    if useful:
        assert use <= 1e-11, (what, use)               # a bar that still says something
    assert np.all(err <= bound), (what, mode, ratio)
    return ref, bound


@pytest.fixture(scope="module")
def ctx():
    from dbslmm_amd import Context
    c = Context(0)
    yield c
    c.close()


PANELS = [(13, "all"), (150, "ind"), (4197, "all"), (4197, "drop1")]


@pytest.mark.gpu
@pytest.mark.parametrize("n_total,sel", PANELS)
def test_scores_match_the_oracle_after_run_multi(ctx, n_total, sel):
    """COUNTS and STD of three h2f copies on the PCG route: the library's chunk_slots and 96 (many
    chunks, boundaries inside blocks and inside padding), a repeat bit for bit, and no indicator
    against an explicit all-ones array bit for bit."""
    from dbslmm_amd import Plan
    c = case(n_total, sel)
    plan = Plan(ctx, c.prob)
    beta, ok = joint(c.prob, plan.run_multi(sigmas(c.prob)))
    assert plan.workload()["pcg_route"] == 1
    P = panel_of(c)
    assert P.n_test == (n_total if sel == "all" else int((c.ind != 0).sum()))
    for mode in ("counts", "std"):
        for cs in (0, 96):
            got, dr = do_score(plan, c, mode=mode, chunk_slots=cs)
            check(got, dr, P, beta, ok, mode, what=f"n={n_total} {sel} chunk={cs}")
            again, dr2 = do_score(plan, c, mode=mode, chunk_slots=cs)
            np.testing.assert_array_equal(got, again)
            np.testing.assert_array_equal(dr, dr2)
            assert plan.score_gpu_ms > 0.0
            if sel == "all":
                ones, _ = plan.score(c.tbed, np.ones(n_total, dtype=np.int32), c.ts_pos, c.tl_pos, mode=mode,
                                     chunk_slots=cs)
                np.testing.assert_array_equal(got, ones)
    plan.close()


@pytest.mark.gpu
def test_dropped_snps_contribute_nothing_and_are_counted(ctx):
    """A monomorphic block (its SNPs dropped for every copy: the score is the oracle's without that
    block); test-panel rows with a few missing calls (mean imputation), one missing for every
    selected individual (cnt = 0) and one constant over them (STD only); NaN and inf weights."""
    from dbslmm_amd import BLOCK_MONOMORPHIC, Plan
    c = case(150, "ind", mono_block=2)
    nb = R.bytes_per_snp(150)
    tb = c.tbed.copy()
    sel = np.flatnonzero(c.ind)

    def put(row, who, code):
        for i in who:
            o = 3 + int(row) * nb + i // 4
            tb[o] = (tb[o] & ~(3 << (2 * (i % 4))) & 0xFF) | (code << (2 * (i % 4)))
    put(c.ts_pos[10], sel[[0, 5, 17]], 1)               # a few missing calls
    put(c.ts_pos[900], sel[[3]], 1)
    put(c.tl_pos[3], sel[[2, 40]], 1)                   # ... of a large SNP too
    put(c.ts_pos[20], sel, 1)                           # no observed call among the selected
    put(c.ts_pos[1500], sel, 2)                         # heterozygous for every selected individual
    c.tbed = tb
    plan = Plan(ctx, c.prob)
    res = plan.run_multi(sigmas(c.prob))
    beta, ok = joint(c.prob, res)
    assert all(r[2][2] == BLOCK_MONOMORPHIC for r in res)
    m2 = int(c.sizes[2])
    P = panel_of(c, tag="dropped-rules")
    assert P.cnt[20] == 0 and P.const[1500] and P.cnt[1500] == P.n_test and P.cnt[10] == P.n_test - 3
    w = np.ones(beta.shape[1])
    w[30], w[31] = np.nan, np.inf
    for mode in ("counts", "std"):
        got, dr = do_score(plan, c, mode=mode)
        check(got, dr, P, beta, ok, mode, what="dropped rules")
        assert dr.tolist() == [m2 + 1 + (mode == "std")] * 3
        # the oracle without that block at all
        keep = snp_block(c.prob) != 2
        sub = Panel.__new__(Panel)
        sub.n_test, sub.code, sub.mu, sub.cnt, sub.sd, sub.const = (P.n_test, P.code[keep], P.mu[keep], P.cnt[keep],
                                                                    P.sd[keep], P.const[keep])
        ref, _, bound = score_oracle(sub, np.nan_to_num(beta[:, keep]), np.ones_like(ok[:, keep]), mode,
                                     m_plan=beta.shape[1])
        assert np.all(np.abs(got - ref) <= bound)
        got, dr = do_score(plan, c, mode=mode, w_s=w[:c.prob.n_s], w_l=w[c.prob.n_s:])
        check(got, dr, P, beta, ok, mode, w=w, what="dropped rules, NaN / inf weights")
        assert dr.tolist() == [m2 + 3 + (mode == "std")] * 3
    plan.close()


@pytest.mark.gpu
def test_weights_and_flips(ctx):
    """Random weights and about 30 % flips in both modes, small and large SNPs; all-flipped COUNTS
    with unit weights on a panel without missing calls equals 2 sum(beta) - unflipped."""
    from dbslmm_amd import Plan
    c = case(150, "ind")
    plan = Plan(ctx, c.prob)
    beta, ok = joint(c.prob, plan.run_multi(sigmas(c.prob)))
    P = panel_of(c)
    assert np.all(P.cnt == P.n_test)
    rng = np.random.default_rng(17)
    M, ns = beta.shape[1], c.prob.n_s
    w = rng.uniform(0.5, 2.0, M)
    flip = (rng.random(M) < 0.3).astype(np.uint8)
    flip[ns:ns + 2] = (1, 0)
    for mode in ("counts", "std"):
        got, dr = do_score(plan, c, mode=mode, w_s=w[:ns], w_l=w[ns:], flip_s=flip[:ns], flip_l=flip[ns:],
                           chunk_slots=96)
        check(got, dr, P, beta, ok, mode, w=w, flip=flip, what="weights + flips")
        assert dr.tolist() == [0, 0, 0]
    plain, _ = do_score(plan, c)
    allf, dr = do_score(plan, c, flip_s=np.ones(ns, np.uint8), flip_l=np.ones(M - ns, np.uint8))
    _, bound = check(allf, dr, P, beta, ok, "counts", flip=np.ones(M), what="all flipped")
    _, bound0 = check(plain, dr, P, beta, ok, "counts", what="unflipped")
    want = 2 * beta.astype(LD).sum(axis=1)[:, None] - plain.astype(LD)
    assert np.all(np.abs(allf - want) <= bound + bound0)
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["run", "multi1", "multi4", "multi5", "factor", "lmm"])
def test_copies_and_routes(ctx, route):
    """One copy after run(); 1, 4 and 5 copies after run_multi (5 leaves the PCG route and takes two
    kernel passes); the factorisation route; LMM-only (no large SNPs).  Another n_copies is refused."""
    from dbslmm_amd import DbslmmError, Plan
    c = case(150, "ind", lmm=route == "lmm", **({"solver": 1} if route == "factor" else {}))
    plan = Plan(ctx, c.prob)
    if route == "run":
        plan.run()
        res = [plan.download()]
    else:
        f = {"multi1": (1.0,), "multi4": (0.7, 0.9, 1.0, 1.2), "multi5": (0.7, 0.8, 1.0, 1.2, 1.4)}.get(route, H2F)
        res = plan.run_multi(sigmas(c.prob, f))
    assert plan.workload()["pcg_route"] == (0 if route in ("multi5", "factor") else 1)
    beta, ok = joint(c.prob, res)
    P = panel_of(c)
    for mode in ("counts", "std"):
        got, dr = do_score(plan, c, mode=mode, chunk_slots=96 if route == "multi5" else 0)
        assert got.shape == (len(res), P.n_test)
        check(got, dr, P, beta, ok, mode, what=route)
    with pytest.raises(DbslmmError, match="n_copies"):
        do_score(plan, c, n_copies=len(res) + 1)
    plan.close()


@pytest.mark.gpu
def test_state_rules(ctx):
    """Before a run: refused.  After variance() had to re-solve (PCG run): refused, naming the cause;
    the next run_multi scores bit for bit as a fresh plan.  score() moves neither variance() nor
    download()."""
    from dbslmm_amd import DbslmmError, Plan
    c = case(150, "ind")
    sig = sigmas(c.prob)
    plan = Plan(ctx, c.prob)
    with pytest.raises(DbslmmError, match="before plan_run"):
        do_score(plan, c)
    res = plan.run_multi(sig)
    fresh, fdr = do_score(plan, c, mode="std")
    dl = plan.download()
    for a, b in zip(dl, res[2]):
        np.testing.assert_array_equal(a, b)             # download() after score(): still the last copy
    v1 = plan.variance(c.tbed, c.ind, c.ts_pos, c.tl_pos)
    with pytest.raises(DbslmmError, match="variance"):
        do_score(plan, c)
    plan.run_multi(sig)
    again, adr = do_score(plan, c, mode="std")
    np.testing.assert_array_equal(again, fresh)
    np.testing.assert_array_equal(adr, fdr)
    other = Plan(ctx, c.prob)
    other.run_multi(sig)
    v0 = other.variance(c.tbed, c.ind, c.ts_pos, c.tl_pos)   # variance() alone
    np.testing.assert_array_equal(v1, v0)
    plan.close()
    other.close()


@pytest.mark.gpu
def test_three_shards_and_units_plans_agree_with_one_device(ctx):
    """Context([0, 0, 0]) within the bar of one device and bit-identical on repeat; the three units
    plans of shard_units_problem add up to the same within the bar."""
    from dbslmm_amd import Context, Plan
    from dbslmm_amd.dist import shard_units_problem
    c = case(150, "ind")
    sig = sigmas(c.prob)
    one = Plan(ctx, c.prob)
    beta, ok = joint(c.prob, one.run_multi(sig))
    P = panel_of(c)
    rng = np.random.default_rng(23)
    M, ns = beta.shape[1], c.prob.n_s
    w = rng.uniform(0.5, 2.0, M)
    flip = (rng.random(M) < 0.3).astype(np.uint8)
    kw = dict(w_s=w[:ns], w_l=w[ns:], flip_s=flip[:ns], flip_l=flip[ns:])
    mctx = Context([0, 0, 0])
    many = Plan(mctx, c.prob)
    mb, mok = joint(c.prob, many.run_multi(sig))
    np.testing.assert_array_equal(mb, beta)
    ud, _ = shard_units_problem(c.prob, sig, 3)
    for mode in ("counts", "std"):
        ref1, dr1 = do_score(one, c, mode=mode, **kw)
        got, dr = do_score(many, c, mode=mode, **kw)
        check(got, dr, P, beta, ok, mode, w=w, flip=flip, what="three shards")
        np.testing.assert_array_equal(dr, dr1)
        again, _ = do_score(many, c, mode=mode, **kw)
        np.testing.assert_array_equal(got, again)
        tot, tdr = np.zeros_like(got), np.zeros_like(dr)
        for d in range(3):
            u = Plan.units(ctx, c.prob, ud, d)
            u.run_multi(sig)
            s, k = do_score(u, c, mode=mode, **kw)
            tot += s
            tdr += k
            u.close()
        check(tot, tdr, P, beta, ok, mode, w=w, flip=flip, what="units plans")
    one.close()
    many.close()
    mctx.close()


@pytest.mark.gpu
def test_copy_split_units_map_copies():
    """shard_copies = 3 on three devices: the dominant block's copies are solved on distinct
    devices (tests/test_multi.py); every shard's local copy lands in the caller's copy."""
    from test_dist import _split_problem
    from dbslmm_amd import Context, Plan, synth
    prob, m = _split_problem()
    _quiet(prob)
    prob.z_l[:] = 6.0 * np.sign(prob.z_l)
    n_total = 50
    t = synth.simulate(int(m.sum()) + 50, n_total, pop="EUR", chroms=[22], seed=106, miss_rate=0.0, large_every=0)
    sig = sigmas(prob)
    prob.opts["shard_copies"] = 3
    mctx = Context([0, 0, 0])
    many = Plan(mctx, prob)
    res = many.run_multi(sig)
    beta, ok = joint(prob, res)
    ind = (np.arange(n_total) % 7 != 3).astype(np.int32)
    rows = np.concatenate([prob.s_pos, prob.l_pos])
    P = Panel(t.bed, n_total, ind, rows)
    for mode in ("counts", "std"):
        got, dr = many.score(t.bed, ind, prob.s_pos, prob.l_pos, mode=mode)
        ref, bound = check(got, dr, P, beta, ok, mode, what="copy-split units")
        assert np.abs(ref[0] - ref[2]).max() > 1e3 * bound.max()      # (a swapped copy would not pass)
    many.close()
    mctx.close()


# ----------------------------------------------------------------------------- GPU: the CLI
@pytest.mark.gpu
@pytest.mark.parametrize("h2f", [False, True])
def test_cli_score_files(tmp_path, h2f):
    """dbslmm --score on test_dat with -dat_str test_chr1 and an indicator: every score column equals
    the oracle evaluated from the CLI's own effect file (column 4: the non-scaled effect) with the
    orientation read from the test .bim; variance.txt and the effect files are what a run without
    the flag writes; with -h2f, hval / hbest equal tune_r2 on phenotypes written into the .fam."""
    import shutil
    from dbslmm_amd import tune_r2
    from _common import BLOCKS_EUR1
    from test_cli import REF, SUMM, split_summary
    from test_variance import td_variance_problem
    v = td_variance_problem(False, drop_test_mono=True)
    summ = str(tmp_path / "summ.txt")
    with open(SUMM) as f, open(summ, "w") as o:
        for line in f:
            if line.split("\t")[1] not in v["dropped"]:
                o.write(line)
    s, l = split_summary(tmp_path, summ)
    ind = v["ind"]
    indf = str(tmp_path / "ind.txt")
    open(indf, "w").write("".join(f"{x}\n" for x in ind))
    # the test panel with synthetic phenotypes in column 6 of its .fam (some absent: -9 / NA)
    dat = str(tmp_path / "panel")
    for ext in (".bed", ".bim"):
        shutil.copy(os.path.join(TD, "test_chr1" + ext), dat + ext)
    fam = [ln.split() for ln in open(os.path.join(TD, "test_chr1.fam")) if ln.strip()]
    n_total = len(fam)
    assert n_total == ind.size
    rng = np.random.default_rng(29)
    y = rng.standard_normal(n_total)
    ytxt = [repr(float(x)) for x in y]
    for i, t in ((4, "-9"), (11, "NA"), (30, "-9")):
        ytxt[i], y[i] = t, np.nan
    with open(dat + ".fam", "w") as o:
        for t, yy in zip(fam, ytxt):
            o.write(" ".join(t[:5] + [yy]) + "\n")
    base = [CLI, "-s", s, "-l", l, "-r", REF, "-b", BLOCKS_EUR1, "-n", "2400", "-nsnp", "996", "-h", "0.5",
            "-mafMax", "0.2", "--precise-out", "-dat_str", dat, "-test_indicator_file", indf]
    if h2f:
        base += ["-h2f", "0.8,1,1.2"]
    outs = {}
    for name, extra in (("plain", []), ("scored", ["--score", str(tmp_path / "scored" / "sc")])):
        d = tmp_path / name
        d.mkdir()
        r = subprocess.run(base + ["-eff", str(d / "o.dbslmm")] + extra, capture_output=True, text=True, cwd=str(d),
                           timeout=300)
        assert r.returncode == 0, r.stderr
        effs = [f"o_h2f{t}.dbslmm.txt" for t in ("0.8", "1", "1.2")] if h2f else ["o.dbslmm.txt"]
        outs[name] = [open(d / f).read() for f in ["variance.txt"] + effs]
        stdout = r.stdout
    assert outs["plain"] == outs["scored"]              # the flag moves neither variance.txt nor the effects
    lines = open(tmp_path / "scored" / "sc.score.txt").read().splitlines()
    cols = [f"SCORE_h2f{t}" for t in ("0.8", "1", "1.2")] if h2f else ["SCORE"]
    assert lines[0].split() == ["FID", "IID"] + cols
    sel = np.flatnonzero(ind)
    assert [ln.split()[:2] for ln in lines[1:]] == [fam[i][:2] for i in sel]
    got = np.array([[float(x) for x in ln.split()[2:]] for ln in lines[1:]]).T
    # the oracle from the effect files and the test .bim
    tbim = [ln.rstrip("\n").split("\t") for ln in open(dat + ".bim")]
    row_of = {e["snp"]: int(r) for e, r in zip(v["info_s"], v["ts_pos"])}
    row_of.update({e["snp"]: int(r) for e, r in zip(v["info_l"], v["tl_pos"])})
    tbed = load_bed(dat + ".bed")
    m_plan = len(v["info_s"]) + len(v["info_l"])
    for c, eff in enumerate(outs["scored"][1:]):
        rows, beta, w, flip = [], [], [], []
        for ln in eff.splitlines():
            snp, a1, _, noscl, _ = ln.split()
            r = row_of[snp]
            rows.append(r)
            beta.append(float(noscl))
            flip.append(a1 == tbim[r][5])
            w.append(1.0 if a1 in (tbim[r][4], tbim[r][5]) else 0.0)
        assert len(rows) == m_plan
        P = Panel(tbed, n_total, ind, np.array(rows))
        ref, _, bound = score_oracle(P, np.array(beta)[None], np.ones((1, len(rows)), bool), "counts", np.array(w),
                                     np.array(flip), m_plan=m_plan)
        err = np.abs(got[c].astype(LD) - ref[0])
        print(f"cli score column {c}: worst |got - ref| / bound = {float(np.max(err / bound[0])):.3g}")
        assert np.all(err <= bound[0]), c
    if h2f:
        r2, best = tune_r2(got, y[sel])
        hv = [ln.split() for ln in open(tmp_path / "scored" / "sc.hval.r2").read().splitlines()]
        assert [t[0] for t in hv] == ["0.8", "1", "1.2"]
        assert np.all(np.abs(np.array([float(t[1]) for t in hv]) - r2) <= 1e-12)
        assert open(tmp_path / "scored" / "sc.hbest.r2").read().split() == [("0.8", "1", "1.2")[best]]
        assert "R2 =" in stdout
    else:
        assert not os.path.exists(tmp_path / "scored" / "sc.hval.r2")
