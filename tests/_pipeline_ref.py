"""The panel and the oracle of tests/test_pipeline.py: a three-chromosome reference panel with its
GEMMA summary, built on the CPU, and what `dbslmm --summary / --pth` and `dbslmm --ldsc` must make
of it, composed from the oracles the repository already has: the candidate list and the greedy
clump on exact integers (tests/_clump_ref.py), the host steps and the direct solve of the reference
(oracle/ref_numpy.py), the LD scores in longdouble with their bars (tests/_ldsc_ref.py,
tests/test_ldsc.py) and the regression rule in NumPy.

The panel (build_panel): synth.simulate(2400, 701, chromosomes 19, 20, 21) -- 701 individuals leave
pad bits in the last byte of a row and give kpad 768 -- with 1 % missing calls in the rows of
chromosome 20 and in 100 consecutive rows of chromosome 21 (elsewhere none: raw and four-product
tiles both occur, in the clump and in the LD scores), one monomorphic and one all-missing row, a
handful of duplicate .bim ids, and the block file without one block in the middle of chromosome 20.

The summary: z_j = 9 sum_c r(j, c) + N(0, 1) over the causal rows c within 60 rows of j, r the
float64 correlation of the mean-imputed dosages; se = 1 / sqrt(N_j), N_j in [90000, 100000) per line.
36 causal rows, 10 pairs of them 5 to 9 rows apart inside one block (the rows between two causal
rows are linked to their neighbours but not to both ends: chains), one inside the removed block.
Then lines are perturbed: swapped alleles, a wrong a2, ids absent from the .bim (one of each forced
onto a causal row), two neighbouring lines with the same beta / se text (a priority tie), one
duplicated line with another z and N, one line with N = 0."""
from __future__ import annotations

import functools
import math
import os

import numpy as np

import _clump_ref as CR
import _ldsc_ref as LR
import ref_numpy as R

LD = np.longdouble
N_REF = 701
N_OBS = 100_000
PTH = 1e-6
LD_WIND_KB = 200
SEED = 21


class Panel:
    """paths (ref, summ, blocks), n_rows, n_lines, bed (uint8 image), X (dosages, -1 missing), chrom
    (as in the .bim), bp, snp (.bim ids), own (the ids before the duplicates), causal, mono, allmiss,
    swapped_causal / absent_causal (the ids of the causal rows whose line has swapped alleles / an id
    the .bim lacks), tie (the two tied summary lines), dup (the two lines of the duplicated SNP),
    zero_n (the line with N = 0), removed (chr, start, end of the block the block file lacks)"""


def build_panel(out: str, seed: int = SEED) -> Panel:
    from dbslmm_amd import synth
    os.makedirs(out, exist_ok=True)
    sp = synth.simulate(2400, N_REF, pop="EUR", chroms=[19, 20, 21], seed=seed, miss_rate=0.0, large_every=0)
    m = sp.m
    rng = np.random.default_rng(seed)
    chrom, ps, blk = np.asarray(sp.chrom), np.asarray(sp.ps), np.asarray(sp.block)
    X = CR.decode(sp.bed, N_REF, np.arange(m)).copy()
    c19, c21 = np.flatnonzero(chrom == 19), np.flatnonzero(chrom == 21)
    holes = chrom == 20
    holes[c21[150:250]] = True
    X[(rng.random(X.shape) < 0.01) & holes[:, None]] = -1
    mono, allmiss = int(c19[300]), int(c21[40])
    X[mono] = 2
    X[allmiss] = -1
    bed = CR.encode(X)

    P = Panel()
    P.ref, P.summ, P.blocks = (os.path.join(out, f) for f in ("ref", "summary.assoc.txt", "blocks.bed"))
    bed.tofile(P.ref + ".bed")
    with open(P.ref + ".fam", "w") as f:
        for i in range(N_REF):
            f.write(f"id{i} id{i} 0 0 0 -9\n")
    own = [f"rs{c}_{p}" for c, p in zip(chrom, ps)]
    snp = list(own)
    for k in rng.choice(np.arange(100, m), size=6, replace=False):   # duplicate ids: the first .bim line keeps the id
        if k not in (mono, allmiss) and k - 37 not in (mono, allmiss):
            snp[k] = own[k - 37]
    with open(P.ref + ".bim", "w") as f:
        for c, s, p in zip(chrom, snp, ps):
            f.write(f"{c}\t{s}\t0\t{p}\tA\tG\n")
    blocks = [list(b) for b in sp.blocks]
    c20 = [i for i, b in enumerate(blocks) if b[0] == 20]
    gone = c20[len(c20) // 2]
    P.removed = tuple(blocks[gone])
    with open(P.blocks, "w") as f:
        for i, (c, s, e) in enumerate(blocks):
            if i != gone:
                f.write(f"chr{c}\t{s}\t{e}\n")

    # causal rows: pairs inside one block, one in the removed block, singles; none near the two NaN rows
    sizes = np.bincount(blk, minlength=len(blocks))
    near_nan = lambda j: min(abs(j - mono), abs(j - allmiss)) <= 3          # noqa: E731
    causal = []
    roomy = [b for b in np.flatnonzero(sizes >= 16) if b not in (gone, blk[mono], blk[allmiss])]
    for b in rng.choice(roomy, size=10, replace=False):
        idx = np.flatnonzero(blk == b)
        a = int(idx[int(rng.integers(1, 4))])
        causal += [a, a + int(rng.integers(5, 10))]
        assert blk[causal[-1]] == b
    in_gone = np.flatnonzero(blk == gone)
    causal.append(int(in_gone[len(in_gone) // 2]))
    while len(causal) < 36:
        j = int(rng.integers(5, m - 5))
        if not near_nan(j) and min(abs(j - c) for c in causal) > 20:
            causal.append(j)
    singles = causal[21:]                                              # neither of a pair nor in the removed block
    P.causal = np.array(sorted(causal))

    # z = 9 sum_c r(j, c) + N(0, 1), r of the mean-imputed rows (0 for a row without variance)
    obs = X >= 0
    g = np.where(obs, X, 0).astype(np.float64)
    xc = np.where(obs, g - g.sum(axis=1, keepdims=True) / np.maximum(obs.sum(axis=1, keepdims=True), 1), 0.0)
    sd = np.sqrt((xc * xc).sum(axis=1))
    xn = xc / np.where(sd > 0, sd, np.inf)[:, None]
    r = xn @ xn[P.causal].T                                           # m x causal; 0 for a NaN row
    near = np.abs(np.arange(m)[:, None] - P.causal[None, :]) <= 60
    z = 9.0 * np.where(near, r, 0.0).sum(axis=1) + rng.standard_normal(m)
    nobs = rng.integers(90000, 100000, size=m)

    def line(j, zj, nj):
        se = 1.0 / math.sqrt(nj)
        pv = math.erfc(abs(zj) / math.sqrt(2.0))
        return [str(chrom[j]), own[j], str(ps[j]), "0", str(nj), "A", "G", f"{sp.af[j]:.6f}",
                f"{zj * se:.6e}", f"{se:.6e}", f"{pv:.6e}"]

    lines = [line(j, z[j], int(nobs[j])) for j in range(m)]            # one per .bim row, in .bim order
    for j in range(m):
        u = rng.random()
        if j in (mono, allmiss):
            lines[j][6] = "T"          # the solve never sees the two NaN rows; --ldsc (no allele check) does
        elif u < 0.03:
            lines[j][5], lines[j][6] = lines[j][6], lines[j][5]
        elif u < 0.04:
            lines[j][6] = "T"
        elif u < 0.05:
            lines[j][1] += "_absent"
    lines[singles[0]][5], lines[singles[0]][6] = "G", "A"              # a causal row with swapped alleles
    lines[singles[1]][1] = own[singles[1]] + "_absent"                 # a causal row the .bim does not hold
    # a priority tie: the line before a causal row takes the causal row's beta / se text (and N)
    t = singles[2]
    for col in (4, 8, 9, 10):
        lines[t - 1][col] = lines[t][col]
    lines[t - 1][1], lines[t - 1][5], lines[t - 1][6] = own[t - 1], "A", "G"
    lines[t][1], lines[t][5], lines[t][6] = own[t], "A", "G"
    # N = 0 on one ordinary line
    quiet = [j for j in range(200, m) if min(abs(j - c) for c in causal) > 25 and not near_nan(j)]
    zero = quiet[0]
    lines[zero][4] = "0"
    # one duplicated SNP: the second line has another z and N (the first one counts in --ldsc)
    d = quiet[50]
    lines[d][1], lines[d][5], lines[d][6] = own[d], "A", "G"
    out_lines, at = [], {}
    for j, l in enumerate(lines):
        at[j] = len(out_lines)
        out_lines.append(l)
        if j == d:
            out_lines.append(line(d, -1.5 * z[d] + 3.0, 90000 + (int(nobs[d]) - 85000) % 10000))
    with open(P.summ, "w") as f:
        for l in out_lines:
            f.write("\t".join(l) + "\n")
    P.n_rows, P.n_lines = m, len(out_lines)
    P.bed, P.X, P.chrom, P.bp, P.snp, P.own = bed, X, chrom, ps.astype(np.int64), snp, own
    P.mono, P.allmiss = mono, allmiss
    P.swapped_causal, P.absent_causal = own[singles[0]], own[singles[1]] + "_absent"
    P.tie = (at[t - 1], at[t])
    P.zero_n, P.dup = at[zero], (at[d], at[d] + 1)
    X.setflags(write=False)
    return P


# ------------------------------------------------------------------------------------ --summary
def in_window(chrom, bp, window_bp):
    return LR.window_matrix(chrom, bp, window_bp) & ~np.eye(len(bp), dtype=bool)


def clump_tiles_four_product(nmiss, chrom, bp):
    """[i, j] True where dbslmm_clump computes the candidate pair in a four-product tile: a row with a
    missing call among the candidates of the 32-position tile row of i or of j (position order)"""
    order = LR.position_order(chrom, bp)
    rank = np.empty(len(order), dtype=np.int64)
    rank[order] = np.arange(len(order))
    t = rank // 32
    bm = np.zeros(int(t.max()) + 1, dtype=bool)
    np.logical_or.at(bm, t, np.asarray(nmiss) > 0)
    return bm[t][:, None] | bm[t][None, :]


class SummaryOracle:
    """dbslmm --summary P.summ --pth pth --clump-r2 r2 --clump-kb kb: cand (CR.summary_candidates),
    index_of, margin, link (candidate pairs in the window with r2 >= the threshold, exactly), index
    (candidates that are index SNPs, in priority order), index_lines (their summary lines)"""

    def __init__(self, P: Panel, pth=PTH, r2=0.2, kb=1000.0):
        self.P, self.r2, self.kb = P, r2, kb
        self.cand = c = CR.summary_candidates(P.summ, P.ref + ".bim", pth)
        n = len(c["snp"])
        self.Xc = CR.decode(P.bed, N_REF, c["row"]) if n else np.zeros((0, N_REF), dtype=np.int8)
        w = int(round(kb * 1000))
        if n:
            Nm, den = CR.pair_integers(self.Xc)
            self.index_of, self.margin = CR.clump_ref(self.Xc, c["chrom"], c["bp"], r2, w, pairs_int=(Nm, den))
            self.window = in_window(c["chrom"], c["bp"], w)
            self.link = CR.ge_threshold(Nm, den, r2) & self.window
        else:
            self.index_of, self.margin = np.zeros(0, dtype=np.int32), np.inf
            self.window = self.link = np.zeros((0, 0), dtype=bool)
        self.index = [k for k in range(n) if self.index_of[k] == k]
        self.index_lines = [int(c["line"][k]) for k in self.index]
        self.n_absorbed = [int((self.index_of == k).sum()) - 1 for k in self.index]

    def split(self, tmp: str):
        """the -s / -l files of the split by the oracle's index SNPs, by summary line"""
        s_path, l_path = os.path.join(tmp, "s.txt"), os.path.join(tmp, "l.txt")
        L = set(self.index_lines)
        with open(self.P.summ) as f, open(s_path, "w") as fs, open(l_path, "w") as fl:
            for i, line in enumerate(f):
                (fl if i in L else fs).write(line)
        return s_path, l_path

    @functools.lru_cache(maxsize=None)
    def host(self, maf_max: float):
        """the host steps after the split: (blocks, inter_s, inter_l, info_s, info_l, badsnps lines)"""
        P = self.P
        bim = _bim(P, abs(maf_max - 1.0) >= 1e-10)
        blocks = R.read_block(P.blocks)
        summ = R.read_summ(P.summ)
        L = set(self.index_lines)
        summ_s = [s for i, s in enumerate(summ) if i not in L]
        summ_l = [s for i, s in enumerate(summ) if i in L]
        inter_s, good_s = R.match_ref(summ_s, bim, maf_max)
        inter_l, good_l = R.match_ref(summ_l, bim, maf_max)
        bad = [f"{x.snp} 0" for x, g in zip(summ_s, good_s) if not g] + [f"{x.snp} 1" for x, g in zip(summ_l, good_l) if not g]
        return blocks, inter_s, inter_l, R.add_block(inter_s, blocks), R.add_block(inter_l, blocks), bad

    def est(self, h: float, maf_max: float = 0.2):
        """the reference's estimate at heritability h: R.est by one Cholesky per block"""
        blocks, _, _, info_s, info_l, _ = self.host(maf_max)
        return R.est(self.P.bed, N_REF, N_OBS, h / self.P.n_lines, len(blocks), info_s, info_l, tau=0.8, method="chol")


@functools.lru_cache(maxsize=None)
def _bim(P: Panel, constr: bool):
    with np.errstate(invalid="ignore"):                # the all-missing row: 0 / 0, a NaN MAF as in the reference
        return R.read_bim(P.ref, N_REF, constr)


# --------------------------------------------------------------------------------------- --ldsc
class LdscOracle:
    """dbslmm --ldsc --summary P.summ -r P.ref --ld-wind-kb 200: l2 (longdouble, NaN rows NaN), bar
    (tests/test_ldsc.py's, the tiles of the whole list), nan_row, M (M_5_50), td (LR.test_dat_inputs),
    reg (.bim rows of the regression: named by a summary line with N > 0, finite score)"""

    def __init__(self, P: Panel, l2_bar):
        import oracle as O
        self.P = P
        self.td = td = LR.test_dat_inputs(P.summ, P.ref)
        n = P.n_rows
        code, bp = td["chrom"], td["bp"]
        nmiss = (P.X < 0).sum(axis=1)
        fp_all_rows = _tile_missing(nmiss, code, bp)
        self.l2, self.bar = np.zeros(n, dtype=LD), np.zeros(n, dtype=LD)
        self.nan_row, self.uses_fp = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
        for c in np.unique(code):                    # the dense longdouble arrays of one chromosome at a time
            idx = np.flatnonzero(code == c)
            ref = LR.ld_scores_ref(P.X[idx], code[idx], bp[idx], LD_WIND_KB * 1000, True, N_REF)
            fp = fp_all_rows[idx][:, None] | fp_all_rows[idx][None, :]
            bar, _ = l2_bar(ref, P.X[idx], code[idx], bp[idx], True, N_REF, fp=fp)
            self.l2[idx], self.bar[idx], self.nan_row[idx] = ref["l2"], bar, ref["nan_row"]
            self.uses_fp[idx] = (fp & ref["used"]).any(axis=1)
        self.maf = O.bed_maf(P.bed, N_REF, n)
        self.M = int((~self.nan_row & (self.maf > 0.05)).sum())
        self.named = td["summ_of"] >= 0                      # --dry-run's count
        self.reg = np.flatnonzero(self.named & ~self.nan_row)

    def fit(self, intercept=None, chisq_max=0.0):
        s = self.td["summ_of"][self.reg]
        return LR.ldsc_fit_ref(self.td["z"][s] ** 2, self.td["n_obs"][s], self.l2[self.reg].astype(np.float64), self.M,
                               intercept=intercept, chisq_max=chisq_max)


def _tile_missing(nmiss, chrom, bp):
    """per row: a missing call among the rows of its 128-position tile row (position order of the whole
    list, as one dbslmm_ld_scores call lays it out)"""
    order = LR.position_order(chrom, bp)
    rank = np.empty(len(order), dtype=np.int64)
    rank[order] = np.arange(len(order))
    t = rank // LR.TILE
    bm = np.zeros(int(t.max()) + 1, dtype=bool)
    np.logical_or.at(bm, t, np.asarray(nmiss) > 0)
    return bm[t]
