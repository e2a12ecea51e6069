"""Oracle of the LD score entry points (dbslmm_ld_scores, dbslmm_ldsc_fit), built on
tests/_clump_ref.py: r2 in longdouble from the exact integers, the window decided on integers, the
terms summed in longdouble; and the regression rule of dbslmm_amd/csrc/ldsc_fit.hpp in NumPy."""
from __future__ import annotations

import numpy as np

import _clump_ref as CR

LD = np.longdouble
TILE = 128


def position_order(chrom, bp) -> np.ndarray:
    """position p -> caller index: sorted by (chr, bp, caller index), as ldsc_layout.hpp sorts"""
    chrom = np.asarray(chrom, dtype=np.int64)
    bp = np.asarray(bp, dtype=np.int64)
    return np.array(sorted(range(len(bp)), key=lambda k: (chrom[k], bp[k], k)), dtype=np.int64)


def window_matrix(chrom, bp, window_bp: int) -> np.ndarray:
    """[k, j] True where j lies inside the window of k: same chromosome, |bp_j - bp_k| <= window_bp"""
    chrom = np.asarray(chrom, dtype=np.int64)
    bp = np.asarray(bp, dtype=np.int64)
    return (chrom[:, None] == chrom[None, :]) & (np.abs(bp[:, None] - bp[None, :]) <= int(window_bp))


def ld_scores_ref(X: np.ndarray, chrom, bp, window_bp: int, unbiased: bool, n_ref: int, r2=None) -> dict:
    """The LD scores of the rows X (dosages, -1 = missing; one row per listed row, in the caller's
    order) as include/dbslmm_hip.h defines them.  Returns l2 (longdouble, NaN for a row whose own r2
    is NaN), n_window (exact), and the pieces a bar needs: r2 and t (longdouble matrices), used
    ([k, j]: the term t_kj is part of l2_k), sum_abs = sum over the used terms of |t|, n_terms.
    r2: CR.r2_longdouble(X) when the caller already has it."""
    n = len(X)
    assert X.shape[1] == n_ref
    W = window_matrix(chrom, bp, window_bp)
    n_window = W.sum(axis=1).astype(np.int32)
    if r2 is None:
        r2 = CR.r2_longdouble(X) if n else np.zeros((0, 0), dtype=LD)
    nan_row = np.isnan(np.diagonal(r2))
    t = r2 - (LD(1) - r2) / LD(n_ref - 2) if unbiased else r2.copy()
    used = W & ~nan_row[:, None] & ~nan_row[None, :]
    assert not np.isnan(t[used]).any()
    tz = np.where(used, t, LD(0))
    l2 = tz.sum(axis=1, dtype=LD)
    l2[nan_row] = np.nan
    return dict(l2=l2, n_window=n_window, r2=r2, t=t, used=used, sum_abs=np.abs(tz).sum(axis=1, dtype=LD),
                n_terms=used.sum(axis=1), nan_row=nan_row)


def four_product_pairs128(nmiss, chrom, bp) -> np.ndarray:
    """[k, j] (caller order) True where the library computes the pair in a four-product tile: a row
    with a missing call among the rows of the 128-position tile row of k or of j"""
    order = position_order(chrom, bp)
    n = len(order)
    rank = np.empty(n, dtype=np.int64)
    rank[order] = np.arange(n)
    blk = rank // TILE
    nm = np.asarray(nmiss)
    bm = np.zeros(int(blk.max()) + 1 if n else 0, dtype=bool)
    np.logical_or.at(bm, blk, nm > 0)
    return bm[blk][:, None] | bm[blk][None, :]


# ------------------------------------------------------------------------------------ regression
def _weights(l, N, M, h2, a):
    h2 = min(max(h2, 0.0), 1.0)
    lj = np.maximum(l, 1.0)
    c = a + h2 * N / M * lj
    return 1.0 / (2.0 * (c * c)) / lj


def _solve(A, b):
    """(coef, ok): the singularity rule of ldsc_fit.hpp"""
    if A.shape == (1, 1):
        if not (A[0, 0] > 0 and np.isfinite(A[0, 0]) and np.isfinite(b[0])):
            return None, False
        return b / A[0, 0], True
    det = A[0, 0] * A[1, 1] - A[0, 1] * A[0, 1]
    if not (np.isfinite(det) and np.all(np.isfinite(b)) and abs(det) > 1e-12 * A[0, 0] * A[1, 1]):
        return None, False
    return np.linalg.solve(A, b), True


def ldsc_fit_ref(chi2, N, l, M, intercept=None, n_blocks=200, chisq_max=0.0) -> dict:
    """The rule of ldsc_fit.hpp.  status 0 ok, 1 too few SNPs, 2 singular."""
    chi2, N, l = (np.asarray(v, dtype=np.float64) for v in (chi2, np.broadcast_to(N, np.shape(chi2)), l))
    if chisq_max > 0:
        keep = ~(chi2 > chisq_max)
        chi2, N, l = chi2[keep], N[keep], l[keep]
    n = len(chi2)
    free = intercept is None
    P = 2 if free else 1
    out = dict(h2=np.nan, h2_se=np.nan, intercept=np.nan, intercept_se=np.nan, n=n, status=0,
               mean_chi2=float(chi2.mean()) if n else np.nan)
    if n < 2 * P:
        out["status"] = 1
        return out
    Nbar = N.mean()
    x = N * l / Nbar
    a0 = 1.0 if free else float(intercept)
    X = np.stack([x, np.ones_like(x)], 1) if free else x[:, None]
    y = chi2 if free else chi2 - a0
    h2 = M * (chi2.mean() - a0) / (l * N).mean()
    a = a0

    def scaled(w):
        s = np.sqrt(w)
        s = s / s.sum()
        return X * s[:, None], y * s

    w = _weights(l, N, M, h2, a)
    for _ in range(2):
        Xw, yw = scaled(w)
        c, ok = _solve(Xw.T @ Xw, Xw.T @ yw)
        if not ok:
            out["status"] = 2
            return out
        h2 = c[0] * M / Nbar
        a = c[1] if free else a0
        w = _weights(l, N, M, h2, a)
    Xw, yw = scaled(w)
    B = min(n_blocks, n)
    sep = [(b * n) // B for b in range(B + 1)]
    XtX = np.array([Xw[s:e].T @ Xw[s:e] for s, e in zip(sep[:-1], sep[1:])])
    Xty = np.array([Xw[s:e].T @ yw[s:e] for s, e in zip(sep[:-1], sep[1:])])
    tX, ty = XtX.sum(0), Xty.sum(0)
    est, ok = _solve(tX, ty)
    if not ok:
        out["status"] = 2
        return out
    dele = []
    for b in range(B):
        d, ok = _solve(tX - XtX[b], ty - Xty[b])
        if not ok:
            out["status"] = 2
            return out
        dele.append(d)
    pseudo = B * est - (B - 1) * np.array(dele)
    se = np.sqrt(np.var(pseudo, axis=0, ddof=1) / B)
    out.update(h2=est[0] * M / Nbar, h2_se=se[0] * M / Nbar)
    if free:
        out.update(intercept=est[1], intercept_se=se[1])
    else:
        out.update(intercept=a0, intercept_se=0.0)
    return out


def simulate(rng, M=100_000, h2=0.4, a=1.05):
    """The simulation of the recovery test: independent chi2 with E = a + N h2 l / M"""
    N = rng.integers(40000, 50000, M).astype(float)
    l = rng.gamma(2.0, 20.0, M) + 1
    chi2 = (a + N * h2 * l / M) * rng.chisquare(1, M)
    return chi2, N, l


# ------------------------------------------------------------------------------- test_dat inputs
def test_dat_inputs(summ_path: str, ref_prefix: str) -> dict:
    """The CLI's --ldsc inputs restated: per .bim row snp, chrom (int code by first appearance), bp and
    summ_of (the first summary line that names the row and has n_obs > 0, else -1); per summary line
    with at least 11 fields z = beta / se (0 when se is not a positive number) and n_obs (column 5)."""
    snp, chrom, bp, code, row_of = [], [], [], {}, {}
    for r, line in enumerate(open(ref_prefix + ".bim")):
        f = line.rstrip("\n").split("\t")
        snp.append(f[1])
        chrom.append(code.setdefault(f[0], len(code)))
        bp.append(int(f[3]))
        row_of.setdefault(f[1], r)
    z, n_obs, name = [], [], []
    for line in open(summ_path):
        f = line.rstrip("\n").split("\t")
        if len(f) < 11:
            continue
        z.append(float(f[8]) / float(f[9]) if f[9][:1].isdigit() and float(f[9]) > 1e-20 else 0.0)
        n_obs.append(float(f[4]))
        name.append(f[1])
    summ_of = np.full(len(snp), -1, dtype=np.int64)
    for s, nm in enumerate(name):
        r = row_of.get(nm, -1)
        if r >= 0 and n_obs[s] > 0 and summ_of[r] < 0:
            summ_of[r] = s
    return dict(snp=snp, chrom=np.array(chrom, dtype=np.int32), bp=np.array(bp, dtype=np.int64), summ_of=summ_of,
                z=np.array(z), n_obs=np.array(n_obs), n_summ=len(name))
