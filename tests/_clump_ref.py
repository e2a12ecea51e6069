"""Oracle of the clumping entry points (dbslmm_ld_r2, dbslmm_clump): exact integers, then PLINK's
greedy rule as include/dbslmm_hip.h restates it.

r_ij is the Pearson correlation of the dosages of two rows, missing calls at the row mean.  With o
the observed-call indicator, g the dosage (0 where missing), S, sq, m the observed sum, sum of
squares and count of a row, and the cross sums GG = sum g_i g_j, GO = sum g_i o_j, OG = sum o_i g_j,
OO = sum o_i o_j, the centred cross product and sums of squares are ratios of integers:

    c_ij = (GG m_i m_j - S_j GO m_i - S_i OG m_j + S_i S_j OO) / (m_i m_j) = Nm / (m_i m_j)
    c_ii = (sq_i m_i - S_i^2) / m_i = Dm_i / m_i
    r2   = Nm^2 / (m_i m_j Dm_i Dm_j)                                  (Nm^2 / den below)

(no missing call: m = n, GO = S_i, OG = S_j, OO = n, and Nm = n (n GG - S_i S_j), the N of the raw
path times n).  `Nm` and `den` are Python integers, so r2 >= t is decided exactly against
Fraction(t) -- the double the library receives -- and the values are rounded once to longdouble.
den == 0 (a row without variance or without an observed call) is NaN: it compares false."""
from __future__ import annotations

from fractions import Fraction

import numpy as np


def decode(bed: np.ndarray, n_ref: int, rows) -> np.ndarray:
    """Dosages of the bed rows `rows` over the n_ref individuals as int8, -1 = missing call
    (PLINK codes, low bits first: 00 -> 2, 10 -> 1, 11 -> 0, 01 -> missing)."""
    bps = (n_ref + 3) // 4
    rows = np.asarray(rows, dtype=np.int64)
    raw = np.asarray(bed, dtype=np.uint8)[3:].reshape(-1, bps)[rows]
    codes = np.stack([(raw >> s) & 3 for s in (0, 2, 4, 6)], axis=-1).reshape(len(rows), 4 * bps)[:, :n_ref]
    return np.array([2, -1, 1, 0], dtype=np.int8)[codes]


def encode(X: np.ndarray) -> np.ndarray:
    """The .bed image (magic bytes included) of dosage rows X (int, -1 = missing)."""
    X = np.asarray(X)
    n_rows, n = X.shape
    bps = (n + 3) // 4
    code = np.full((n_rows, 4 * bps), 0, dtype=np.uint8)          # pad bits 00, as PLINK writes them
    code[:, :n] = np.array([1, 3, 2, 0], dtype=np.uint8)[X + 1]    # -1 -> 01, 0 -> 11, 1 -> 10, 2 -> 00
    q = code.reshape(n_rows, bps, 4)
    body = (q[:, :, 0] | (q[:, :, 1] << 2) | (q[:, :, 2] << 4) | (q[:, :, 3] << 6)).astype(np.uint8)
    return np.concatenate([np.array([0x6C, 0x1B, 0x01], dtype=np.uint8), body.ravel()])


def _gram(A: np.ndarray, B: np.ndarray) -> np.ndarray:
    """A B^T of small non-negative integer matrices as exact int64 (float32 operands, exact fp64
    partial sums: every entry stays far below 2^53), in chunks of the long axis."""
    out = np.zeros((A.shape[0], B.shape[0]))
    for k in range(0, A.shape[1], 1 << 16):
        out += A[:, k:k + (1 << 16)].astype(np.float32).astype(np.float64) @ \
               B[:, k:k + (1 << 16)].astype(np.float32).astype(np.float64).T
    return np.rint(out).astype(np.int64)


def sums(X: np.ndarray) -> dict:
    """The exact integers of the rows X: per row S, sq, m (observed count), nmiss; per pair GG, GO,
    OG, OO (int64)."""
    o = (X >= 0).astype(np.int8)
    g = np.where(X >= 0, X, 0).astype(np.int8)
    S = g.sum(axis=1, dtype=np.int64)
    sq = (g * g).sum(axis=1, dtype=np.int64)
    m = o.sum(axis=1, dtype=np.int64)
    if np.all(m == X.shape[1]):                       # no missing call: the cross sums are the row sums
        GG = _gram(g, g)
        n = np.int64(X.shape[1])
        GO = np.repeat(S[:, None], len(S), axis=1)
        return dict(S=S, sq=sq, m=m, nmiss=X.shape[1] - m, GG=GG, GO=GO, OG=GO.T.copy(),
                    OO=np.full((len(S), len(S)), n, dtype=np.int64))
    return dict(S=S, sq=sq, m=m, nmiss=X.shape[1] - m, GG=_gram(g, g), GO=_gram(g, o), OG=_gram(o, g),
                OO=_gram(o, o))


def pair_factors(X: np.ndarray):
    """(Nm, mm, Dm): object arrays of Python integers, r2_ij = Nm_ij^2 / (mm_ij Dm_i Dm_j) exactly,
    mm_ij = m_i m_j."""
    s = sums(X)
    O = lambda a: np.asarray(a).astype(object)     # noqa: E731  (Python integers from here on)
    S, sq, m = O(s["S"]), O(s["sq"]), O(s["m"])
    Dm = sq * m - S * S
    mi, mj, Si, Sj = m[:, None], m[None, :], S[:, None], S[None, :]
    Nm = O(s["GG"]) * mi * mj - Sj * O(s["GO"]) * mi - Si * O(s["OG"]) * mj + Si * Sj * O(s["OO"])
    return Nm, mi * mj, Dm


def pair_integers(X: np.ndarray):
    """(Nm, den): object matrices of Python integers with r2_ij = Nm_ij^2 / den_ij exactly; den = 0
    where r2 is NaN."""
    Nm, mm, Dm = pair_factors(X)
    return Nm, mm * Dm[:, None] * Dm[None, :]


def to_longdouble(a) -> np.ndarray:
    """Object array of Python integers below 2^144 -> longdouble in three exact 48-bit pieces (a
    direct conversion may pass through double), added from the top: within one ulp of longdouble,
    exact below 2^64."""
    a = np.asarray(a, dtype=object)
    sign = np.where(a < 0, -1, 1).astype(np.longdouble)
    mag = np.abs(a)
    assert np.all(mag < (1 << 144))
    mask = (1 << 48) - 1
    piece = lambda sh: ((mag >> sh) & mask).astype(np.float64).astype(np.longdouble)   # noqa: E731
    two48 = np.longdouble(2.0) ** 48
    return sign * ((piece(96) * two48 + piece(48)) * two48 + piece(0))


def r2_longdouble(X: np.ndarray) -> np.ndarray:
    """r2 of every pair of rows of X in longdouble from the exact integers (NaN where the
    denominator is 0): Nm Nm / (mm Dm_i Dm_j), every factor converted within an ulp of longdouble
    (exactly below 2^64) -- some seven roundings of 2^-64, 2^-61 relative in all."""
    Nm, mm, Dm = pair_factors(X)
    with np.errstate(invalid="ignore", divide="ignore"):
        nm, d = to_longdouble(Nm), to_longdouble(Dm)
        out = nm * nm / (to_longdouble(mm) * d[:, None] * d[None, :])
    out[(mm * Dm[:, None] * Dm[None, :]) == 0] = np.nan
    return out


def ge_threshold(Nm, den, t: float) -> np.ndarray:
    """r2 >= t decided exactly (t the double itself); False where den = 0 (NaN compares false)."""
    ft = Fraction(t)
    ok = Nm * Nm * ft.denominator >= den * ft.numerator
    return np.asarray(ok & (den > 0), dtype=bool)


def clump_ref(X: np.ndarray, chrom, bp, t: float = 0.2, window_bp: int = 1_000_000, brute: bool = False,
              pairs_int=None):
    """The greedy rule on candidates X (rows in priority order, most significant first):
    (index_of, margin).  margin = the smallest |r2 - t| / t over the same-chromosome in-window
    candidate pairs with a defined r2.  brute: no window test at all (every same-chromosome pair) --
    the O(n^2) cross-check, equal to the windowed walk whenever the window covers the span.
    pairs_int: pair_integers(X) when the caller already has it (several settings on one list)."""
    chrom = np.asarray(chrom, dtype=np.int64)
    bp = np.asarray(bp, dtype=np.int64)
    n = len(chrom)
    if n == 0:
        return np.zeros(0, dtype=np.int32), np.inf
    Nm, den = pair_integers(X) if pairs_int is None else pairs_int
    link = ge_threshold(Nm, den, t)
    np.fill_diagonal(link, False)
    same = chrom[:, None] == chrom[None, :]
    if brute:
        adj = link & same
        neigh = [np.flatnonzero(adj[k]) for k in range(n)]
        pairs = same
    else:
        # windowed: per candidate, scan outwards in position order until the window or chromosome ends
        order = sorted(range(n), key=lambda k: (chrom[k], bp[k], k))
        rank = {k: p for p, k in enumerate(order)}
        neigh, pairs = [], np.zeros((n, n), dtype=bool)
        for k in range(n):
            mine = []
            for step in (1, -1):
                p = rank[k] + step
                while 0 <= p < n and chrom[order[p]] == chrom[k] and abs(int(bp[order[p]]) - int(bp[k])) <= window_bp:
                    pairs[k, order[p]] = True
                    if link[k, order[p]]:
                        mine.append(order[p])
                    p += step
            neigh.append(np.array(sorted(mine), dtype=np.int64))
    index_of = np.full(n, -1, dtype=np.int32)
    for k in range(n):
        if index_of[k] >= 0:
            continue
        index_of[k] = k
        for j in neigh[k]:
            if index_of[j] < 0:
                index_of[j] = k
    pairs = pairs & (den > 0)
    np.fill_diagonal(pairs, False)
    if pairs.any():
        ft = Fraction(t)
        r2 = to_longdouble(Nm[pairs]) ** 2 / to_longdouble(den[pairs])
        margin = float(np.min(np.abs(r2 - np.longdouble(ft.numerator) / np.longdouble(ft.denominator))) / t)
    else:
        margin = np.inf
    return index_of, margin


# ------------------------------------------------------------------------------- test_dat inputs
def summary_candidates(summ_path: str, bim_path: str, pth: float):
    """The CLI's candidate list (software/DBSLMM.R:132-134 restated): z = beta / se (columns 9, 10 of
    the GEMMA summary, 0 when se is not a positive number), p = erfc(|z| / sqrt 2); the summary SNPs
    found in the .bim with p <= pth, by descending |z|, ties by summary line.  Returns a dict of
    parallel arrays in that priority order: snp, line (summary line), row (.bim line = bed row),
    chrom (int code per distinct .bim chromosome string, by first appearance), bp, z, p."""
    import math
    bim = {}
    chrom_code = {}
    for r, line in enumerate(open(bim_path)):
        f = line.rstrip("\n").split("\t")
        if len(f) < 6 or f[1] in bim:
            continue
        bim[f[1]] = (r, chrom_code.setdefault(f[0], len(chrom_code)), int(f[3]))
    cand = []
    for i, line in enumerate(open(summ_path)):
        f = line.rstrip("\n").split("\t")
        if len(f) < 11:
            continue
        z = 0.0
        if f[9][:1].isdigit() and float(f[9]) > 1e-20:
            z = float(f[8]) / float(f[9])
        p = math.erfc(abs(z) / math.sqrt(2.0))
        if f[1] in bim and p <= pth:
            cand.append((-abs(z), i, f[1], z, p))
    cand.sort(key=lambda c: (c[0], c[1]))
    rows = [bim[c[2]] for c in cand]
    return dict(snp=[c[2] for c in cand], line=np.array([c[1] for c in cand], dtype=np.int64),
                row=np.array([r[0] for r in rows], dtype=np.int32), chrom=np.array([r[1] for r in rows], dtype=np.int32),
                bp=np.array([r[2] for r in rows], dtype=np.int64), z=np.array([c[3] for c in cand]),
                p=np.array([c[4] for c in cand]))
