"""dbslmm_ld_scores (ldscore.hip: dbslmm_l2_tiles, dbslmm_l2_reduce; ldsc_layout.hpp) on the GPU and the
CLI's --ldsc mode, against tests/_ldsc_ref.py: r2 in longdouble from the exact integers, the window
decided on integers, the terms summed in longdouble.

The bar of an LD score (u = 2^-53), from the kernel's roundings, not from what it returns.  l_k is a
sum of T_k terms t_kj, each computed from one r2:

* r2 of a pair in a RAW tile (no missing call among the 256 rows of its 128 x 128 tile) is
  dbslmm_r2_tiles' raw form: exact int64 N and D, three roundings, within 4 ulp(r2)
  (tests/test_clump.py).  r2 of a pair in a FOUR-PRODUCT tile (a missing call among the rows of
  its tile row or tile column) is within `four_product_bar` of tests/test_clump.py, whose
  derivation stands unchanged: the expressions are the same.
* the adjustment (unbiased): t = fl(fl(r2 (n - 1) - 1) / (n - 2)), the inner one fma.  n - 1 and n - 2
  are exact.  An error e of r2 becomes e (n - 1) / (n - 2) = e (1 + 1 / (n - 2)) of t; the fma rounds
  (n - 2) t once and the division once more: 2 u |t|.  So per term
      delta = bar(r2) (1 + 1 / (n - 2)) + 2 u |t|
  and delta = bar(r2) without the adjustment (t = r2 itself).
* the summation: T terms added in any order -- lane butterflies, the four parts of a tile, the
  slots of the tiles, each partial sum at most sum |t| -- make at most (T - 1) roundings of at most
  u sum |t| each to first order.
      Bar_k = 1.01 [ sum_j delta_kj + (T_k - 1) u sum_j |t_kj| ] + 2^-60 sum_j |t_kj|
  (1.01: the second-order terms; 2^-60: the longdouble reference's own roundings).
* NaN exactly where the row's own r2 is NaN (no variance or no observed call), and such a row adds
  nothing to any other row; n_window exact.

Each case prints the worst observed |got - ref| / Bar; DESIGN.md section 3.9 records them.  Each
case also asserts from the reference alone that Bar / l < 1e-9 wherever l > 1e-3."""
import functools
import os
import subprocess

import numpy as np
import pytest

import _clump_ref as CR
import _ldsc_ref as LR
from _common import TD, load_bed
from test_clump import _rows, four_product_bar
from test_gram_range import N_CAP, _bed_of, _cap_dosages, flip_alleles

gpu = pytest.mark.gpu
LD = np.longdouble
U = LD(2.0) ** -53
SUMM = os.path.join(TD, "summary_gemma_chr1.assoc.txt")
REF = os.path.join(TD, "ref_chr1")
N_ROWS = 300


@functools.lru_cache(maxsize=None)
def _ctx():
    from dbslmm_amd import Context
    return Context(0)


def l2_bar(ref: dict, X, chrom, bp, unbiased, n_ref, fpbar=None, fp=None):
    """(Bar per row, four-product pair mask) of the module docstring; fpbar: four_product_bar of
    every pair of X when the caller already has it; fp: the four-product pair mask when the rows are
    part of a longer list (the tiles are those of the whole call's position order)"""
    if fp is None:
        fp = LR.four_product_pairs128((np.asarray(X) < 0).sum(axis=1), chrom, bp)
    r2, t, used = ref["r2"], ref["t"], ref["used"]
    with np.errstate(invalid="ignore"):
        rbar = 4 * np.spacing(np.abs(r2.astype(np.float64))).astype(LD)
        if fp.any():
            rbar = np.where(fp, four_product_bar(X, r2) if fpbar is None else fpbar, rbar)
        if unbiased:
            delta = rbar * (1 + 1 / LD(n_ref - 2)) + 2 * U * np.abs(t)
        else:
            delta = rbar
    sum_delta = np.where(used, delta, LD(0)).sum(axis=1, dtype=LD)
    T = ref["n_terms"].astype(LD)
    bar = LD(1.01) * (sum_delta + np.maximum(T - 1, 0) * U * ref["sum_abs"]) + LD(2.0) ** -60 * ref["sum_abs"]
    return bar, fp


def check_l2(got, got_nw, X, chrom, bp, window_bp, unbiased, n_ref, what, r2=None, fpbar=None):
    """got = ld_scores of the rows X (caller order) against the reference, every row at its bar"""
    ref = LR.ld_scores_ref(X, chrom, bp, window_bp, unbiased, n_ref, r2=r2)
    np.testing.assert_array_equal(got_nw, ref["n_window"], err_msg=f"{what}: n_window")
    nan = ref["nan_row"]
    np.testing.assert_array_equal(np.isnan(got), nan, err_msg=f"{what}: NaN pattern")
    bar, fp = l2_bar(ref, X, chrom, bp, unbiased, n_ref, fpbar)
    ok = ~nan
    err = np.abs(got.astype(LD) - ref["l2"])
    uses_fp = (fp & ref["used"]).any(axis=1)
    worst = {}
    for name, sel in (("raw", ok & ~uses_fp), ("four-product", ok & uses_fp)):
        if sel.any():
            worst[name] = float(np.max(err[sel] / bar[sel]))
    print(f"{what}: n {len(X)}, worst |got - ref| / bar {worst}")
    big = ok & (ref["l2"] > 1e-3)
    if big.any():                                  # the bar still says something (from the reference alone)
        assert float(np.max(bar[big] / ref["l2"][big])) < 1e-9
    assert np.all(err[ok] <= bar[ok]), (what, worst)
    return ref, bar, worst


@functools.lru_cache(maxsize=None)
def _edge_panel(n_ref, with_missing):
    """300 rows at n_ref individuals in LD runs of 4, among them flipped (major-allele) rows, a
    monomorphic row and a repeated row; with_missing: rows 130..259 carry 8 % missing calls, one of
    them all missing and one without variance among its observed calls.  Returns bed, X, r2 of every
    pair (longdouble) and their four-product bars."""
    rng = np.random.default_rng(1000 + 2 * n_ref + with_missing)
    X = _rows(rng, N_ROWS, n_ref)
    if with_missing:
        sub = X[130:260]
        sub[rng.random(sub.shape) < 0.08] = -1
        X[200] = -1                                # all missing
        X[201, X[201] >= 0] = 1                    # no variance among the observed calls
    X[7] = 2                                       # monomorphic
    X[40] = X[39]                                  # a repeat
    X[290] = X[3]                                  # ... and one two tile rows away
    bed = flip_alleles(CR.encode(X), n_ref, np.arange(1, N_ROWS, 3))
    X = CR.decode(bed, n_ref, np.arange(N_ROWS))
    X.setflags(write=False)
    r2 = CR.r2_longdouble(X)
    fpbar = four_product_bar(X, r2) if with_missing else None
    return bed, X, r2, fpbar


def _sub(r2, fpbar, n):
    return r2[:n, :n], (None if fpbar is None else fpbar[:n, :n])


@gpu
@pytest.mark.parametrize("n_ref,with_missing", [(3, False)] + [(n, m) for n in (255, 256, 257, 400, 4097) for m in (False, True)] +
                         [(513, False), (769, False)])
def test_ld_scores_shape_edges(n_ref, with_missing):
    """n_rows 1, 127, 128, 129, 256, 257, 300 at every n_ref (pad individuals, pad bits, kpad 256 / 512 /
    4352, and 768 / 1024 on the raw list: 1, 2, 17, 3 and 4 K stages of 256 individuals -- 3 is odd with
    one load ahead only, 4 the smallest even count that loads stage st + 3; one, two and three tile
    rows, whole and partial), rows 1 kb apart under a 150 kb window (a band two tile columns wide at
    300 rows), with and without ldsc's adjustment.  Without missing calls every tile is raw; with them
    the 300-row list mixes raw tile (0, 0) with four-product tiles.  n_ref = 3 (n - 2 = 1) runs on the
    raw list only: unbiased = 0, plus one call with the adjustment."""
    from dbslmm_amd import ld_r2, ld_scores
    bed, X, r2, fpbar = _edge_panel(n_ref, with_missing)
    worst = {}
    for n_rows in (1, 127, 128, 129, 256, 257, 300):
        rows = np.arange(n_rows, dtype=np.int32)
        chrom, bp = np.ones(n_rows, dtype=np.int32), 1000 * np.arange(n_rows, dtype=np.int64)
        s_r2, s_fp = _sub(r2, fpbar, n_rows)
        for unbiased in ((False,) if n_ref == 3 and n_rows != 300 else (False, True)):
            got, nw = ld_scores(_ctx(), bed, n_ref, rows, chrom, bp, kb=150, unbiased=unbiased)
            _, _, w = check_l2(got, nw, X[:n_rows], chrom, bp, 150_000, unbiased, n_ref,
                               f"n_ref {n_ref} missing {with_missing} n_rows {n_rows} unbiased {unbiased}", s_r2, s_fp)
            for k, v in w.items():
                worst[k] = max(worst.get(k, 0.0), v)
        if n_rows <= 257:
            # a covering window, no adjustment: the row sums of ld_r2 on the same rows
            got, nw = ld_scores(_ctx(), bed, n_ref, rows, chrom, bp, kb=1000, unbiased=False)
            ref, bar, _ = check_l2(got, nw, X[:n_rows], chrom, bp, 1_000_000, False, n_ref,
                                   f"n_ref {n_ref} covering n_rows {n_rows}", s_r2, s_fp)
            assert np.all(nw == n_rows)
            dense = ld_r2(_ctx(), bed, n_ref, rows).astype(LD)
            ok = ~ref["nan_row"]
            sums = np.where(ok[None, :], dense, LD(0)).sum(axis=1, dtype=LD)
            assert np.all(np.abs(got.astype(LD) - sums)[ok] <= bar[ok])
    print(f"shape edges n_ref {n_ref} missing {with_missing}: worst of all {worst}")
    if n_ref > 3:
        got, _ = ld_scores(_ctx(), bed, n_ref, np.arange(N_ROWS), np.ones(N_ROWS), 1000 * np.arange(N_ROWS), kb=150)
        assert np.isnan(got[7]) and not np.isnan(got[[6, 8, 39, 40]]).any()
        if with_missing:
            assert np.isnan(got[200]) and np.isnan(got[201])
            assert set(worst) == {"raw", "four-product"}


def _band_width(chrom, bp, window_bp):
    """tile columns the band spans, from the positions alone"""
    order = LR.position_order(chrom, bp)
    rank = np.empty(len(order), dtype=np.int64)
    rank[order] = np.arange(len(order))
    W = LR.window_matrix(chrom, bp, window_bp)
    i, j = np.nonzero(W)
    return int(np.max(np.abs(rank[i] // 128 - rank[j] // 128))) + 1


WINDOW_CASES = {
    # name: (chrom, bp, window_bp, band width in tile columns)
    "one column, gaps wider than the window": (np.ones(N_ROWS), 1000 * np.arange(N_ROWS) + 10_000_000 * (np.arange(N_ROWS) // 128),
                                               50_000, 1),
    "two columns": (np.ones(N_ROWS), 1000 * np.arange(N_ROWS), 100_000, 2),
    "three columns": (np.ones(N_ROWS), 1000 * np.arange(N_ROWS), 200_000, 3),
    "window 0, runs of equal bp": (np.ones(N_ROWS), 1000 * (np.arange(N_ROWS) // 5), 0, 2),
    "two chromosomes sharing bp": (1 + np.arange(N_ROWS) % 2, 1000 * (np.arange(N_ROWS) // 2), 100_000, 2),
}


@gpu
@pytest.mark.parametrize("name", list(WINDOW_CASES))
def test_ld_scores_windows(name):
    from dbslmm_amd import ld_scores
    n_ref = 400
    bed, X, r2, fpbar = _edge_panel(n_ref, True)
    chrom, bp, window_bp, width = WINDOW_CASES[name]
    chrom, bp = chrom.astype(np.int32), bp.astype(np.int64)
    assert _band_width(chrom, bp, window_bp) == width
    got, nw = ld_scores(_ctx(), bed, n_ref, np.arange(N_ROWS), chrom, bp, kb=window_bp / 1000)
    check_l2(got, nw, X, chrom, bp, window_bp, True, n_ref, name, r2, fpbar)
    if name.startswith("window 0"):
        assert np.all(nw == 5)
    if name.startswith("two chromosomes"):
        assert nw.max() <= 150                   # never across the chromosomes


@gpu
def test_ld_scores_in_any_caller_order():
    """rows in shuffled caller order (distinct positions, so the position order is the same list):
    the sorted call's result, permuted, bit for bit; repeated rows allowed"""
    from dbslmm_amd import ld_scores
    n_ref = 400
    bed, X, r2, fpbar = _edge_panel(n_ref, True)
    chrom = (1 + np.arange(N_ROWS) // 170).astype(np.int32)
    bp = (1000 * (np.arange(N_ROWS) % 170)).astype(np.int64)
    rows = np.arange(N_ROWS, dtype=np.int32)
    rows[17] = 16                                   # a bed row listed twice
    a, nwa = ld_scores(_ctx(), bed, n_ref, rows, chrom, bp, kb=60)
    perm = np.random.default_rng(5).permutation(N_ROWS)
    b, nwb = ld_scores(_ctx(), bed, n_ref, rows[perm], chrom[perm], bp[perm], kb=60)
    assert b.tobytes() == a[perm].tobytes()
    np.testing.assert_array_equal(nwb, nwa[perm])
    check_l2(b, nwb, X[rows[perm]], chrom[perm], bp[perm], 60_000, True, n_ref, "shuffled")


@gpu
def test_ld_scores_slices_and_repeats_give_the_same_bytes():
    """max_tiles_per_launch 1, 2, 3 and the default on the three-column band (6 tiles), and two
    consecutive calls: byte-identical"""
    from dbslmm_amd import ld_scores
    n_ref = 400
    bed, X, r2, fpbar = _edge_panel(n_ref, True)
    chrom, bp, window_bp, _ = WINDOW_CASES["three columns"]
    rows = np.arange(N_ROWS)
    base, nw = ld_scores(_ctx(), bed, n_ref, rows, chrom, bp, kb=window_bp / 1000)
    check_l2(base, nw, X, chrom.astype(np.int32), bp.astype(np.int64), window_bp, True, n_ref, "slices", r2, fpbar)
    for mt in (1, 2, 3, 0):
        got, nw2 = ld_scores(_ctx(), bed, n_ref, rows, chrom, bp, kb=window_bp / 1000, max_tiles=mt)
        assert got.tobytes() == base.tobytes(), mt
        np.testing.assert_array_equal(nw2, nw)


# ------------------------------------------------------------------------------------------------
# a ragged band: the tile rows reach 0, 1, 2 and 3 tile columns past the diagonal, up and down
# ------------------------------------------------------------------------------------------------
RAGGED_N, RAGGED_WINDOW = 900, 100_000


def _ragged_bp():
    """bp of 900 positions (8 tile rows, the last one 4 positions): stretches 900, 240, 1500 and 800 bp
    apart (111, 416, 66 and 125 rows inside a 100 kb window) and 500 kb of nothing between positions 599 and 600 (inside tile row 4) and 300 kb after position 639 (where it ends)"""
    d = np.zeros(RAGGED_N, dtype=np.int64)
    for a, b, step in ((0, 200, 900), (200, 520, 240), (520, 640, 1500), (640, RAGGED_N, 800)):
        d[a:b] = step
    d[600], d[640] = 500_000, 300_000
    return np.cumsum(d)


def _ragged_two_chromosomes():
    """the same rows, positions 450.. on a second chromosome whose bp start again: the change falls
    inside tile row 3 (positions 384..511)"""
    bp = _ragged_bp()
    chrom = np.where(np.arange(RAGGED_N) < 450, 1, 2)
    return chrom, np.where(chrom == 1, bp, bp - bp[450] + 1000)


RAGGED_CASES = {
    # name: (chrom, bp, reach of every tile row: hi(last p of I) / 128 - I)
    "one chromosome": (np.ones(RAGGED_N, dtype=np.int64), _ragged_bp(), [2, 3, 2, 1, 0, 1, 1, 0]),
    "two chromosomes, the change inside a tile": _ragged_two_chromosomes() + ([2, 2, 1, 1, 0, 1, 1, 0],),
}
RAGGED_MISSING = (380, 520)        # caller rows (= positions) with missing calls: tile rows 2, 3 and 4


def tile_row_reach(chrom, bp, window_bp):
    """per tile row I of the position order, the tile columns its last position's window reaches past
    the diagonal: from the oracle's order and window matrix alone"""
    order = LR.position_order(chrom, bp)
    W = LR.window_matrix(chrom, bp, window_bp)[np.ix_(order, order)]
    n = len(order)
    return [int(np.flatnonzero(W[min(n, 128 * (I + 1)) - 1]).max()) // 128 - I for I in range((n + 127) // 128)]


@functools.lru_cache(maxsize=None)
def _ragged_panel():
    """900 rows at n_ref 400 in LD runs of 4; rows 380..519 carry 8 % missing calls, one of them all
    missing; a monomorphic row among the others; flipped rows.  bed, X, r2, four-product bars."""
    n_ref = 400
    rng = np.random.default_rng(77)
    X = _rows(rng, RAGGED_N, n_ref)
    sub = X[RAGGED_MISSING[0]:RAGGED_MISSING[1]]
    sub[rng.random(sub.shape) < 0.08] = -1
    X[400] = -1                                    # all missing
    X[50] = 2                                      # monomorphic, in a raw tile
    bed = flip_alleles(CR.encode(X), n_ref, np.arange(1, RAGGED_N, 3))
    X = CR.decode(bed, n_ref, np.arange(RAGGED_N))
    X.setflags(write=False)
    r2 = CR.r2_longdouble(X)
    return bed, X, r2, four_product_bar(X, r2)


@gpu
@pytest.mark.parametrize("name", list(RAGGED_CASES))
def test_ld_scores_ragged_band(name):
    """dbslmm_l2_reduce finds tile (I, P) at row_ptr[I] + (P - I) and starts at col_lo[P]: a band whose
    width changes from tile row to tile row (tests/test_ldsc_host.py asserts the reaches from the
    positions alone), raw and four-product tiles in it.  Every row at its bar with and without the
    adjustment, n_window exact, and the bytes of the whole launch for slices of 1, 5 and 7 tiles and
    for a shuffled caller order."""
    from dbslmm_amd import ld_scores
    n_ref = 400
    bed, X, r2, fpbar = _ragged_panel()
    chrom, bp, _ = RAGGED_CASES[name]
    chrom, bp = chrom.astype(np.int32), bp.astype(np.int64)
    rows = np.arange(RAGGED_N, dtype=np.int32)
    base = {}
    for unbiased in (True, False):
        got, nw = ld_scores(_ctx(), bed, n_ref, rows, chrom, bp, kb=RAGGED_WINDOW / 1000, unbiased=unbiased)
        _, _, worst = check_l2(got, nw, X, chrom, bp, RAGGED_WINDOW, unbiased, n_ref, f"ragged, {name}, unbiased {unbiased}",
                               r2, fpbar)
        assert set(worst) == {"raw", "four-product"}
        assert np.isnan(got[50]) and np.isnan(got[400]) and int(np.isnan(got).sum()) == 2
        base[unbiased] = (got, nw)
    got, nw = base[True]
    for mt in (1, 5, 7, 0):
        g2, nw2 = ld_scores(_ctx(), bed, n_ref, rows, chrom, bp, kb=RAGGED_WINDOW / 1000, max_tiles=mt)
        assert g2.tobytes() == got.tobytes(), mt
        np.testing.assert_array_equal(nw2, nw)
    perm = np.random.default_rng(9).permutation(RAGGED_N)
    for mt in (0, 5):
        g3, nw3 = ld_scores(_ctx(), bed, n_ref, rows[perm], chrom[perm], bp[perm], kb=RAGGED_WINDOW / 1000, max_tiles=mt)
        assert g3.tobytes() == got[perm].tobytes(), mt
        np.testing.assert_array_equal(nw3, nw[perm])


@gpu
def test_ld_scores_at_the_n_ref_cap():
    """n_ref = 1 863 936, the 40 rows of test_gram_range's cap panel, with the adjustment"""
    from dbslmm_amd import ld_scores
    dos = _cap_dosages()
    n = len(dos)
    chrom, bp = np.ones(n, dtype=np.int32), np.arange(n, dtype=np.int64)
    got, nw = ld_scores(_ctx(), _bed_of(dos), N_CAP, np.arange(n), chrom, bp, kb=1000, unbiased=True)
    check_l2(got, nw, dos, chrom, bp, 1_000_000, True, N_CAP, "cap")


@gpu
def test_ld_scores_none_one_and_argument_errors():
    from dbslmm_amd import DbslmmError, ld_scores
    bed, X, _, _ = _edge_panel(400, False)
    e = np.zeros(0, dtype=np.int32)
    l2, nw = ld_scores(_ctx(), bed, 400, e, e, e)
    assert l2.shape == (0,) and nw.shape == (0,)
    l2, nw = ld_scores(_ctx(), bed, 400, [5], [1], [100])
    assert l2[0] == 1.0 and nw[0] == 1
    l2, nw = ld_scores(_ctx(), bed, 400, [7], [1], [100])          # a monomorphic row alone
    assert np.isnan(l2[0]) and nw[0] == 1
    bed3, _, _, _ = _edge_panel(3, False)
    for call in (lambda: ld_scores(_ctx(), bed, 400, [0, N_ROWS], [1, 1], [1, 2]),
                 lambda: ld_scores(_ctx(), bed, 400, [-1], [1], [1]),
                 lambda: ld_scores(_ctx(), bed, 400, [0], [1], [1], kb=-1),
                 lambda: ld_scores(_ctx(), bed, 400, [0], [1], [1], max_tiles=-1),
                 lambda: ld_scores(_ctx(), bed, N_CAP + 1, [0], [1], [1]),
                 lambda: ld_scores(_ctx(), bed3[:3 + 1], 2, [0], [1], [1], unbiased=True)):
        with pytest.raises(DbslmmError) as ei:
            call()
        assert "rc=-1" in str(ei.value), str(ei.value)


@gpu
def test_ld_scores_multi_device_context_and_cached_image():
    """a context over [0, 0] answers from its first device, and a context's cached image serves the
    same answer: the bytes of a one-device context"""
    from dbslmm_amd import Context, ld_scores
    n_ref = 400
    bed, _, _, _ = _edge_panel(n_ref, True)
    chrom, bp, window_bp, _ = WINDOW_CASES["two columns"]
    rows = np.arange(N_ROWS)
    a, nwa = ld_scores(_ctx(), bed, n_ref, rows, chrom, bp, kb=window_bp / 1000)
    b, nwb = ld_scores(Context([0, 0]), bed, n_ref, rows, chrom, bp, kb=window_bp / 1000)
    assert a.tobytes() == b.tobytes() and nwa.tobytes() == nwb.tobytes()
    ctx = Context(0)
    ctx.cache_bed(bed)
    c, _ = ld_scores(ctx, bed, n_ref, rows, chrom, bp, kb=window_bp / 1000)
    assert a.tobytes() == c.tobytes()


# ------------------------------------------------------------------------------------------------
# CLI
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _td_oracle():
    """test_dat at 50 kb: the oracle's LD scores, their bars, M_5_50 and the regression inputs"""
    td = LR.test_dat_inputs(SUMM, REF)
    X = CR.decode(load_bed(REF + ".bed"), 400, np.arange(len(td["bp"])))
    ref = LR.ld_scores_ref(X, td["chrom"], td["bp"], 50_000, True, 400)
    bar, _ = l2_bar(ref, X, td["chrom"], td["bp"], True, 400)
    maf = np.minimum(X.sum(axis=1) / 800.0, 1 - X.sum(axis=1) / 800.0)
    M = int((~ref["nan_row"] & (maf > 0.05)).sum())
    return td, ref, bar, M


def _h2_file(path):
    return {l.split()[0]: l.split()[1:] for l in open(path).read().splitlines()}


@gpu
@pytest.mark.parametrize("intercept", [None, 1.0])
def test_cli_ldsc_on_test_dat(intercept, tmp_path):
    """dbslmm --ldsc on test_dat at --ld-wind-kb 50: every L2 of the .l2.ldscore within its bar + the
    %.10g of the file, M_5_50 the oracle's count, the .h2.txt values within rtol 1e-6 of the oracle's
    regression on the oracle's LD scores; a two-panel call doubles M and n_snp."""
    from test_cli import CLI
    td, ref, bar, M = _td_oracle()
    out = str(tmp_path / "o")
    extra = [] if intercept is None else ["--intercept", str(intercept)]
    r = subprocess.run([CLI, "--ldsc", "--summary", SUMM, "-r", REF, "--out", out, "--ld-wind-kb", "50"] + extra,
                       capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
    assert r.returncode == 0, r.stderr
    lines = [l.split("\t") for l in open(out + ".l2.ldscore").read().splitlines()]
    assert lines[0] == ["CHR", "SNP", "BP", "L2"] and len(lines) == 1 + 723
    assert [l[1] for l in lines[1:]] == td["snp"] and [int(l[2]) for l in lines[1:]] == list(td["bp"])
    got = np.array([float(l[3]) for l in lines[1:]])
    assert not np.isnan(got).any()
    err = np.abs(got.astype(LD) - ref["l2"])
    print(f"cli test_dat: worst |got - ref| / (bar + 1e-9 l) {float(np.max(err / (bar + LD(1e-9) * np.abs(ref['l2'])))):.3g}")
    assert np.all(err <= bar + LD(1e-9) * np.abs(ref["l2"]))
    assert int(open(out + ".l2.M_5_50").read()) == M
    sel = td["summ_of"] >= 0
    chi2, nobs = td["z"][td["summ_of"][sel]] ** 2, td["n_obs"][td["summ_of"][sel]]
    fit = LR.ldsc_fit_ref(chi2, nobs, ref["l2"][sel].astype(np.float64), M, intercept=intercept)
    assert fit["status"] == 0
    h = _h2_file(out + ".h2.txt")
    np.testing.assert_allclose([float(v) for v in h["h2"]], [fit["h2"], fit["h2_se"]], rtol=1e-6)
    if intercept is None:
        np.testing.assert_allclose([float(v) for v in h["intercept"]], [fit["intercept"], fit["intercept_se"]], rtol=1e-6)
    else:
        assert h["intercept"] == ["1", "fixed"]
    assert int(h["M"][0]) == M and int(h["n_snp"][0]) == int(sel.sum()) == 722
    np.testing.assert_allclose(float(h["mean_chi2"][0]), fit["mean_chi2"], rtol=1e-6)
    if intercept is None:
        out2 = str(tmp_path / "o2")
        r = subprocess.run([CLI, "--ldsc", "--summary", SUMM + "," + SUMM, "-r", REF + "," + REF, "--out", out2,
                            "--ld-wind-kb", "50"], capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
        assert r.returncode == 0, r.stderr
        h2 = _h2_file(out2 + ".h2.txt")
        assert int(h2["M"][0]) == 2 * M and int(h2["n_snp"][0]) == 2 * 722
        assert len(open(out2 + ".l2.ldscore").read().splitlines()) == 1 + 2 * 723
