"""dbslmm_ld_r2 and dbslmm_clump (clump.hip: dbslmm_r2_tiles; clump_layout.hpp) on the GPU, and the
CLI's --summary / --pth path, against tests/_clump_ref.py: exact integers, longdouble values, exact
threshold decisions.

Bars of ld_r2 (u = 2^-53), from the kernel's epilogues, not from what it returns:

* a pair computed in a RAW tile (no row of the tile's 64 has a missing call): N, D_i, D_j are exact
  int64, their conversions exact (< 2^53), and r2 = fl(fl(N N) / fl(D_i D_j)) has three roundings,
  3 u relative, so |got - ref| <= 4 ulp(ref) (an ulp is at least 2^-53 |ref|).  The diagonal and a
  repeated row are fl(x) / fl(x) = 1 exactly.
* a pair computed in a FOUR-PRODUCT tile: with the exact integers of _clump_ref.sums and mu = S / m,
      c   = ((GG - mu_j GO) - mu_i OG) + (mu_i mu_j) (OO - pad_k)
      css = sq - S S / m,   r2 = c c / (css_i css_j).
  mu carries u; mu_j GO and mu_i OG 2 u of themselves; (mu_i mu_j) OO' 4 u; the three additions u
  each of a partial sum that A = GG + mu_j GO + mu_i OG + mu_i mu_j OO' bounds: |dc| <= 7 u A to
  first order, dc = 8 u A here.  S S is exact, S S / m rounds once, the subtraction once:
  |dcss| <= u (S^2 / m + css), e_i = dcss_i / css_i.  The squaring, the product of the css and the
  division add u each:
      |got - ref| <= 1.01 [ (2 |c| dc + dc^2) / (css_i css_j) + r2 (e_i + e_j + 3 u) ] + 2^-60 r2
  (1.01: the second-order terms, each at most u of a first-order one; 2^-60: the longdouble
  reference's own roundings).  A contraction of a product and an addition into one fma drops a
  rounding, never adds one.
* NaN exactly where the reference's denominator is 0 (a row without variance or observed call).

The worst observed |got - ref| / bar of each case is printed; DESIGN.md section 3.8 records them.
Clumping decisions are not held to a tolerance: every case asserts the oracle's margin (the smallest
|r2 - t| / t over its in-window pairs) >= 1e-9 from the exact integers, then compares index_of whole."""
import functools
import os
import subprocess

import numpy as np
import pytest

import _clump_ref as CR
from _common import BLOCKS_EUR1, TD, load_bed
from test_gram_range import N_CAP, _bed_of, _cap_dosages, flip_alleles

gpu = pytest.mark.gpu
LD = np.longdouble
U = LD(2.0) ** -53
SUMM = os.path.join(TD, "summary_gemma_chr1.assoc.txt")
REF = os.path.join(TD, "ref_chr1")
MIN_MARGIN = 1e-9


@functools.lru_cache(maxsize=None)
def _ctx():
    from dbslmm_amd import Context
    return Context(0)


# ------------------------------------------------------------------------------------------------
# ld_r2 values
# ------------------------------------------------------------------------------------------------
def _rows(rng, n_rows, n_ref, miss=0.0):
    """random dosage rows, allele frequency U(0.05, 0.95) per row, in LD runs of 4 (a row copies its
    predecessor's call with probability 0.7)"""
    X = np.zeros((n_rows, n_ref), dtype=np.int8)
    for r in range(n_rows):
        X[r] = rng.binomial(2, rng.uniform(0.05, 0.95), size=n_ref)
        if r % 4:
            keep = rng.random(n_ref) < 0.7
            X[r, keep] = X[r - 1, keep]
    if miss:
        X[rng.random(X.shape) < miss] = -1
    return X


def four_product_pairs(nmiss):
    """[i, j] True where the library computes the pair in a four-product tile: a row with a missing
    call among the list's rows of tile row i // 32 or of tile row j // 32"""
    n = len(nmiss)
    blk = np.arange(n) // 32
    bm = np.array([np.any(nmiss[blk == b] > 0) for b in range(blk.max() + 1)])
    return bm[blk][:, None] | bm[blk][None, :]


def four_product_bar(X, ref):
    """the bar of the module docstring for every pair of rows X (longdouble; NaN where ref is)"""
    s = CR.sums(X)
    S, sq, m = s["S"].astype(LD), s["sq"].astype(LD), s["m"].astype(LD)
    with np.errstate(invalid="ignore", divide="ignore"):
        mu = S / m
        css = sq - S * S / m
        GG, GO, OG, OO = (s[k].astype(LD) for k in ("GG", "GO", "OG", "OO"))   # OO over the individuals: OO - pad_k
        mi, mj = mu[:, None], mu[None, :]
        A = GG + mj * GO + mi * OG + mi * mj * OO
        c = GG - mj * GO - mi * OG + mi * mj * OO
        dc = 8 * U * A
        e = U * (S * S / m + css) / css
        dd = css[:, None] * css[None, :]
        return LD(1.01) * ((2 * np.abs(c) * dc + dc * dc) / dd + ref * (e[:, None] + e[None, :] + 3 * U)) + \
            LD(2.0) ** -60 * ref


def check_r2(got, X, what):
    """got = ld_r2 of the rows X (in list order) against the reference, every pair at its bar"""
    n = len(X)
    assert got.shape == (n, n)
    ref = CR.r2_longdouble(X)
    nan = np.isnan(ref)
    np.testing.assert_array_equal(np.isnan(got), nan, err_msg=f"{what}: NaN pattern")
    assert np.array_equal(got, got.T, equal_nan=True), f"{what}: not symmetric"
    fp = four_product_pairs(CR.sums(X)["nmiss"])
    err = np.abs(got.astype(LD) - ref)
    raw_bar = 4 * np.spacing(ref.astype(np.float64)).astype(LD)
    fp_bar = four_product_bar(X, ref) if fp.any() else raw_bar
    bar = np.where(fp, fp_bar, raw_bar)
    ok = ~nan
    worst = {}
    for name, sel in (("raw", ok & ~fp), ("four-product", ok & fp)):
        if sel.any():
            worst[name] = float(np.max(err[sel] / bar[sel]))
    print(f"{what}: n {n}, worst |got - ref| / bar {worst}")
    assert np.all(err[ok] <= bar[ok]), (what, worst)
    if (ok & fp).any():                        # the bar still says something (from the reference alone)
        big = ok & fp & (ref > 1e-3)
        if big.any():
            assert float(np.max(bar[big] / ref[big])) < 1e-9
    d = np.arange(n)
    raw_diag = ok[d, d] & ~fp[d, d]
    assert np.all(got[d, d][raw_diag] == 1.0)
    return worst


@functools.lru_cache(maxsize=None)
def _edge_panel(n_ref):
    """130 rows at n_ref individuals: 0..64 without a missing call, 65..129 with (8 % of the calls; 20 % at
    n_ref = 3), among them flipped (major-allele), monomorphic and all-missing rows"""
    rng = np.random.default_rng(100 + n_ref)
    X = np.concatenate([_rows(rng, 65, n_ref), _rows(rng, 65, n_ref, 0.08 if n_ref > 3 else 0.2)])
    X[7] = 2                                   # monomorphic (raw list)
    X[40] = X[39]                              # a repeat
    X[70] = -1                                 # all missing
    X[71, X[71] >= 0] = 1                      # no variance among the observed calls
    bed = flip_alleles(CR.encode(X), n_ref, np.arange(1, 130, 3))
    X = CR.decode(bed, n_ref, np.arange(130))
    X.setflags(write=False)
    return bed, X


@gpu
@pytest.mark.parametrize("n_ref", [3, 255, 256, 257, 400, 513, 769, 4097])
def test_ld_r2_shape_edges(n_ref):
    """n_rows 1, 31, 32, 33, 64, 65 at every n_ref (pad individuals, pad bits, kpad steps 256 / 512 /
    768 / 1024 / 4352): a list without a missing call (raw tiles) and one with (four-product tiles), each holding
    flipped rows, a monomorphic row and, the second, an all-missing row and one without variance:
    NaN row, column and diagonal."""
    from dbslmm_amd import ld_r2
    bed, X = _edge_panel(n_ref)
    for lo in (0, 65):
        for n_rows in (1, 31, 32, 33, 64, 65):
            rows = np.arange(lo, lo + n_rows)
            got = ld_r2(_ctx(), bed, n_ref, rows)
            check_r2(got, X[rows], f"n_ref {n_ref} rows {lo}..{lo + n_rows - 1}")
    got = ld_r2(_ctx(), bed, n_ref, np.arange(65))
    assert np.all(np.isnan(got[7])) and np.all(np.isnan(got[:, 7]))
    if n_ref > 3:
        assert got[39, 40] == 1.0 and got[40, 39] == 1.0
    got = ld_r2(_ctx(), bed, n_ref, np.arange(65, 130))
    for r in (5, 6):
        assert np.all(np.isnan(got[r])) and np.all(np.isnan(got[:, r]))


@gpu
def test_ld_r2_rows_repeat_and_any_order():
    """the list is a gather: rows in any order, a row listed twice (r2 = 1 with its twin, raw path)"""
    from dbslmm_amd import ld_r2
    bed, X = _edge_panel(400)
    rows = np.array([12, 3, 12, 60, 0, 33, 3], dtype=np.int32)
    got = ld_r2(_ctx(), bed, 400, rows)
    check_r2(got, X[rows], "repeats")
    assert got[0, 2] == 1.0 and got[1, 6] == 1.0


@gpu
def test_ld_r2_mixed_tiles():
    """96 rows of which only rows 32..63 hold missing calls: tiles (0, 0), (0, 2), (2, 2) take the raw
    form, the others the four products; every pair at its own bar, and a pair of rows without a
    missing call has in a raw tile of the long list the bits ld_r2 returns for just that pair."""
    from dbslmm_amd import ld_r2
    n_ref = 400
    bed, X = _edge_panel(n_ref)
    rows = np.concatenate([np.arange(0, 32), np.arange(65, 97), np.arange(32, 64)]).astype(np.int32)
    nmiss = CR.sums(X[rows])["nmiss"]
    assert np.all(nmiss[:32] == 0) and np.any(nmiss[32:64] > 0) and np.all(nmiss[64:] == 0)
    fp = four_product_pairs(nmiss)
    assert not fp[3, 70] and not fp[70, 90] and fp[3, 40] and fp[40, 70]
    got = ld_r2(_ctx(), bed, n_ref, rows)
    worst = check_r2(got, X[rows], "mixed")
    assert set(worst) == {"raw", "four-product"}
    for i, j in ((3, 70), (0, 95), (20, 25), (66, 90)):
        pair = ld_r2(_ctx(), bed, n_ref, rows[[i, j]])
        assert pair[0, 1].tobytes() == got[i, j].tobytes(), (i, j)


@gpu
def test_ld_r2_at_the_n_ref_cap():
    """n_ref = 1 863 936 (9 kpad = 2^24 - 1792), the 40 rows of test_gram_range's cap panel:
    singletons, doubletons, rare variants and near-monomorphic major-allele rows, no missing call.
    n G reaches 1.4e13 and the numerators cancel to a few units; every pair within 4 ulp."""
    from dbslmm_amd import ld_r2
    dos = _cap_dosages()
    got = ld_r2(_ctx(), _bed_of(dos), N_CAP, np.arange(len(dos)))
    check_r2(got, dos, "cap")


@gpu
def test_ld_r2_and_clump_argument_errors():
    from dbslmm_amd import DbslmmError, clump, ld_r2
    bed, _ = _edge_panel(400)
    rows, chrom, bp = np.arange(4), np.ones(4), np.arange(4)
    for call in (lambda: ld_r2(_ctx(), bed, 400, [0, 130]),
                 lambda: ld_r2(_ctx(), bed, 400, [-1]),
                 lambda: ld_r2(_ctx(), bed, N_CAP + 1, [0]),
                 lambda: clump(_ctx(), bed, 400, [0, 1, 2, 130], chrom, bp),
                 lambda: clump(_ctx(), bed, 400, rows, chrom, bp, r2=0.0),
                 lambda: clump(_ctx(), bed, 400, rows, chrom, bp, r2=1.5),
                 lambda: clump(_ctx(), bed, 400, rows, chrom, bp, r2=float("nan")),
                 lambda: clump(_ctx(), bed, 400, rows, chrom, bp, kb=-1)):
        with pytest.raises(DbslmmError) as ei:
            call()
        assert "rc=-1" in str(ei.value), str(ei.value)
    assert len(clump(_ctx(), bed, 400, rows, chrom, bp, r2=1.0, kb=0)) == 4


# ------------------------------------------------------------------------------------------------
# clump decisions
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _td():
    bed = load_bed(REF + ".bed")
    c = CR.summary_candidates(SUMM, REF + ".bim", 1e-6)
    X = CR.decode(bed, 400, c["row"])
    return bed, c, X, CR.pair_integers(X)


@functools.lru_cache(maxsize=None)
def _td_oracle(r2, kb):
    _, c, X, pi = _td()
    return CR.clump_ref(X, c["chrom"], c["bp"], r2, int(kb * 1000), pairs_int=pi)


@gpu
@pytest.mark.parametrize("r2,kb", [(0.2, 1000), (0.1, 1000), (0.2, 50)])
def test_clump_test_dat(r2, kb):
    """test_dat at pth 1e-6 (444 candidates on 300 kb of one chromosome): the 50 kb window is the one
    with a real band."""
    from dbslmm_amd import clump
    bed, c, _, _ = _td()
    ref, margin = _td_oracle(r2, kb)
    assert margin >= MIN_MARGIN, margin
    got = clump(_ctx(), bed, 400, c["row"], c["chrom"], c["bp"], r2=r2, kb=kb)
    print(f"test_dat r2 {r2} kb {kb}: {int((ref == np.arange(len(ref))).sum())} index SNPs, margin {margin:.2e}, "
          f"tile kernel {_ctx().clump_gpu_ms:.3f} ms")
    np.testing.assert_array_equal(got, ref)
    np.testing.assert_array_equal(clump(_ctx(), bed, 400, c["row"], c["chrom"], c["bp"], r2=r2, kb=kb), got)


SYN_N, SYN_WINDOW_KB, SYN_SEED = 300, 150, 3


@functools.lru_cache(maxsize=None)
def synthetic_candidates(seed=SYN_SEED):
    """A multi-chromosome candidate list (tests/test_clump_host.py checks its properties on the CPU):
    chromosome 1 holds 200 candidates 1 kb apart (a 150 kb window: a band five tile columns wide)
    and, 5 Mb on, 50 more (the empty stretch); chromosome 2 repeats the bp of chromosome 1's first 70;
    chromosome 3 holds the chain A - B - C (r2(A, B), r2(B, C) >= 0.2 > r2(A, C)), A, B, C the three
    most significant candidates in that order; the rest in random priority.  Rows in LD runs of 4, 4 %
    of the rows with missing calls.  Returns bed, X (candidates in priority order), rows, chrom, bp."""
    rng = np.random.default_rng(seed)
    n = SYN_N
    chrom = np.concatenate([np.full(250, 1), np.full(70, 2), np.full(3, 3)])
    bp = np.concatenate([1000 * np.arange(200), 5_200_000 + 1000 * np.arange(50), 1000 * np.arange(70),
                         [500, 600, 700]]).astype(np.int64)
    P = _rows(rng, 323, n)
    holes = rng.choice(320, size=13, replace=False)
    P[holes] = np.where(rng.random((13, n)) < 0.03, -1, P[holes])
    a = rng.binomial(2, 0.4, size=n)
    b = np.where(rng.random(n) < 0.62, a, rng.binomial(2, 0.4, size=n))
    c = np.where(rng.random(n) < 0.62, b, rng.binomial(2, 0.4, size=n))
    P[320], P[321], P[322] = a, b, c
    file_row = rng.permutation(323)                      # bed row of position-ordered SNP k
    F = np.zeros_like(P)
    F[file_row] = P
    prio = np.concatenate([[320, 321, 322], rng.permutation(320)])
    rows = file_row[prio].astype(np.int32)
    return CR.encode(F), np.ascontiguousarray(P[prio]), rows, chrom[prio].astype(np.int32), bp[prio]


@functools.lru_cache(maxsize=None)
def synthetic_oracle():
    _, X, _, chrom, bp = synthetic_candidates()
    return CR.clump_ref(X, chrom, bp, 0.2, SYN_WINDOW_KB * 1000)


@gpu
def test_clump_synthetic_multi_chromosome():
    from dbslmm_amd import clump
    bed, X, rows, chrom, bp = synthetic_candidates()
    ref, margin = synthetic_oracle()
    assert margin >= MIN_MARGIN, margin
    got = clump(_ctx(), bed, SYN_N, rows, chrom, bp, r2=0.2, kb=SYN_WINDOW_KB)
    print(f"synthetic: {int((ref == np.arange(len(ref))).sum())} index SNPs of {len(ref)}, margin {margin:.2e}")
    np.testing.assert_array_equal(got, ref)
    assert got[0] == 0 and got[1] == 0 and got[2] == 2          # the chain: C is an index SNP of its own
    np.testing.assert_array_equal(clump(_ctx(), bed, SYN_N, rows, chrom, bp, r2=0.2, kb=SYN_WINDOW_KB), got)
    # the context's cached image serves the same answer
    from dbslmm_amd import Context
    ctx = Context(0)
    ctx.cache_bed(bed)
    np.testing.assert_array_equal(clump(ctx, bed, SYN_N, rows, chrom, bp, r2=0.2, kb=SYN_WINDOW_KB), got)


@gpu
def test_clump_none_and_one_candidate():
    from dbslmm_amd import clump
    bed, _ = _edge_panel(400)
    e = np.zeros(0, dtype=np.int32)
    assert clump(_ctx(), bed, 400, e, e, e).shape == (0,)
    np.testing.assert_array_equal(clump(_ctx(), bed, 400, [5], [1], [100]), [0])
    np.testing.assert_array_equal(clump(_ctx(), bed, 400, [7], [1], [100]), [0])   # a monomorphic row alone


@gpu
def test_clump_degenerate_rows_never_link():
    """rows without variance or observed call (NaN) neither absorb nor are absorbed, on the raw path
    and among rows with missing calls; a repeated row is absorbed by its twin"""
    from dbslmm_amd import clump
    bed, X = _edge_panel(400)
    rows = np.array([7, 39, 40, 70, 71, 66, 0], dtype=np.int32)
    chrom, bp = np.ones(7, dtype=np.int32), np.arange(7, dtype=np.int64)
    ref, margin = CR.clump_ref(X[rows], chrom, bp, 0.2, 1000)
    assert margin >= MIN_MARGIN
    got = clump(_ctx(), bed, 400, rows, chrom, bp, r2=0.2, kb=1)
    np.testing.assert_array_equal(got, ref)
    assert got[0] == 0 and got[3] == 3 and got[4] == 4 and got[2] == 1


# ------------------------------------------------------------------------------------------------
# CLI
# ------------------------------------------------------------------------------------------------
@gpu
def test_cli_summary_equals_split_run(tmp_path):
    """dbslmm --summary ... --pth 1e-6 on test_dat writes byte for byte the effect file of a -s / -l
    run whose inputs are the summary split by the oracle's index SNPs, and <eff>.clumped.txt lists
    those SNPs in priority order."""
    from test_cli import CLI
    _, c, _, _ = _td()
    ref, margin = _td_oracle(0.2, 1000)
    assert margin >= MIN_MARGIN
    index = [k for k in range(len(ref)) if ref[k] == k]
    index_snps = [c["snp"][k] for k in index]
    L = set(index_snps)
    s_path, l_path = str(tmp_path / "s.txt"), str(tmp_path / "l.txt")
    with open(SUMM) as f, open(s_path, "w") as fs, open(l_path, "w") as fl:
        for line in f:
            (fl if line.split("\t")[1] in L else fs).write(line)
    common = ["-r", REF, "-b", BLOCKS_EUR1, "-n", "2400", "-nsnp", "996", "-h", "0.5", "-mafMax", "0.2",
              "--precise-out"]
    a = subprocess.run([CLI, "--summary", SUMM, "--pth", "1e-6", "-eff", str(tmp_path / "a")] + common,
                       capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
    assert a.returncode == 0, a.stderr
    b = subprocess.run([CLI, "-s", s_path, "-l", l_path, "-eff", str(tmp_path / "b")] + common,
                       capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
    assert b.returncode == 0, b.stderr
    assert f"Using 1e-06, {len(index)} SNPs are regarded as fixed effect." in a.stdout, a.stdout
    ea, eb = open(str(tmp_path / "a.txt"), "rb").read(), open(str(tmp_path / "b.txt"), "rb").read()
    assert len(ea) > 0 and ea == eb
    lines = [l.split() for l in open(str(tmp_path / "a.clumped.txt")).read().splitlines()]
    assert lines[0] == ["SNP", "CHR", "BP", "Z", "P", "N_ABSORBED"]
    assert [l[0] for l in lines[1:]] == index_snps
    assert [int(l[5]) for l in lines[1:]] == [int((ref == k).sum()) - 1 for k in index]
    assert [int(l[2]) for l in lines[1:]] == [int(c["bp"][k]) for k in index]
