"""GPU parity of the Gram kernels reading the resident panel image directly (kernels.hip:
dbslmm_bed_repitch -> dbslmm_snp_stats -> dbslmm_gram_i8 / _big / _huge): row geometry of the
verbatim .bed (n_ref % 4, both sides of a 256-individual stage), the three Gram classes with and
without missing calls, the PCG route's uint16 Gram, ragged tile edges, a scattered row gather and
the pad bits of the file rows' last byte.  Every test compares results only."""
import functools

import numpy as np
import pytest

import oracle as O
from _common import normwise
from test_tiled import _oracle

pytestmark = pytest.mark.gpu

N_REFS = [250, 257, 1021, 1024]     # n_ref % 4 = 2, 1, 1, 0; below / above 256 and 1024
CLASSES = ((1, 1), (1, 10 ** 9), (10 ** 9, 10 ** 9))   # (gram_big_min, gram_huge_min)


@functools.lru_cache(maxsize=None)
def _panel(n_ref, miss):
    from dbslmm_amd import synth
    return synth.simulate(6000, n_ref, pop="EUR", chroms=[1], seed=7, miss_rate=miss, large_every=3)


@functools.lru_cache(maxsize=None)
def _panel_oracle(n_ref, miss):
    from dbslmm_amd import synth
    return _oracle(synth.make_problem(_panel(n_ref, miss)))


def _classes(prob, **opts):
    """est() with every block on the 256-tile, the 128-tile and the 32-tile Gram kernel"""
    from dbslmm_amd import DBSLMMFIT
    out = []
    for big, huge in CLASSES:
        prob.opts.update(gram_big_min=big, gram_huge_min=min(huge, 2 ** 31 - 1), **opts)
        out.append(DBSLMMFIT(0).est(prob))
    return out


def _all_equal(out):
    for other in out[1:]:
        for x, y in zip(out[0], other):
            np.testing.assert_array_equal(x, y)


def _rows_problem(n_ref, sizes, rows, seed=5, n_large=1):
    """blocks of sizes[b] SNPs reading the bed rows `rows` (in that order) of a chr1-2 panel"""
    from dbslmm_amd import BlockProblem
    rows = np.asarray(rows, dtype=np.int32)
    total = int(sum(sizes))
    assert rows.size == total
    rng = np.random.default_rng(seed)
    bid = np.repeat(np.arange(len(sizes)), sizes)
    large = np.zeros(total, dtype=bool)
    for b in range(len(sizes)):
        large[rng.choice(np.flatnonzero(bid == b), size=n_large, replace=False)] = True
    z = rng.standard_normal(total)
    z[large] = 6.0 * np.sign(z[large])

    def csr(mask):
        idx = np.flatnonzero(mask)
        ptr = np.zeros(len(sizes) + 1, dtype=np.int64)
        np.add.at(ptr, bid[idx] + 1, 1)
        return np.cumsum(ptr), rows[idx].astype(np.int32), z[idx]
    s_ptr, s_pos, z_s = csr(~large)
    l_ptr, l_pos, z_l = csr(large)
    return dict(n_ref=n_ref, n_obs=100000, sigma_s=0.5 / total, s_ptr=s_ptr, s_pos=s_pos, z_s=z_s,
                l_ptr=l_ptr, l_pos=l_pos, z_l=z_l), BlockProblem


@functools.lru_cache(maxsize=None)
def _wide_panel(n_ref, m_total, miss=0.0):
    from dbslmm_amd import synth
    return synth.simulate(m_total, n_ref, pop="EUR", chroms=[1, 2], seed=11, miss_rate=miss, large_every=0)


@pytest.mark.parametrize("miss", [0.0, 0.01])
@pytest.mark.parametrize("n_ref", N_REFS)
def test_gram_classes_row_geometry(n_ref, miss):
    """Every file row geometry through every Gram kernel: the three classes give the same betas
    and status bit for bit (with missing calls: the 4-product path inside each kernel), and the
    oracle's direct solve to 1e-10."""
    from dbslmm_amd import synth
    prob = synth.make_problem(_panel(n_ref, miss))
    out = _classes(prob)
    _all_equal(out)
    ref, _ = _panel_oracle(n_ref, miss)
    err = normwise(np.concatenate(out[0][:2]), ref)
    print(f"n_ref {n_ref} miss {miss}: normwise {err:.3e}")
    assert err < 1e-10


def test_pcg_route_integer_gram():
    """Forced PCG route (solver = 2): the uint16 integer Gram epilogue of each Gram kernel."""
    from dbslmm_amd import Context, Plan, synth
    prob = synth.make_problem(_panel(257, 0.0))
    ref, _ = _panel_oracle(257, 0.0)
    out = []
    for big, huge in CLASSES:
        prob.opts.update(solver=2, gram_big_min=big, gram_huge_min=min(huge, 2 ** 31 - 1))
        plan = Plan(Context(0), prob)
        plan.run()
        plan.sync()
        out.append(plan.download())
        assert plan.workload()["pcg_route"] == 1
        plan.close()
    for res in out:
        err = normwise(np.concatenate(res[:2]), ref)
        print(f"pcg route: normwise {err:.3e}")
        assert err < 1e-10
        np.testing.assert_array_equal(res[2], out[0][2])


def test_tile_edges():
    """Blocks of m = 383, 385, 512, 513: ragged last tile rows and columns of the 256- and 128-tile
    kernels, whose rows past m read the zero-dosage row (or re-read the last valid row)."""
    sizes = [383, 385, 512, 513]
    total = sum(sizes)
    p = _wide_panel(257, total + 50)
    assert p.m >= total
    d, BlockProblem = _rows_problem(257, sizes, np.arange(total))
    prob = BlockProblem(bed=p.bed, **d)
    out = _classes(prob)
    _all_equal(out)
    ref, _ = _oracle(prob)
    err = normwise(np.concatenate(out[0][:2]), ref)
    print(f"tile edges: normwise {err:.3e}")
    assert err < 1e-10
    assert np.all(out[0][2] == 0)


def test_scattered_gather():
    """Block rows that are neither sorted nor contiguous and include bed row 0 and the last bed row
    (the image's last row, with the zero-dosage row right behind it)."""
    sizes = [130, 400, 70]
    total = sum(sizes)
    p = _wide_panel(257, 1843)
    rng = np.random.default_rng(3)
    rows = rng.permutation(p.m)[:total]
    for want, at in ((0, 17), (p.m - 1, 140)):        # row 0 in block 0, the last row in block 1
        if want in rows:
            rows[np.flatnonzero(rows == want)[0]] = rows[at]
        rows[at] = want
    assert len(set(rows.tolist())) == total and np.any(np.diff(rows) < 0) and np.any(np.diff(rows) > 1)
    assert (p.bed.size - 3) // ((257 + 3) // 4) == p.m
    d, BlockProblem = _rows_problem(257, sizes, rows)
    prob = BlockProblem(bed=p.bed, **d)
    out = _classes(prob)
    _all_equal(out)
    ref, _ = _oracle(prob)
    err = normwise(np.concatenate(out[0][:2]), ref)
    print(f"gather: normwise {err:.3e}")
    assert err < 1e-10


@pytest.mark.parametrize("miss", [0.0, 0.01])
@pytest.mark.parametrize("n_ref", [250, 257])
def test_pad_bits_ignored(n_ref, miss):
    """The unused bits of every row's last byte set to 1 or to random values: betas, status and
    read_snp_std equal, array for array, those of the same file with zero pad bits."""
    from dbslmm_amd import Context, DBSLMMFIT, read_snp_std, synth
    p = _panel(n_ref, miss)
    nb = (n_ref + 3) // 4
    keep = np.uint8((1 << (2 * (n_ref % 4))) - 1)
    pad = np.uint8(~keep & 0xFF)
    rows0 = p.bed[3:].reshape(p.m, nb)
    assert not np.any(rows0[:, -1] & pad)       # pack_dosages leaves them zero
    rng = np.random.default_rng(9)
    variants = [np.full(p.m, pad, dtype=np.uint8), rng.integers(0, 256, size=p.m, dtype=np.uint8) & pad]
    sel = [0, 1, 77, p.m // 2, p.m - 1]
    prob = synth.make_problem(p)
    fit = DBSLMMFIT(0)
    base = fit.est(prob)
    ctx = Context(0)
    base_std = read_snp_std(ctx, p.bed, n_ref, sel)
    for fill in variants:
        bed = p.bed.copy()
        bed[3:].reshape(p.m, nb)[:, -1] |= fill
        prob.bed = bed
        for x, y in zip(base, fit.est(prob)):
            np.testing.assert_array_equal(x, y)
        for x, y in zip(base_std, read_snp_std(ctx, bed, n_ref, sel)):
            np.testing.assert_array_equal(x, y)
    prob.bed = p.bed


def test_statistics_match_oracle():
    """read_snp_std and bed_maf (both read the image) at n_ref = 257 with missing calls: the
    standardised columns to 1e-12, their MAF to 1e-14, the Armadillo-order MAF pass bit for bit."""
    from dbslmm_amd import Context, bed_maf, read_snp_std
    n_ref = 257
    p = _panel(n_ref, 0.01)
    ctx = Context(0)
    rows = [0, 1, 2, 3, 4, 500, 2999, p.m - 2, p.m - 1]
    X, maf = read_snp_std(ctx, p.bed, n_ref, rows)
    idv = np.ones(n_ref, dtype=np.int32)
    for j, r in enumerate(rows):
        g, m = O.read_snp_im(p.bed, r, idv)
        np.testing.assert_allclose(X[:, j], O.normalize(g), rtol=0, atol=1e-12)
        assert abs(maf[j] - m) < 1e-14
    np.testing.assert_array_equal(bed_maf(ctx, p.bed, n_ref, p.m), O.bed_maf(p.bed, n_ref, p.m, threads=4))
