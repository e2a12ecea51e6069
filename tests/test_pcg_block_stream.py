"""dbslmm_pcg_block keeps two quadrant loads in flight across its reductions and iterations (the
first two quadrants of iteration k + 1 are loaded during iteration k) and steps through a wave's
quadrants with a running (qi, qj) pair: every block size at which a wave's share of the quadrants changes, sequences
taken second and third by a workgroup, exits with loads in flight, and the streamed results.

Bounds.  Against the oracle's direct solve: the project's per-block bar, 1e-10 (_common.blockwise).
Against the chip-wide kernels on the same plan (pcg_whole = -1): each path stops a block and copy at
||r|| <= pcg_tol * lambda_min * ||x||, i.e. within pcg_tol of the solution in the relative 2-norm
(DESIGN 3.6), so two paths differ by at most 2 * pcg_tol * ||x||_2 per block and copy; at a
pcg_maxit cap both hold the same iterate up to rounding, far inside that."""
import numpy as np
import pytest

from _common import blockwise, pcg_case
from test_tiled import _oracle

pytestmark = pytest.mark.gpu

# 1 to 136 quadrants: waves with no quadrant (1 .. 64: one quadrant; 65 .. 128: three), with 1, 2, 3
# and 4 (129 .. 257: 6, 10 and 15 quadrants), a diagonal quadrant as a wave's last, sizes that are no
# multiple of 8, the z row alone in a quadrant (64, 128, 192), the largest block the kernel takes
SIZES = (1, 8, 63, 64, 65, 128, 129, 192, 193, 257, 449, 1000, 1024)
FACTORS = {1: (1.0,), 3: (0.8, 1.0, 1.2), 4: (0.5, 0.8, 1.0, 1.3)}
PCG_TOL = 1e-12            # dbslmm_options.pcg_tol's default
NOT_CONVERGED, MONOMORPHIC = 4, 3

_CTX = []
_ORACLE = {}


def _ctx():
    from dbslmm_amd import Context
    if not _CTX:
        _CTX.append(Context(0))
    return _CTX[0]


def _run(prob, sig, out=None, **opts):
    """One plan of prob with opts, one run_multi: results (copies of the arrays), workload, block_iters."""
    from dbslmm_amd import Plan
    saved = dict(prob.opts)
    prob.opts.update(opts)
    try:
        plan = Plan(_ctx(), prob)
        res = plan.run_multi(sig, out=out)
        res = [tuple(np.array(x) for x in r) for r in res]
        wl, it = plan.workload(), plan.block_iters().copy()
        plan.close()
    finally:
        prob.opts.clear()
        prob.opts.update(saved)
    assert wl["pcg_route"] == 1
    return res, wl, it


def _oracle_at(key, prob, sigma):
    """The oracle's direct solve of prob at sigma, computed once per (panel, sigma)."""
    k = (key, float(sigma))
    if k not in _ORACLE:
        base = prob.sigma_s
        prob.sigma_s = sigma
        try:
            _ORACLE[k] = _oracle(prob)[0]
        finally:
            prob.sigma_s = base
    return _ORACLE[k]


def _block(prob, r, b):
    s = r[0][prob.s_ptr[b]:prob.s_ptr[b + 1]]
    if prob.l_ptr is None:
        return s
    return np.concatenate([s, r[1][prob.l_ptr[b]:prob.l_ptr[b + 1]]])


def _within_stopping_bound(prob, a, b, what):
    """per block and copy ||a - b||_2 <= 2 pcg_tol ||b||_2 (the module docstring); NaN where b is"""
    worst = 0.0
    for c in range(len(a)):
        for blk in range(prob.num_block):
            x, y = _block(prob, a[c], blk), _block(prob, b[c], blk)
            if y.size == 0:
                continue
            ok = np.isfinite(y)
            assert np.array_equal(np.isfinite(x), ok), (what, c, blk)
            ny = float(np.linalg.norm(y[ok]))
            d = float(np.linalg.norm(x[ok] - y[ok]))
            if ny == 0.0:
                assert d == 0.0, (what, c, blk)
                continue
            worst = max(worst, d / ny)
    print(f"{what}: worst block and copy, whole-block against chip-wide, {worst:.3e}")
    assert worst <= 2 * PCG_TOL, (what, worst)


def _same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for ra, rb in zip(a, b) for x, y in zip(ra, rb))


@pytest.mark.parametrize("n_large", [0, 1], ids=["multishift", "one_large"])
@pytest.mark.parametrize("copies", [1, 3, 4])
def test_every_size_against_the_oracle_and_the_chip_wide_path(n_large, copies):
    """Every size with 1, 3 and 4 copies: without large SNPs one multi-shift sequence per block,
    with one large SNP a sequence per copy."""
    c = pcg_case(sizes=SIZES, n_large=(n_large,) * len(SIZES), n_ref=509)
    prob = c.prob
    sig = [prob.sigma_s * f for f in FACTORS[copies]]
    whole, _, it = _run(prob, sig)
    chip, _, itc = _run(prob, sig, pcg_whole=-1)
    assert np.all(it > 0) and np.all(it < 60), it
    for k, s in enumerate(sig):
        assert np.all(whole[k][2] == 0) and np.all(chip[k][2] == 0)
        ref = _oracle_at(("sizes", n_large), prob, s)
        err = blockwise(prob, np.concatenate(whole[k][:2]), ref)
        print(f"n_large {n_large}, {copies} copies, copy {k}: worst block vs oracle {err:.3e}")
        assert err <= 1e-10, (k, err)
    _within_stopping_bound(prob, whole, chip, f"n_large {n_large}, {copies} copies")


def _scattered():
    """600 blocks of 65 SNPs with the 13 sizes scattered among them (every other one of those with a
    large SNP): 627 sequences at 3 copies, more than twice the launch's workgroups."""
    sizes, large, special = [], [], []
    for j in range(600):
        if j % 46 == 7 and len(special) < len(SIZES):
            special.append(len(sizes))
            sizes.append(SIZES[len(special) - 1])
            large.append(len(special) % 2)
        sizes.append(65)
        large.append(0)
    assert len(special) == len(SIZES)
    return pcg_case(sizes=sizes, n_large=large, n_ref=128), special


def test_results_do_not_depend_on_which_workgroup_takes_a_sequence_or_when():
    """More sequences than workgroups: a workgroup takes its second and third sequence with the
    previous one's last loads issued and unread.  Every block's betas, statuses and iteration count
    are bit-equal to the block solved in a plan of its own and to the panel with the block order
    reversed; two runs of one plan are bit-equal."""
    from dbslmm_amd.dist import sub_problem
    c, special = _scattered()
    prob = c.prob
    sig = [prob.sigma_s * f for f in FACTORS[3]]
    a, _, it = _run(prob, sig)
    b, _, it2 = _run(prob, sig)
    assert _same(a, b) and np.array_equal(it, it2)
    assert all(np.all(r[2] == 0) for r in a)
    nb = prob.num_block
    order = np.arange(nb)[::-1]
    rev, s_idx, l_idx = sub_problem(prob, order)
    r, _, itr = _run(rev, sig)
    for k in range(len(sig)):
        assert np.array_equal(r[k][0], a[k][0][s_idx]) and np.array_equal(r[k][1], a[k][1][l_idx])
        assert np.array_equal(r[k][2], a[k][2][order])
    assert np.array_equal(itr, it[order])
    for blk in special + [0, 300, nb - 1]:
        one, s_idx, l_idx = sub_problem(prob, np.array([blk]))
        o, _, ito = _run(one, sig)
        for k in range(len(sig)):
            assert np.array_equal(o[k][0], a[k][0][s_idx]), (blk, k)
            assert np.array_equal(o[k][1], a[k][1][l_idx]), (blk, k)
            assert o[k][2][0] == a[k][2][blk]
        assert ito[0] == it[blk], (blk, ito, it[blk])


CAP_SIZES, CAP_LARGE = (65, 193, 1000, 65, 193, 1000), (0, 0, 0, 1, 1, 1)


@pytest.mark.parametrize("maxit", [1, 2, 3])
def test_the_cap_ends_a_sequence_with_loads_in_flight(maxit):
    """pcg_maxit = 1, 2, 3: NOT_CONVERGED with the iterate, equal to the chip-wide path's."""
    c = pcg_case(sizes=CAP_SIZES, n_large=CAP_LARGE, n_ref=256)
    prob = c.prob
    sig = [prob.sigma_s * f for f in FACTORS[3]]
    whole, _, it = _run(prob, sig, pcg_maxit=maxit)
    chip, _, itc = _run(prob, sig, pcg_maxit=maxit, pcg_whole=-1)
    assert np.all(it == maxit), it
    for k in range(len(sig)):
        assert np.all(whole[k][2] == NOT_CONVERGED) and np.all(chip[k][2] == NOT_CONVERGED)
        assert np.all(np.isfinite(whole[k][0])) and np.all(np.isfinite(whole[k][1]))
    _within_stopping_bound(prob, whole, chip, f"pcg_maxit {maxit}")


# list order = tile rows descending, then block order: all five have 8 tile rows
ZERO_SIZES, ZERO_BLOCKS, ZERO_MONO, ZERO_MISS = (1024, 900, 1000, 950, 1010), (0, 4), 1, 3


def _zero_case():
    return pcg_case(sizes=ZERO_SIZES, n_large=(0, 0, 1, 0, 1), n_ref=256, zero_blocks=ZERO_BLOCKS,
                    mono_block=ZERO_MONO, miss_block=ZERO_MISS)


def test_a_sequence_that_stops_at_once_before_and_after_a_long_one():
    """A right-hand side that is exactly zero (stops in its first iteration) directly before and
    directly after a 1000-SNP block, a monomorphic block and one with a missing call (handed to the
    chip-wide kernels) between them in list order."""
    c = _zero_case()
    prob = c.prob
    sig = [prob.sigma_s * f for f in FACTORS[3]]
    whole, _, it = _run(prob, sig)
    chip, _, itc = _run(prob, sig, pcg_whole=-1)
    for k in range(len(sig)):
        assert np.array_equal(whole[k][2], chip[k][2])
        assert list(whole[k][2]) == [0, MONOMORPHIC, 0, 0, 0]
        for blk in ZERO_BLOCKS:
            assert np.all(_block(prob, whole[k], blk) == 0.0), (k, blk)
        assert np.all(np.isnan(_block(prob, whole[k], ZERO_MONO)))
    assert it[0] == 1 and it[4] == 1 and it[2] > 5, it
    _within_stopping_bound(prob, whole, chip, "zero right-hand sides")


@pytest.mark.parametrize("kind", ["sizes", "cap", "zero"])
def test_streamed_results_equal_the_download(kind):
    """run_multi(out=...) with stream_out on and off: the mirror stores of a sequence's end write
    the same bytes as the device arrays the download reads."""
    opts = {}
    if kind == "sizes":
        prob = pcg_case(sizes=SIZES, n_large=tuple(j % 2 for j in range(len(SIZES))), n_ref=128).prob
    elif kind == "cap":
        prob = pcg_case(sizes=CAP_SIZES, n_large=CAP_LARGE, n_ref=128).prob
        opts = dict(pcg_maxit=2)
    else:
        prob = _zero_case().prob
    sig = [prob.sigma_s * f for f in FACTORS[3]]
    outs = []
    for stream in (1, 0):
        o = (np.full((3, prob.n_s), 7.0), np.full((3, prob.n_l), 7.0), np.full((3, prob.num_block), 9, dtype=np.int32))
        res, _, it = _run(prob, sig, out=o, stream_out=stream, **opts)
        outs.append((res, it))
    assert _same(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
