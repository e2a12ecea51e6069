"""The PCG route's seams: the uint16 unpack of both products (converted a sub-block row at a time), the cap on
dbslmm_pcg_block's workgroups (dbslmm_options.pcg_block_wgs), dbslmm_pcg_init launched only where
its vectors are read, and the single launch in front of the Gram.

Bounds.  Every solve is held per block to the oracle's direct solve at the project's bar, 1e-10
(_common.blockwise).  Everything else here is bit-equality: the sequences of dbslmm_pcg_block are
taken from a counter, so which workgroup solves one (and how many there are) never changes a
result; a trimmed init writes the same header fields a full one writes; and the front kernel zeroes
what the memsets zeroed."""
import numpy as np
import pytest

from _common import blockwise, pcg_case
from test_gram_range import _bed_rows, flip_alleles, unpack_dosages
from test_tiled import _oracle

pytestmark = pytest.mark.gpu

FACTORS = {1: (1.0,), 3: (0.8, 1.0, 1.2)}
NOT_CONVERGED, MONOMORPHIC = 4, 3

_CTX = []
_CACHE = {}


def _ctx():
    from dbslmm_amd import Context
    if not _CTX:
        _CTX.append(Context(0))
    return _CTX[0]


def _plan(prob, **opts):
    from dbslmm_amd import Plan
    saved = dict(prob.opts)
    prob.opts.update(opts)
    try:
        return Plan(_ctx(), prob)
    finally:
        prob.opts.clear()
        prob.opts.update(saved)


def _once(plan, sig):
    """one run_multi of the plan: (copies of the result arrays, block_iters)"""
    res = [tuple(np.array(x) for x in r) for r in plan.run_multi(sig)]
    assert plan.workload()["pcg_route"] == 1
    return res, plan.block_iters().copy()


def _run(prob, sig, **opts):
    plan = _plan(prob, **opts)
    try:
        return _once(plan, sig)
    finally:
        plan.close()


def _same(a, b):
    return (all(np.array_equal(x, y, equal_nan=True) for ra, rb in zip(a[0], b[0]) for x, y in zip(ra, rb))
            and np.array_equal(a[1], b[1]))


def _oracle_at(key, prob, sigma):
    """The oracle's direct solve of prob at sigma, computed once per (panel, sigma)."""
    k = (key, float(sigma))
    if k not in _CACHE:
        base = prob.sigma_s
        prob.sigma_s = sigma
        try:
            _CACHE[k] = _oracle(prob)[0]
        finally:
            prob.sigma_s = base
    return _CACHE[k]


def _assert_oracle(key, prob, sig, res, what, mono=()):
    for k, s in enumerate(sig):
        ref = _oracle_at(key, prob, s)
        err = blockwise(prob, np.concatenate(res[k][:2]), ref, skip=mono)
        print(f"{what}, copy {k}: worst block vs oracle {err:.3e}")
        assert err <= 1e-10, (what, k, err)


def _block(prob, r, b):
    s = r[0][prob.s_ptr[b]:prob.s_ptr[b + 1]]
    if prob.l_ptr is None:
        return s
    return np.concatenate([s, r[1][prob.l_ptr[b]:prob.l_ptr[b + 1]]])


# ------------------------------------------------------------------------------------------------
# the unpack: both halves of a dword with bit 15 set, on both products
# ------------------------------------------------------------------------------------------------
# a lone diagonal quadrant (7, 64), an off-diagonal quadrant (65, 129), a ragged last dword (7, 65, 129)
UNPACK_SIZES, UNPACK_LARGE, UNPACK_NREF = (7, 64, 65, 129), (0, 1, 0, 1), 16383


def _unpack_panel():
    """Every allele flipped at n_ref = 16 383 (dosage 2 the common genotype), and in the first and
    the last block a row of dosage 2 everywhere but three heterozygotes: G_ii = 65 523."""
    if "unpack" not in _CACHE:
        from dbslmm_amd import synth
        n = UNPACK_NREF
        prob = pcg_case(sizes=UNPACK_SIZES, n_large=UNPACK_LARGE, n_ref=n).prob
        total = int(sum(UNPACK_SIZES))
        bed = flip_alleles(prob.bed, n, np.arange(total))
        hand = np.full((1, n), 2, dtype=np.int8)
        hand[0, np.random.default_rng(3).choice(n, size=3, replace=False)] = 1
        first = np.concatenate([[0], np.cumsum(UNPACK_SIZES)])
        for b in (0, 3):
            _bed_rows(bed, n)[first[b] + 4] = synth.pack_dosages(hand)
        prob.bed = np.ascontiguousarray(bed)
        # the preconditions, from the exact integer Gram of each block in its slot order [small | large]
        gmax, pairs = 0, 0
        for b in range(len(UNPACK_SIZES)):
            rows = np.concatenate([prob.s_pos[prob.s_ptr[b]:prob.s_ptr[b + 1]], prob.l_pos[prob.l_ptr[b]:prob.l_ptr[b + 1]]])
            d = unpack_dosages(prob.bed, n, rows).astype(np.float64)
            assert d.min() >= 0                                   # (no missing call: the uint16 Gram)
            G = np.tril(d @ d.T)
            gmax = max(gmax, int(G.max()))
            m2 = G.shape[0] // 2 * 2
            top = G[:, :m2] >= 32768                              # dwords: columns (2j, 2j + 1)
            pairs += int(np.sum(top[:, 0::2] & top[:, 1::2]))
        assert gmax == 65523 and pairs > 100, (gmax, pairs)
        _CACHE["unpack"] = prob
    return _CACHE["unpack"]


@pytest.mark.parametrize("whole", [0, -1], ids=["whole_block", "chip_wide"])
@pytest.mark.parametrize("copies", [1, 3])
def test_unpack_of_both_halves_with_the_top_bit_set(copies, whole):
    prob = _unpack_panel()
    sig = [prob.sigma_s * f for f in FACTORS[copies]]
    res, it = _run(prob, sig, pcg_whole=whole)
    assert np.all(it > 0) and np.all(it < 100), it
    for k in range(copies):
        assert np.all(res[k][2] == 0), res[k][2]
    _assert_oracle("unpack", prob, sig, res, f"unpack, pcg_whole {whole}, {copies} copies")


# ------------------------------------------------------------------------------------------------
# pcg_block_wgs
# ------------------------------------------------------------------------------------------------
WGS_MONO, WGS_CHIP, WGS_LARGE = 5, 11, 17


def _wgs_panel():
    """40 blocks: one chip-wide (1 025 SNPs), one with large SNPs, one monomorphic, the rest 30 to
    300 SNPs without large ones (multi-shift sequences at three copies)."""
    if "wgs" not in _CACHE:
        sizes = [30 + (37 * j) % 271 for j in range(40)]
        large = [0] * 40
        sizes[WGS_CHIP] = 1025
        sizes[WGS_LARGE], large[WGS_LARGE] = 200, 2
        _CACHE["wgs"] = pcg_case(sizes=sizes, n_large=large, n_ref=128, mono_block=WGS_MONO).prob
    return _CACHE["wgs"]


def _n_cu():
    """compute units of device 0, asked of the HIP runtime the library has loaded"""
    import ctypes
    _ctx()
    path = next(l.split()[-1] for l in open("/proc/self/maps") if "libamdhip64" in l)
    hip = ctypes.CDLL(path)
    v = ctypes.c_int(0)
    assert hip.hipDeviceGetAttribute(ctypes.byref(v), 63, 0) == 0      # hipDeviceAttributeMultiprocessorCount
    assert 0 < v.value <= 4096, v.value
    return v.value


@pytest.mark.parametrize("copies", [1, 3])
def test_any_number_of_block_workgroups_gives_the_same_bits(copies):
    prob = _wgs_panel()
    sig = [prob.sigma_s * f for f in FACTORS[copies]]
    base = _run(prob, sig)
    for k in range(copies):
        st = base[0][k][2]
        assert st[WGS_MONO] == MONOMORPHIC and np.all(np.delete(st, WGS_MONO) == 0), st
        assert np.all(np.isnan(_block(prob, base[0][k], WGS_MONO)))
    _assert_oracle("wgs", prob, sig, base[0], f"pcg_block_wgs default, {copies} copies", mono=(WGS_MONO,))
    n_cu = _n_cu()
    print(f"compute units: {n_cu}")
    for wgs in (1, 2, n_cu, n_cu + 7):
        assert _same(_run(prob, sig, pcg_block_wgs=wgs), base), wgs


# ------------------------------------------------------------------------------------------------
# dbslmm_pcg_init only where its vectors are read, and the one launch in front of the Gram
# ------------------------------------------------------------------------------------------------
# "miss": a fused block with a missing call keeps every later run on the full init (as before);
# "trim": without one, every run after the plan's first launches the trimmed init
SEAM_SIZES, SEAM_LARGE, SEAM_MONO, SEAM_MISS = (70, 200, 1030, 130, 40, 300), (0, 1, 0, 0, 0, 0), 0, 3


def _seam_panel(kind, lmm=False):
    key = ("seam", kind, lmm)
    if key not in _CACHE:
        _CACHE[key] = pcg_case(sizes=SEAM_SIZES, n_large=SEAM_LARGE, n_ref=128, mono_block=SEAM_MONO, lmm=lmm,
                               miss_block=SEAM_MISS if kind == "miss" else None).prob
    return _CACHE[key]


def _assert_mono(prob, res):
    for k, r in enumerate(res):
        assert r[2][SEAM_MONO] == MONOMORPHIC and np.all(np.delete(r[2], SEAM_MONO) == 0), (k, r[2])
        assert np.all(np.isnan(_block(prob, r, SEAM_MONO)))
        assert np.all(np.isfinite(np.delete(np.concatenate(r[:2]), np.arange(prob.s_ptr[SEAM_MONO], prob.s_ptr[SEAM_MONO + 1]))))


@pytest.mark.parametrize("kind", ["miss", "trim"])
@pytest.mark.parametrize("copies", [1, 3])
def test_first_run_later_runs_and_a_fresh_plan_agree(kind, copies):
    prob = _seam_panel(kind)
    sig = [prob.sigma_s * f for f in FACTORS[copies]]
    fresh = _run(prob, sig)
    plan = _plan(prob)
    try:
        runs = [_once(plan, sig) for _ in range(3)]
    finally:
        plan.close()
    for j, r in enumerate(runs):
        assert _same(r, fresh), j
        _assert_mono(prob, r[0])
    assert np.all(np.delete(fresh[1], SEAM_MONO) > 0), fresh[1]
    _assert_oracle(("seam", kind), prob, sig, fresh[0], f"seams {kind}, {copies} copies", mono=(SEAM_MONO,))


@pytest.mark.parametrize("kind", ["miss", "trim"])
def test_three_copies_then_one_then_three(kind):
    prob = _seam_panel(kind)
    sig3, sig1 = [prob.sigma_s * f for f in FACTORS[3]], [prob.sigma_s * 0.9]
    fresh3, fresh1 = _run(prob, sig3), _run(prob, sig1)
    plan = _plan(prob)
    try:
        a = [_once(plan, sig3), _once(plan, sig3)]          # (the second one trimmed)
        b = [_once(plan, sig1), _once(plan, sig1)]
        c = [_once(plan, sig3), _once(plan, sig3)]
    finally:
        plan.close()
    for r in a + c:
        assert _same(r, fresh3)
        _assert_mono(prob, r[0])
    for r in b:
        assert _same(r, fresh1)
        _assert_mono(prob, r[0])


@pytest.mark.parametrize("kind", ["miss", "trim"])
def test_nothing_is_left_of_a_run_that_ended_at_the_cap(kind):
    """pcg_maxit = 2 at the usual shift: NOT_CONVERGED everywhere.  The next run of the same plan at a
    shift of 2e13 (the matrix all but a multiple of the identity: one iteration reaches pcg_tol =
    1e-6) converges inside the cap and is bit-equal to a plan without the cap."""
    prob = _seam_panel(kind, lmm=True)
    sig, easy = [prob.sigma_s * f for f in FACTORS[3]], [prob.sigma_s * 1e-12 * f for f in FACTORS[3]]
    fresh = _run(prob, easy, pcg_tol=1e-6)
    assert np.all(fresh[1] <= 2), fresh[1]
    _assert_mono(prob, fresh[0])
    plan = _plan(prob, pcg_maxit=2, pcg_tol=1e-6)
    try:
        capped = _once(plan, sig)
        for r in capped[0]:
            assert r[2][SEAM_MONO] == MONOMORPHIC and np.all(np.delete(r[2], SEAM_MONO) == NOT_CONVERGED), r[2]
        for _ in range(2):
            assert _same(_once(plan, easy), fresh)
            capped2 = _once(plan, sig)
            assert _same(capped2, capped)
    finally:
        plan.close()


@pytest.mark.parametrize("kind", ["miss", "trim"])
def test_kernel_spans_with_timing_on(kind):
    from dbslmm_amd import KERNEL_NAMES
    prob = _seam_panel(kind)
    sig = [prob.sigma_s * f for f in FACTORS[3]]
    plan = _plan(prob)
    try:
        _once(plan, sig)
        plan.enable_timing(True)
        for _ in range(3):
            _once(plan, sig)
        ms, n = plan.kernel_ms()
    finally:
        plan.close()
    print(dict(zip(KERNEL_NAMES, ms.tolist())), n)
    assert n == 3 and np.all(np.isfinite(ms)) and np.all(ms >= 0.0), (ms, n)
    for name in ("dbslmm_gram", "dbslmm_pcg", "dbslmm_pcg_block"):
        assert ms[KERNEL_NAMES.index(name)] > 0.0, name
    assert ms[KERNEL_NAMES.index("dbslmm_pcg_block")] <= ms[KERNEL_NAMES.index("dbslmm_pcg")]
    for name in ("dbslmm_chol_large", "dbslmm_chol_small", "dbslmm_tchol", "dbslmm_trsv"):
        assert ms[KERNEL_NAMES.index(name)] == 0.0, name
