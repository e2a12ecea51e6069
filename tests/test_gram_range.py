"""The Gram at the edges of its value ranges (kernels.hip: dbslmm_bed_repitch -> dbslmm_snp_stats
-> dbslmm_gram_i8 / _big / _huge, pcg.hip's uint16 unpack, plan_create's n_ref bounds and upload.hip's image cache).

Every other Gram test draws A1 frequencies p <= 0.5 (synth.simulate), so dosage 2 is the rare
genotype and no integer Gram entry comes near 2^15, let alone the 4 n_ref <= 65535 the uint16 Gram
of the PCG route may hold; none sits at either side of that threshold, at the n_ref cap of the
raw-form FP4 accumulation (9 kpad < 2^24), below one 16-byte chunk per file row, or passes a second
n_ref to a cached image.  The panels here do: alleles flipped (A1 the major allele), near-monomorphic
major-allele rows, rare variants at n_ref = 1 863 936.  References: the oracle's direct solve, and
exact_reference -- exact integers, then np.longdouble -- where the oracle's own error matters.
Every precondition (top bit set, max T within 2^11 of 2^24, rows polymorphic) is asserted from the
exact integers, never from the library."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle as O
from _common import normwise

gpu = pytest.mark.gpu

CLASSES = ((1, 1), (1, 2 ** 31 - 1), (2 ** 31 - 1, 2 ** 31 - 1))   # (gram_big_min, gram_huge_min)
MAGIC = (0x6C, 0x1B, 0x01)
N_CAP = 1_863_936              # 9 * N_CAP = 2^24 - 1792: the largest n_ref plan_create accepts
KPAD_ALIGN = 256


# ------------------------------------------------------------------------------------------------
# helpers (plain NumPy)
# ------------------------------------------------------------------------------------------------
def _bps(n_ref):
    return (n_ref + 3) // 4


def _bed_rows(bed, n_ref):
    """[n_rows, bps] view of the SNP-major rows of a .bed image"""
    bps = _bps(n_ref)
    n_rows = (bed.size - 3) // bps
    return bed[3:3 + n_rows * bps].reshape(n_rows, bps)


def flip_alleles(bed, n_ref, rows):
    """A copy of `bed` with the alleles of the given rows swapped: PLINK codes 00 <-> 11, 10 and 01
    unchanged, so a dosage g becomes 2 - g and a missing call stays missing.  (The pad bits of a
    row's last byte change too: harmless, test_rawbed_gram.py::test_pad_bits_ignored.)"""
    out = np.array(bed, dtype=np.uint8, copy=True)
    v = _bed_rows(out, n_ref)
    b = v[rows]
    eq = ~(b ^ (b >> 1)) & np.uint8(0x55)
    v[rows] = b ^ (eq | (eq << 1))
    return out


_DOSE_OF_CODE = np.array([2, -1, 1, 0], dtype=np.int8)     # 00 -> 2, 01 -> missing, 10 -> 1, 11 -> 0
_BYTE_DOSE = _DOSE_OF_CODE[(np.arange(256)[:, None] >> (2 * np.arange(4))) & 3]


def unpack_dosages(bed, n_ref, rows):
    """int8 dosages [len(rows), n_ref] of .bed rows (-1 = missing)"""
    v = _bed_rows(bed, n_ref)[np.asarray(rows)]
    return _BYTE_DOSE[v].reshape(len(v), -1)[:, :n_ref]


def exact_gram(dos):
    """Integer Gram G = D D^T and dosage sums S of int8 dosages [m, n] without missing calls, in fp64
    over chunks of 2^18 individuals: every partial sum is an integer below 2^53, so both are exact."""
    assert dos.dtype == np.int8 and dos.min() >= 0 and dos.max() <= 2
    m, n = dos.shape
    G = np.zeros((m, m))
    S = np.zeros(m)
    for k0 in range(0, n, 1 << 18):
        d = dos[:, k0:k0 + (1 << 18)].astype(np.float64)
        G += d @ d.T
        S += d.sum(axis=1)
    assert G.max() < 2.0 ** 53
    return G, S


def _chol_solve(M, b):
    """M^-1 b in M's precision (np.linalg has no longdouble): Cholesky and two substitutions"""
    m = len(b)
    L = np.array(M, copy=True)
    for j in range(m):
        L[j, j] = np.sqrt(L[j, j] - L[j, :j] @ L[j, :j])
        L[j + 1:, j] = (L[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    y = np.array(b, copy=True)
    for j in range(m):
        y[j] = (y[j] - L[j, :j] @ y[:j]) / L[j, j]
    for j in range(m - 1, -1, -1):
        y[j] = (y[j] - L[j + 1:, j] @ y[j + 1:]) / L[j, j]
    return y


def exact_reference(dos, n_small, z, n_obs, sigma_s, tau=0.8):
    """High-precision reference of one block's Gram -> Sigma -> beta: dosages [m, n] (int8, no missing
    call) in the joint order [small | large], z alike.  G and S are exact integers (exact_gram); then
    in np.longdouble  C = G - S_i S_j / n,  s_i = sqrt(C_ii / (n - 1)),
    Sigma = tau / n * C / (s_i s_j) + (1 - tau) I,  and the joint solve of DESIGN 3.3,
    beta = M^-1 [z_s; z_l] / sqrt(n_obs)  with 1 / (sigma_s n_obs) added on the small-SNP diagonal.
    Returns G, S (float64, exact), Sigma (longdouble) and beta (float64)."""
    ld = np.longdouble
    m, n = dos.shape
    G, S = exact_gram(dos)
    Gl, Sl, nl = G.astype(ld), S.astype(ld), ld(n)
    Cm = Gl - np.outer(Sl, Sl) / nl
    s = np.sqrt(np.diag(Cm) / (nl - 1))
    Sigma = ld(tau) / nl * Cm / np.outer(s, s) + (1 - ld(tau)) * np.eye(m, dtype=ld)
    M = Sigma.copy()
    M[np.arange(n_small), np.arange(n_small)] += 1 / (ld(sigma_s) * ld(n_obs))
    beta = _chol_solve(M, np.asarray(z, dtype=ld)) / np.sqrt(ld(n_obs))
    return G, S, Sigma, beta.astype(np.float64)


def _bed_of(dos):
    from dbslmm_amd import synth
    return np.concatenate([np.array(MAGIC, dtype=np.uint8), synth.pack_dosages(dos).ravel()])


def _rows_problem(bed, n_ref, sizes, rows, seed=5, sigma_s=None):
    """BlockProblem with blocks of sizes[b] SNPs reading the bed rows `rows` (in that order), one
    large SNP per block, plus each block's joint order [small | large] as indices into `rows`."""
    from dbslmm_amd import BlockProblem
    rows = np.asarray(rows, dtype=np.int32)
    total = int(sum(sizes))
    assert rows.size == total
    rng = np.random.default_rng(seed)
    bid = np.repeat(np.arange(len(sizes)), sizes)
    large = np.zeros(total, dtype=bool)
    for b in range(len(sizes)):
        large[rng.choice(np.flatnonzero(bid == b), size=1, replace=False)] = True
    z = rng.standard_normal(total)
    z[large] = 6.0 * np.sign(z[large])

    def csr(mask):
        idx = np.flatnonzero(mask)
        ptr = np.zeros(len(sizes) + 1, dtype=np.int64)
        np.add.at(ptr, bid[idx] + 1, 1)
        return np.cumsum(ptr), rows[idx], z[idx]
    s_ptr, s_pos, z_s = csr(~large)
    l_ptr, l_pos, z_l = csr(large)
    prob = BlockProblem(bed=bed, n_ref=n_ref, n_obs=100000, sigma_s=sigma_s or 0.5 / total, s_ptr=s_ptr,
                        s_pos=s_pos, z_s=z_s, l_ptr=l_ptr, l_pos=l_pos, z_l=z_l)
    order = [np.concatenate([np.flatnonzero((bid == b) & ~large), np.flatnonzero((bid == b) & large)])
             for b in range(len(sizes))]
    return prob, order, z


def _oracle(prob, sigma_s=None, blas=True):
    """the oracle's direct solve; blas=False leaves the process-wide BLAS choice of the oracle (and
    with it NumPy's thread count) as it is: the CPU checks must not change it under other tests"""
    if blas:
        O.use_blas(True)
    bs, bl, st, rc = O.est(prob.bed, prob.n_ref, prob.n_obs, sigma_s or prob.sigma_s, prob.s_ptr, prob.s_pos,
                           prob.z_s, prob.l_ptr, prob.l_pos, prob.z_l, tau=prob.tau, method="direct",
                           threads=8)
    assert rc == 0
    return np.concatenate([bs, bl])


def _cat(res):
    return np.concatenate([res[0], res[1]])


def _run(prob, sigmas=None, **opts):
    """One plan run with the given options -> ((beta_s, beta_l, status) per copy, workload, block_iters)"""
    from dbslmm_amd import Context, Plan
    keep = dict(prob.opts)
    prob.opts.update(opts)
    try:
        plan = Plan(Context(0), prob)
        if sigmas is None:
            plan.run()
            plan.sync()
            out = [plan.download()]
        else:
            out = plan.run_multi(sigmas)
        wl, it = plan.workload(), plan.block_iters()
        plan.close()
    finally:
        prob.opts.clear()
        prob.opts.update(keep)
    return out, wl, it


def _classes(prob, **opts):
    """the same run with every block on the 256-tile, the 128-tile and the 32-tile Gram kernel"""
    return [_run(prob, gram_big_min=big, gram_huge_min=huge, **opts) for big, huge in CLASSES]


def _all_equal(outs):
    for other in outs[1:]:
        for x, y in zip(outs[0], other):
            np.testing.assert_array_equal(x, y)


# ------------------------------------------------------------------------------------------------
# panels
# ------------------------------------------------------------------------------------------------
FLIP_SIZES = [70, 130, 400, 600]      # block 0 as simulated; 1 and 3 flipped; a random half of 2
FLIP_HAND = 1                         # the hand-made rows go into this (flipped) block


def _flipped(bed, n_ref, sizes, miss=False):
    """flip_alleles on all rows of blocks 1 and 3 and a random half of block 2; into block FLIP_HAND
    two hand-made rows (panels without missing calls): dosage 2 everywhere except 3 heterozygotes /
    except 50 zeros.  Returns the bed and the flipped rows."""
    rng = np.random.default_rng(17)
    start = np.concatenate([[0], np.cumsum(sizes)])
    half = start[2] + np.sort(rng.choice(sizes[2], size=sizes[2] // 2, replace=False))
    rows = np.concatenate([np.arange(start[1], start[2]), half, np.arange(start[3], start[4])])
    bed = flip_alleles(bed, n_ref, rows)
    if not miss:
        hand = np.full((2, n_ref), 2, dtype=np.int8)
        hand[0, rng.choice(n_ref, size=3, replace=False)] = 1
        hand[1, rng.choice(n_ref, size=50, replace=False)] = 0
        from dbslmm_amd import synth
        _bed_rows(bed, n_ref)[[start[FLIP_HAND] + 7, start[FLIP_HAND] + 90]] = synth.pack_dosages(hand)
    return bed, rows


@functools.lru_cache(maxsize=None)
def _flip_panel(n_ref, miss=0.0, extra=0):
    """The flipped panel at n_ref individuals (+ `extra` more, dosages drawn at random, same rows):
    problem, per-block joint order, z, dosages [1200, n_ref + extra] and the exact per-block (G, S)."""
    from dbslmm_amd import synth
    total = sum(FLIP_SIZES)
    p = synth.simulate(total + 100, n_ref, pop="EUR", chroms=[1, 2], seed=11, miss_rate=miss, large_every=0)
    assert p.m >= total
    bed, flipped = _flipped(p.bed, n_ref, FLIP_SIZES, miss > 0)
    dos = unpack_dosages(bed, n_ref, np.arange(total))
    if extra:
        assert miss == 0.0
        more = np.random.default_rng(23).integers(0, 3, size=(total, extra), dtype=np.int8)
        dos = np.ascontiguousarray(np.concatenate([dos, more], axis=1))
        bed = _bed_of(dos)
    prob, order, z = _rows_problem(bed, n_ref + extra, FLIP_SIZES, np.arange(total))
    exact = None
    if miss == 0.0:
        exact = [exact_gram(np.ascontiguousarray(dos[o])) for o in order]
    return dict(prob=prob, order=order, z=z, dos=dos, exact=exact, flipped=flipped)


def _assert_polymorphic(exact, n):
    """no monomorphic row: the exact centred sum of squares n G_ii - S_i^2 is positive"""
    for G, S in exact:
        assert np.all(n * np.diag(G) - S * S > 0)


def _flip_preconditions(d, n):
    """the inputs sit at the edge: top bit of the uint16 Gram set (and, at 16 383+, the range all
    but used up), every row polymorphic -- from the exact integers"""
    gmax = max(G.max() for G, _ in d["exact"])
    assert gmax >= 32768, gmax
    if n >= 16383:
        assert gmax >= 65000, gmax
    if n <= 16383:
        assert gmax <= 65535
    _assert_polymorphic(d["exact"], n)


@functools.lru_cache(maxsize=None)
def _flip_oracle(n_ref, miss=0.0, extra=0, sigma_s=None):
    return _oracle(_flip_panel(n_ref, miss, extra)["prob"], sigma_s)


CAP_M, CAP_LARGE = 40, (11, 33)       # the cap panel: one block of 40 rows, two large SNPs


@functools.lru_cache(maxsize=None)
def _cap_dosages():
    """The cap panel at N_CAP individuals; the carriers of the hand-made rows lie among the first
    N_CAP - 3, so the panel cut to n_ref = N_CAP - 3 keeps their counts.  Rows: exactly 1, 2, 3, 37 and
    1000 heterozygous carriers; all dosage 2 except one heterozygote / except 50 zeros; 9 rows with
    MAF ~ U(0.001, 0.01), 12 with U(0.05, 0.5), 12 with U(0.9, 0.999)."""
    rng = np.random.default_rng(29)
    n = N_CAP
    dos = np.zeros((CAP_M, n), dtype=np.int8)
    r = 0
    for k in (1, 2, 3, 37, 1000):
        dos[r, rng.choice(n - 3, size=k, replace=False)] = 1
        r += 1
    dos[r] = 2
    dos[r, rng.choice(n - 3, size=1)] = 1
    r += 1
    dos[r] = 2
    dos[r, rng.choice(n - 3, size=50, replace=False)] = 0
    r += 1
    for cnt, lo, hi in ((9, 0.001, 0.01), (12, 0.05, 0.5), (12, 0.9, 0.999)):
        for p in rng.uniform(lo, hi, size=cnt):
            dos[r] = rng.binomial(2, p, size=n)
            r += 1
    assert r == CAP_M
    return dos[rng.permutation(CAP_M)]       # the edge rows spread over the 32 + 8 tiles


@functools.lru_cache(maxsize=None)
def _cap_panel(n_ref):
    """problem, joint order and z of the cap panel's first n_ref individuals"""
    dos = np.ascontiguousarray(_cap_dosages()[:, :n_ref])
    from dbslmm_amd import BlockProblem
    rng = np.random.default_rng(31)
    large = np.zeros(CAP_M, dtype=bool)
    large[list(CAP_LARGE)] = True
    z = rng.standard_normal(CAP_M)
    z[large] = 6.0 * np.sign(z[large])
    si, li = np.flatnonzero(~large), np.flatnonzero(large)
    prob = BlockProblem(bed=_bed_of(dos), n_ref=n_ref, n_obs=100000, sigma_s=0.5 / CAP_M,
                        s_ptr=np.array([0, si.size]), s_pos=si, z_s=z[si], l_ptr=np.array([0, li.size]),
                        l_pos=li, z_l=z[li])
    order = np.concatenate([si, li])
    return dict(prob=prob, order=order, z=z, dos=dos)


@functools.lru_cache(maxsize=None)
def _cap_exact(n_ref):
    """exact_reference of the cap panel, with its preconditions: max T = max(9 kpad - 3 (S_a + S_b)
    + G_ab), the largest value the fp32 MFMA accumulator must hold exactly, within 2^11 of 2^24
    (and below it); every row polymorphic"""
    d = _cap_panel(n_ref)
    o = d["order"]
    G, S, Sigma, beta = exact_reference(np.ascontiguousarray(d["dos"][o]), CAP_M - len(CAP_LARGE), d["z"][o],
                                        d["prob"].n_obs, d["prob"].sigma_s)
    kpad = -(-n_ref // KPAD_ALIGN) * KPAD_ALIGN
    assert kpad == N_CAP
    tmax = (9.0 * kpad - 3.0 * (S[:, None] + S[None, :]) + G).max()
    assert 2 ** 24 - 2 ** 11 <= tmax < 2 ** 24, tmax
    _assert_polymorphic([(G, S)], n_ref)
    return dict(G=G, S=S, Sigma=Sigma, beta=beta, tmax=tmax)


def _short_panel(n_ref, miss):
    """200 polymorphic rows of n_ref < 65 individuals (host-built; a monomorphic row is redrawn)"""
    rng = np.random.default_rng(1000 * n_ref + int(miss * 100))
    dos = np.zeros((200, n_ref), dtype=np.int8)
    for r in range(200):
        while True:
            g = rng.binomial(2, rng.uniform(0.1, 0.9), size=n_ref).astype(np.int8)
            if miss:
                g[rng.random(n_ref) < miss] = -1
            obs = g[g >= 0]
            if obs.size >= 2 and obs.min() != obs.max():
                break
        dos[r] = g
    return dos


# ------------------------------------------------------------------------------------------------
# CPU checks of the helpers
# ------------------------------------------------------------------------------------------------
def test_flip_alleles_decodes_to_two_minus_g():
    """Through the oracle's readSNPIm: a flipped row decodes to 2 - g with the same missing
    positions (their imputed mean becomes 2 - mean); rows not named are untouched."""
    from dbslmm_amd import synth
    n_ref = 203                                           # n_ref % 4 = 3: pad bits in the last byte
    rng = np.random.default_rng(2)
    dos = rng.integers(0, 3, size=(12, n_ref), dtype=np.int8)
    dos[rng.random(dos.shape) < 0.05] = -1
    dos[3] = 2                                            # a row of 00 codes only
    bed = _bed_of(dos)
    np.testing.assert_array_equal(unpack_dosages(bed, n_ref, np.arange(12)), dos)
    rows = [0, 3, 7, 11]
    fl = flip_alleles(bed, n_ref, rows)
    assert fl is not bed and np.array_equal(bed, _bed_of(dos))
    idv = np.ones(n_ref, dtype=np.int32)
    for r in range(12):
        g0, _ = O.read_snp_im(bed, r, idv)
        g1, _ = O.read_snp_im(fl, r, idv)
        if r not in rows:
            np.testing.assert_array_equal(g1, g0)
            continue
        obs = dos[r] >= 0
        np.testing.assert_array_equal(g1[obs], 2.0 - dos[r][obs])
        np.testing.assert_array_equal(unpack_dosages(fl, n_ref, [r])[0] < 0, ~obs)
        np.testing.assert_allclose(g1[~obs], 2.0 - g0[~obs], rtol=0, atol=1e-14)
    np.testing.assert_array_equal(flip_alleles(fl, n_ref, rows)[3:].reshape(12, -1)[:, :-1],
                                  bed[3:].reshape(12, -1)[:, :-1])


def test_exact_gram_is_the_integer_gram():
    rng = np.random.default_rng(4)
    dos = rng.integers(0, 3, size=(9, (1 << 18) + 77), dtype=np.int8)     # two chunks
    G, S = exact_gram(dos)
    d = dos.astype(np.int64)
    np.testing.assert_array_equal(G, d @ d.T)
    np.testing.assert_array_equal(S, d.sum(axis=1))


def test_exact_reference_and_oracle_agree_at_the_cap():
    """The two references against each other on the cap panel (n_ref = 1 863 936, singleton and
    near-monomorphic major-allele rows): the oracle's direct solve of its fp64-standardised columns
    within 1e-10 normwise of exact_reference (measured 1.3e-11), so either may hold the library to
    the project's 1e-10 bar there."""
    ref = _cap_exact(N_CAP)
    d = _cap_panel(N_CAP)
    got = _oracle(d["prob"], blas=False)
    err = normwise(got, ref["beta"])
    print(f"oracle direct vs exact_reference at n_ref {N_CAP}: normwise {err:.3e}, max T {ref['tmax']:.0f}")
    assert err < 1e-10


# ------------------------------------------------------------------------------------------------
# 1. high-frequency alleles on every route
# ------------------------------------------------------------------------------------------------
ROUTES = {"factor": dict(solver=1), "pcg_whole": dict(solver=2), "pcg_chip": dict(solver=2, pcg_whole=-1)}


@functools.lru_cache(maxsize=None)
def _flip_route(n_ref, route):
    return _classes(_flip_panel(n_ref)["prob"], **ROUTES[route])


@gpu
@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("n_ref", [10000, 16383])
def test_flipped_alleles_on_every_route(n_ref, route):
    """Blocks of 70 / 130 / 400 / 600 SNPs, two of them with every allele flipped (A1 frequency
    0.5-0.95, dosage 2 the common genotype: G_ij up to 4 n_ref), one half flipped, one as simulated,
    two near-monomorphic major-allele rows -- on the factorisation, on the whole-block PCG kernel
    and on the chip-wide PCG kernels (both unpack the uint16 Gram, whose top bit is set here), each
    with every block on the 256-, 128- and 32-tile Gram kernel: bit-identical across the Gram
    classes, status 0, within 1e-10 normwise of the oracle's direct solve."""
    d = _flip_panel(n_ref)
    _flip_preconditions(d, n_ref)
    runs = _flip_route(n_ref, route)
    ref = _flip_oracle(n_ref)
    _all_equal([out[0] for out, _, _ in runs])
    for (out,), wl, _ in runs:
        assert wl["pcg_route"] == (0 if route == "factor" else 1)
        assert np.all(out[2] == 0), out[2]
    err = normwise(_cat(runs[0][0][0]), ref)
    print(f"n_ref {n_ref} {route}: normwise {err:.3e}")
    assert err < 1e-10


@gpu
@pytest.mark.parametrize("n_ref", [10000, 16383])
def test_flipped_whole_block_kernel_matches_chip_path(n_ref):
    """dbslmm_pcg_block against the chip-wide kernels on the flipped panel: 1e-11, test_pcg.py's bar"""
    a = _cat(_flip_route(n_ref, "pcg_whole")[0][0][0])
    b = _cat(_flip_route(n_ref, "pcg_chip")[0][0][0])
    err = normwise(a, b)
    print(f"n_ref {n_ref}: whole-block vs chip-wide {err:.3e}")
    assert err < 1e-11


@gpu
@pytest.mark.parametrize("route", list(ROUTES))
def test_flipped_run_multi(route):
    """h2f 0.8 / 1 / 1.2 in one run_multi at n_ref = 16 383 (factorisation: one factorisation per
    sigma; PCG, whole-block and chip-wide: the copies as right-hand sides of one iteration), each
    copy against the oracle."""
    d = _flip_panel(16383)
    _flip_preconditions(d, 16383)
    prob = d["prob"]
    sig = [prob.sigma_s * f for f in (0.8, 1.0, 1.2)]
    out, wl, _ = _run(prob, sig, h2f_mode=1, **ROUTES[route])
    assert wl["pcg_route"] == (0 if route == "factor" else 1)
    for c, s in enumerate(sig):
        assert np.all(out[c][2] == 0)
        err = normwise(_cat(out[c]), _flip_oracle(16383, 0.0, 0, s))
        print(f"run_multi {route} copy {c}: normwise {err:.3e}")
        assert err < 1e-10, c


# ------------------------------------------------------------------------------------------------
# 2. both sides of pcg_g16 = 4 n_ref <= 65535
# ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("extra", [0, 1], ids=["16383-uint16", "16384-fp64"])
def test_uint16_threshold(extra):
    """n_ref = 16 383 (the integer Gram as uint16, entries up to 65 523) and the same rows with one
    more individual (n_ref = 16 384: the fp64 Sigma), auto route with sigma_s = 0.5 / 1e6 so that
    PCG is chosen: 1e-10 against the oracle, and the bytes the run streamed -- every block its
    lower triangle m (m + 1) / 2 times its own iteration count (dbslmm_plan_block_iters) -- are
    those of 2-byte elements below the threshold and of 8-byte elements above it."""
    import dataclasses
    d = _flip_panel(16383, 0.0, extra)
    n = 16383 + extra
    _flip_preconditions(d, n)
    sigma = 0.5 / 1e6
    prob = dataclasses.replace(d["prob"], sigma_s=sigma, opts={})
    assert prob.n_ref == n
    (out,), wl, it = _run(prob)
    assert wl["pcg_route"] == 1 and np.all(it > 0)
    assert np.all(out[2] == 0)
    err = normwise(_cat(out), _flip_oracle(16383, 0.0, extra, sigma))
    print(f"n_ref {n}: normwise {err:.3e}, iterations {it.tolist()}")
    assert err < 1e-10
    m = np.array(FLIP_SIZES, dtype=np.float64)
    elems = float(np.sum(it * m * (m + 1) / 2))
    assert wl["pcg_block_bytes"] + wl["pcg_chip_bytes"] == (8.0 if extra else 2.0) * elems


# ------------------------------------------------------------------------------------------------
# 3. missing calls with flipped alleles
# ------------------------------------------------------------------------------------------------
@gpu
def test_flipped_alleles_with_missing_calls():
    """n_ref = 1021, 1 % missing calls, blocks flipped as above: the 4-product path with imputation
    means mu ~ 2.  Classes bit-identical, 1e-10 against the oracle; read_snp_std and bed_maf on
    flipped rows as test_rawbed_gram.py::test_statistics_match_oracle."""
    from dbslmm_amd import Context, bed_maf, read_snp_std
    n_ref = 1021
    d = _flip_panel(n_ref, 0.01)
    prob, dos = d["prob"], d["dos"]
    for b, o in enumerate(d["order"]):               # every block takes the missing-call form
        assert np.any(dos[o] < 0), b
    obs = dos >= 0
    mu = np.where(obs, dos, 0).sum(axis=1) / obs.sum(axis=1)
    fl = d["flipped"]
    assert np.median(mu[fl]) > 1.3 and mu[fl].max() > 1.85     # A1 frequency U(0.5, 0.95): mean 2 (1 - p)
    for r in range(len(dos)):
        g = dos[r][obs[r]]
        assert g.min() != g.max(), r
    runs = _classes(prob, solver=1)
    _all_equal([out[0] for out, _, _ in runs])
    out = runs[0][0][0]
    assert np.all(out[2] == 0)
    err = normwise(_cat(out), _flip_oracle(n_ref, 0.01))
    print(f"flipped + missing: normwise {err:.3e}")
    assert err < 1e-10
    ctx = Context(0)
    rows = [int(fl[0]), int(fl[1]), int(fl[len(fl) // 2]), int(fl[np.argmax(mu[fl])]), int(fl[-1])]
    X, maf = read_snp_std(ctx, prob.bed, n_ref, rows)
    idv = np.ones(n_ref, dtype=np.int32)
    for j, r in enumerate(rows):
        g, mf = O.read_snp_im(prob.bed, r, idv)
        np.testing.assert_allclose(X[:, j], O.normalize(g), rtol=0, atol=1e-12)
        assert abs(maf[j] - mf) < 1e-14
    n_rows = (prob.bed.size - 3) // _bps(n_ref)
    np.testing.assert_array_equal(bed_maf(ctx, prob.bed, n_ref, n_rows),
                                  O.bed_maf(prob.bed, n_ref, n_rows, threads=4))


# ------------------------------------------------------------------------------------------------
# 4. Sigma itself
# ------------------------------------------------------------------------------------------------
SIGMA_K = 9


@gpu
def test_sigma_elementwise_against_exact_integers():
    """Sigma of the flipped 130-SNP block (with the two near-monomorphic rows) at n_ref = 16 383,
    after a debug_stop = 1 run on each Gram class, element by element against exact_reference.

    Tolerance of element (i, j), from the exact integers only, eps = 2^-52:
        K eps [ tau/n (|G_ij| + S_i S_j / n) / (s_i s_j)
                + |Sigma_ij - (1 - tau) delta_ij| ((G_ii + S_i^2/n) / C_ii + (G_jj + S_j^2/n) / C_jj) ]
    K = 9: the epilogue chain has 18 fp64 roundings, each at most eps / 2 relative -- 1/n, the
    centring fma, c * rsd_i, * rsd_j, tau / n, its product, 1 - tau and its add (8), and for each
    of s_i, s_j: S^2 / n, sq - it, / (n - 1), sqrt, the reciprocal (2 x 5).  The first two act on
    terms of size S_i S_j / n and |C_ij| <= |G_ij| + S_i S_j / n, the others on Sigma_ij itself
    (<= the first term) or, inside an s, on S^2 / n and C_ii: first-order sums are 4.5 eps on the
    first term and 1.75 eps per s, so K = 9 covers them twice over."""
    from dbslmm_amd import Context, Plan
    n = 16383
    d = _flip_panel(n)
    _flip_preconditions(d, n)
    b = FLIP_HAND
    o = d["order"][b]
    prob = d["prob"]
    m = len(o)
    tau = prob.tau
    G, S, Sigma, _ = exact_reference(np.ascontiguousarray(d["dos"][o]), m - 1, d["z"][o], prob.n_obs, prob.sigma_s,
                                     tau)
    assert G.max() >= 65000
    ld = np.longdouble
    Gl, Sl, nl = G.astype(ld), S.astype(ld), ld(n)
    A = np.abs(Gl) + np.outer(Sl, Sl) / nl
    Cd = np.diag(Gl) - Sl * Sl / nl
    s = np.sqrt(Cd / (nl - 1))
    rel_s = np.diag(A) / Cd
    off = np.abs(Sigma - (1 - ld(tau)) * np.eye(m, dtype=ld))
    tol = SIGMA_K * ld(2.0) ** -52 * (ld(tau) / nl * A / np.outer(s, s) + off * (rel_s[:, None] + rel_s[None, :]))
    tril = np.tril_indices(m)
    got = []
    for big, huge in CLASSES:
        prob.opts.update(debug_stop=1, solver=1, gram_big_min=big, gram_huge_min=huge)
        try:
            plan = Plan(Context(0), prob)
            plan.run()
            plan.sync()
            got.append(plan.block_matrix(b)[:m, :m][tril].copy())
            plan.close()
        finally:
            prob.opts.clear()
    np.testing.assert_array_equal(got[1], got[0])
    np.testing.assert_array_equal(got[2], got[0])
    err = np.abs(got[0].astype(ld) - Sigma[tril])
    ratio = (err / tol[tril]).astype(np.float64)
    print(f"Sigma: max |d| {float(err.max()):.3e}, max |d| / tol {ratio.max():.3f}, max tol {float(tol.max()):.3e}")
    assert np.all(err <= tol[tril]), float(ratio.max())


# ------------------------------------------------------------------------------------------------
# 5. the n_ref cap
# ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n_ref", [N_CAP - 3, N_CAP])
def test_n_ref_cap_exact(n_ref):
    """n_ref = 1 863 933 (n_ref % 4 = 1: three padding individuals and pad bits) and 1 863 936, both
    kpad = 1 863 936 = the cap of 9 kpad < 2^24.  One block of 40 SNPs, two large: singletons,
    doubletons, rare and common variants, major-allele rows (dosage 2 except one heterozygote /
    except 50 zeros).  The raw-form sums T = sum (3 - g_a)(3 - g_b) reach 2^24 - 1797 (asserted from
    the integers): one unit lost in the fp32 MFMA accumulation would change G.  All three Gram
    classes (one ragged tile of the 128- and 256-tile kernels, 32 + 8 of the 32-tile kernel)
    bit-identical, status 0, beta within 1e-10 of exact_reference; the same block on the PCG route
    (fp64 Sigma) within 1e-10.

    Measured on the MI355X with the cancelling forms css = sq - S^2/n and C = fma(-S_i S_j, 1/n, G)
    (they lose ~eps 4n absolute where C_ii ~ 1): normwise 2.76e-11 at 1 863 936 and
    3.57e-12 at 1 863 933, on both routes alike (an fp64 emulation of that epilogue on the exact
    integers gives the same figures; max |dSigma| 4.5e-10).  The test passes as the code stands, so
    nothing was changed: no "after" figure (the exact-numerator forms emulate to 1e-15)."""
    ref = _cap_exact(n_ref)
    prob = _cap_panel(n_ref)["prob"]
    runs = _classes(prob, solver=1)
    _all_equal([out[0] for out, _, _ in runs])
    out = runs[0][0][0]
    assert np.all(out[2] == 0)
    err = normwise(_cat(out), ref["beta"])
    (pout,), wl, _ = _run(prob, solver=2)
    assert wl["pcg_route"] == 1 and np.all(pout[2] == 0)
    perr = normwise(_cat(pout), ref["beta"])
    print(f"n_ref {n_ref}: max T {ref['tmax']:.0f}, factorisation {err:.3e}, PCG route {perr:.3e}")
    assert err < 1e-10
    assert perr < 1e-10


@gpu
def test_n_ref_above_cap_is_rejected():
    """n_ref = 1 863 937 (kpad 1 864 192, 9 kpad >= 2^24): plan_create returns the argument error
    and names the bound, before anything is uploaded or launched."""
    from dbslmm_amd import BlockProblem, Context, DbslmmError, Plan
    n_ref = N_CAP + 1
    bed = np.zeros(3 + 4 * _bps(n_ref), dtype=np.uint8)
    bed[:3] = MAGIC
    prob = BlockProblem(bed=bed, n_ref=n_ref, n_obs=100000, sigma_s=0.1, s_ptr=np.array([0, 4]),
                        s_pos=np.arange(4), z_s=np.ones(4))
    with pytest.raises(DbslmmError) as ei:
        Plan(Context(0), prob)
    assert "rc=-1" in str(ei.value) and "1,863,936" in str(ei.value), str(ei.value)


# ------------------------------------------------------------------------------------------------
# 6. rows shorter than one 16-byte chunk
# ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("miss", [0.0, 0.02])
@pytest.mark.parametrize("n_ref", [9, 17, 60, 64])
def test_rows_shorter_than_a_chunk(n_ref, miss):
    """bytes per row 3, 5, 15 (several file rows share one aligned 16-byte chunk of the upload; the
    last row's second load lands in the pad behind it) and 16: 200 polymorphic rows in blocks of 40 /
    100 / 60 that include file row 0 and the last one.  Classes bit-identical and 1e-10 against the
    oracle; read_snp_std and bed_maf against the oracle's."""
    from dbslmm_amd import Context, bed_maf, read_snp_std
    dos = _short_panel(n_ref, miss)
    bed = _bed_of(dos)
    assert _bps(n_ref) == {9: 3, 17: 5, 60: 15, 64: 16}[n_ref] and bed.size == 3 + 200 * _bps(n_ref)
    rows = np.random.default_rng(n_ref).permutation(200)
    prob, order, _ = _rows_problem(bed, n_ref, [40, 100, 60], rows)
    if miss:
        for o in order:
            assert np.any(dos[rows[o]] < 0)
    runs = _classes(prob, solver=1)
    _all_equal([out[0] for out, _, _ in runs])
    out = runs[0][0][0]
    assert np.all(out[2] == 0)
    err = normwise(_cat(out), _oracle(prob))
    print(f"n_ref {n_ref} miss {miss}: normwise {err:.3e}")
    assert err < 1e-10
    ctx = Context(0)
    sel = [0, 1, 2, 198, 199]
    X, maf = read_snp_std(ctx, bed, n_ref, sel)
    idv = np.ones(n_ref, dtype=np.int32)
    for j, r in enumerate(sel):
        g, mf = O.read_snp_im(bed, r, idv)
        np.testing.assert_allclose(X[:, j], O.normalize(g), rtol=0, atol=1e-12)
        assert abs(maf[j] - mf) < 1e-14
    np.testing.assert_array_equal(bed_maf(ctx, bed, n_ref, 200), O.bed_maf(bed, n_ref, 200, threads=1))


# ------------------------------------------------------------------------------------------------
# 7. the image cache across n_ref
# ------------------------------------------------------------------------------------------------
def _random_bed(seed, n_bytes):
    bed = np.random.default_rng(seed).integers(0, 256, size=n_bytes, dtype=np.uint8)
    bed[:3] = MAGIC
    return bed


@gpu
def test_image_cache_across_n_ref():
    """One cached host array read with n_ref = 1001, 1004 (same 251 bytes per row, other pad), 997
    (250 bytes per row, other row count) and 1001 again: every bed_maf equals a fresh, uncached
    context's bit for bit, and a plan created at the first n_ref runs bit-identically after the
    others were passed (it holds its own reference to the image)."""
    from dbslmm_amd import Context, DBSLMMFIT, Plan, bed_maf
    bed = _random_bed(41, 3 + 2000 * 251)
    ctx = Context(0)
    ctx.cache_bed(bed)
    prob, _, _ = _rows_problem(bed, 1001, [40, 100, 60], np.random.default_rng(2).permutation(2000)[:200])
    plan = Plan(ctx, prob)
    plan.run()
    first = plan.download()
    for n_ref in (1001, 1004, 997, 1001):
        n_snp = (bed.size - 3) // _bps(n_ref)
        assert n_snp == {1001: 2000, 1004: 2000, 997: 2008}[n_ref]
        got = bed_maf(ctx, bed, n_ref, n_snp)
        np.testing.assert_array_equal(got, bed_maf(Context(0), bed, n_ref, n_snp))
    plan.run()
    for x, y in zip(first, plan.download()):
        np.testing.assert_array_equal(x, y)
    for x, y in zip(first, DBSLMMFIT(0).est(prob)):
        np.testing.assert_array_equal(x, y)
    plan.close()


@gpu
def test_fd_key_with_another_n_ref_is_refused(tmp_path):
    """An image cached with dbslmm_ctx_cache_bed_fd serves the n_ref of its first use; once the
    verbatim bytes are gone, (key, bed_len) with another n_ref is a state error that names the
    cached n_ref -- the key is not read (here it is a real array of the file's bytes all the same) --
    and the cached n_ref keeps working."""
    import os
    from dbslmm_amd import Context, DbslmmError, bed_maf, read_snp_std
    bed = _random_bed(43, 3 + 2000 * 251)
    path = str(tmp_path / "x.bed")
    bed.tofile(path)
    ctx = Context(0)
    fd = os.open(path, os.O_RDONLY)
    try:
        ctx.check(ctx.lib.dbslmm_ctx_cache_bed_fd(ctx.h, fd, bed.size, bed.ctypes.data_as(C.c_void_p)),
                  "ctx_cache_bed_fd")
    finally:
        os.close(fd)
    plain = bed_maf(Context(0), bed, 1001, 2000)
    np.testing.assert_array_equal(bed_maf(ctx, bed, 1001, 2000), plain)
    for call in (lambda: bed_maf(ctx, bed, 997, 2008), lambda: read_snp_std(ctx, bed, 1004, [0, 1999])):
        with pytest.raises(DbslmmError) as ei:
            call()
        assert "rc=-3" in str(ei.value) and "n_ref = 1001" in str(ei.value), str(ei.value)
    np.testing.assert_array_equal(bed_maf(ctx, bed, 1001, 2000), plain)
    ctx.cache_bed(None)
    np.testing.assert_array_equal(bed_maf(ctx, bed, 997, 2008), bed_maf(Context(0), bed, 997, 2008))
