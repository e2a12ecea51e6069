"""Streamed results of the PCG route (dbslmm_options.stream_out): on a run_multi(out=...) the
kernels write every result to a host-visible mirror as well as the device arrays, and the calling
thread copies finished blocks into the caller's arrays while the GPU still iterates.  The path
must deliver exactly what the download after the run delivers, so every case here asks for
bit-equality of three things: (a) run_multi(out=...) with stream_out = 1, (b) the same call with
stream_out = 0, (c) the device arrays read back afterwards through plan.download() (the last
copy).  The out arrays are pre-filled with a sentinel, so an entry nobody wrote is seen.
Agreement with the oracle is test_pcg.py's subject, not this file's.

Small panels (n_ref = 128: trivial Grams), the PCG route forced (solver = 2), one case per code
path that writes results: a multi-shift block, per-copy sequences with large SNPs, a chip-wide
block, missing calls, a monomorphic block, empty blocks, LMM-only, 1 / 4 copies, the iteration
cap, a second chunk of iterations, reused and fresh out buffers, two plans, repeatability."""
import functools

import numpy as np
import pytest

SENT, SENT_I = -7.25, -99
FACTORS3 = (0.8, 1.0, 1.2)


# ------------------------------------------------------------------ CPU: the host's copy-out table
def test_out_ranges_cover_every_output_index_exactly_once():
    """dbslmm_out_ranges (the table stream_results copies by) on a problem with empty blocks and
    large SNPs: the rows are the non-empty blocks in order, and their ranges tile beta_s and
    beta_l exactly once; every block has its one status entry or is empty."""
    from dbslmm_amd import out_ranges
    ms = np.array([0, 5, 0, 0, 7, 1, 0, 300, 0, 2, 0])
    ml = np.array([0, 2, 0, 0, 0, 1, 0, 3, 0, 0, 0])
    ml[9], ms[9] = 2, 0                       # a block of large SNPs only
    s_ptr = np.concatenate([[0], np.cumsum(ms)]).astype(np.int64)
    l_ptr = np.concatenate([[0], np.cumsum(ml)]).astype(np.int64)
    t = out_ranges(s_ptr, l_ptr)
    assert t[:, 0].tolist() == np.flatnonzero(ms + ml > 0).tolist()
    hit_s, hit_l = np.zeros(s_ptr[-1], dtype=int), np.zeros(l_ptr[-1], dtype=int)
    for b, s0, s1, l0, l1 in t.tolist():
        assert (s0, s1, l0, l1) == (s_ptr[b], s_ptr[b + 1], l_ptr[b], l_ptr[b + 1])
        hit_s[s0:s1] += 1
        hit_l[l0:l1] += 1
    assert np.all(hit_s == 1) and np.all(hit_l == 1)
    # LMM-only (no l_ptr): empty large ranges; no blocks at all: no rows
    t = out_ranges(s_ptr)
    assert t[:, 0].tolist() == np.flatnonzero(ms > 0).tolist() and np.all(t[:, 3] == t[:, 4])
    assert len(out_ranges(np.zeros(1, dtype=np.int64))) == 0
    assert len(out_ranges(np.zeros(4, dtype=np.int64), np.zeros(4, dtype=np.int64))) == 0


def test_out_ranges_reject_offsets_that_are_not_monotone():
    from dbslmm_amd import DbslmmError, out_ranges
    with pytest.raises(DbslmmError):
        out_ranges(np.array([0, 4, 3, 9]))
    with pytest.raises(DbslmmError):
        out_ranges(np.array([0, 4, 4, 9]), np.array([0, 2, 1, 1]))


def test_python_stream_out_zero_switches_the_path_off():
    """The struct's 0 is "default" (on), so the binding passes an explicit stream_out = 0 as -1."""
    from dbslmm_amd import BlockProblem
    kw = dict(bed=np.zeros(8, dtype=np.uint8), n_ref=4, n_obs=10, sigma_s=0.1, s_ptr=[0, 1], s_pos=[0], z_s=[1.0])
    for given, passed in ((None, 0), (1, 1), (0, -1)):
        p = BlockProblem(opts={} if given is None else {"stream_out": given}, **kw)
        assert p.c_struct().opts.contents.stream_out == passed
        assert p.opts.get("stream_out") == given          # (the caller's dict is left alone)


# ------------------------------------------------------------------ GPU
@functools.lru_cache(maxsize=None)
def _panel(total, n_ref, seed):
    from dbslmm_amd import synth
    return synth.simulate(total + 50, n_ref, pop="EUR", chroms=[1, 2], seed=seed, miss_rate=0.0, large_every=0)


def _build(sizes, n_large=None, n_ref=128, seed=5, miss_block=None, mono_block=None, lmm=False, **opts):
    """Blocks of sizes[b] SNPs (0: an empty block), the first n_large[b] of each large; miss_block
    gets one missing call (its products then read the fp64 Sigma: the whole-block kernel hands
    it back), mono_block one zero-variance SNP."""
    from dbslmm_amd import BlockProblem
    sizes = np.asarray(sizes)
    n_large = np.zeros(len(sizes), dtype=int) if n_large is None else np.asarray(n_large)
    total = int(sizes.sum())
    bed = _panel(total, n_ref, seed).bed.copy()
    rng = np.random.default_rng(seed)
    bid = np.repeat(np.arange(len(sizes)), sizes)
    first = np.concatenate([[0], np.cumsum(sizes)])[:-1]
    large = (np.arange(total) - first[bid]) < n_large[bid]
    z = rng.standard_normal(total)
    z[large] = 6.0 * np.sign(z[large])
    nb = (n_ref + 3) // 4
    if miss_block is not None:
        j = int(first[miss_block]) + 3
        bed[3 + j * nb] = (bed[3 + j * nb] & 0xFC) | 0x01      # PLINK code 01: a missing call
    if mono_block is not None:
        j = int(first[mono_block]) + 5
        bed[3 + j * nb: 3 + (j + 1) * nb] = 0xFF               # every call homozygous: zero variance

    def csr(mask):
        idx = np.flatnonzero(mask)
        ptr = np.zeros(len(sizes) + 1, dtype=np.int64)
        np.add.at(ptr, bid[idx] + 1, 1)
        return np.cumsum(ptr), idx.astype(np.int32), z[idx]
    s_ptr, s_pos, z_s = csr(~large)
    kw = {}
    if not lmm:
        l_ptr, l_pos, z_l = csr(large)
        kw = dict(l_ptr=l_ptr, l_pos=l_pos, z_l=z_l)
    # nsnp = 1M, n = 100 000: 1 / (sigma_s n) = 20, as the flagship config
    return BlockProblem(bed=bed, n_ref=n_ref, n_obs=100000, sigma_s=0.5 / 1e6, s_ptr=s_ptr, s_pos=s_pos,
                        z_s=z_s, opts=dict(solver=2, **opts), **kw)


@pytest.fixture(scope="module")
def ctx():
    from dbslmm_amd import Context
    c = Context(0)
    yield c
    c.close()


def _outs(prob, n):
    return (np.full((n, prob.n_s), SENT), np.full((n, prob.n_l), SENT),
            np.full((n, prob.num_block), SENT_I, dtype=np.int32))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _same(x, y):
    """array_equal on the bit patterns (NaN betas of a monomorphic block included)"""
    return all(u.shape == v.shape and np.array_equal(_bits(u), _bits(v)) for u, v in zip(x, y))


def _no_sentinel(o):
    return not np.any(o[0] == SENT) and not np.any(o[1] == SENT) and not np.any(o[2] == SENT_I)


def _plan(ctx, prob, stream):
    from dbslmm_amd import Plan
    prob.opts["stream_out"] = stream
    plan = Plan(ctx, prob)
    prob.opts.pop("stream_out")
    return plan


def _check(ctx, prob, factors=FACTORS3):
    """(a) = (b) = (c) for one run of each path on fresh plans; returns (a)'s arrays."""
    sig = [prob.sigma_s * f for f in factors]
    got = []
    for stream in (1, 0):
        plan = _plan(ctx, prob, stream)
        o = _outs(prob, len(sig))
        plan.run_multi(sig, out=o)
        assert plan.workload()["pcg_route"] == 1
        assert _no_sentinel(o), stream
        dev = plan.download()                                   # (c): the last copy's device arrays
        assert _same([x[-1] for x in o], dev), stream
        plan.close()
        got.append(o)
    assert _same(got[0], got[1])
    return got[0]


def _status_ok(prob, st):
    m = np.diff(prob.s_ptr) + (np.diff(prob.l_ptr) if prob.l_ptr is not None else 0)
    return bool(np.all(np.where(m > 0, st == 0, st == 1)))


@pytest.mark.gpu
def test_multishift_blocks_three_copies(ctx):
    """Blocks without large SNPs at 3 copies: one multi-shift sequence of dbslmm_pcg_block writes
    every copy; sizes that are no multiple of 128 or 256 (and one of a single SNP)."""
    prob = _build([300, 77, 1, 130])
    o = _check(ctx, prob)
    assert _status_ok(prob, o[2]) and np.all(np.isfinite(o[0]))


@pytest.mark.gpu
def test_blocks_with_large_snps_one_sequence_per_copy(ctx):
    """Large SNPs at 3 copies: one whole-block sequence per copy, each writing its copy's beta_s
    range, its beta_l entries and its status."""
    prob = _build([200, 333, 65], [2, 3, 1])
    o = _check(ctx, prob)
    assert prob.n_l == 6 and _status_ok(prob, o[2]) and np.all(np.isfinite(o[1]))


@pytest.mark.gpu
def test_chip_wide_block_next_to_whole_blocks(ctx):
    """1030 slots: past the whole-block limit of 1024, so the chip-wide kernels iterate it and
    dbslmm_pcg_update writes and flags it when it converges, beside the whole blocks."""
    prob = _build([150, 1030, 90], [0, 1, 0])
    o = _check(ctx, prob)
    assert _status_ok(prob, o[2])


@pytest.mark.gpu
def test_block_with_missing_calls_is_handed_back(ctx):
    prob = _build([150, 260, 70], [0, 1, 0], miss_block=1)
    o = _check(ctx, prob)
    assert _status_ok(prob, o[2])


@pytest.mark.gpu
def test_monomorphic_block(ctx):
    from dbslmm_amd import BLOCK_MONOMORPHIC
    prob = _build([150, 260, 70], [1, 0, 0], mono_block=1)
    o = _check(ctx, prob)
    assert np.all(o[2][:, 1] == BLOCK_MONOMORPHIC) and np.all(o[2][:, [0, 2]] == 0)
    sl = slice(prob.s_ptr[1], prob.s_ptr[2])
    assert np.all(np.isnan(o[0][:, sl])) and np.isfinite(o[0]).sum() == 3 * (prob.n_s - 260)


@pytest.mark.gpu
def test_empty_blocks_get_their_status_from_the_host(ctx):
    from dbslmm_amd import BLOCK_EMPTY
    prob = _build([0, 140, 0, 0, 90, 0], [0, 1, 0, 0, 0, 0])
    o = _check(ctx, prob)
    assert np.all(o[2][:, [0, 2, 3, 5]] == BLOCK_EMPTY) and np.all(o[2][:, [1, 4]] == 0)


@pytest.mark.gpu
def test_lmm_only(ctx):
    prob = _build([140, 300], lmm=True)
    o = _check(ctx, prob)
    assert prob.n_l == 0 and o[1].shape == (3, 0) and _status_ok(prob, o[2])


@pytest.mark.gpu
@pytest.mark.parametrize("factors", [(1.0,), (0.5, 0.8, 1.0, 1.3)], ids=["1copy", "4copies"])
def test_one_and_four_copies(ctx, factors):
    prob = _build([200, 333, 1030], [0, 2, 1])
    o = _check(ctx, prob, factors)
    assert _status_ok(prob, o[2])


@pytest.mark.gpu
def test_not_converged_comes_with_its_iterate(ctx):
    """pcg_maxit = 2 at a tolerance no block reaches by then: NOT_CONVERGED from dbslmm_pcg_block
    and, for the chip-wide block at the cap, from dbslmm_pcg_final (no flag: copied after the
    run); the iterate finite and the same through every path."""
    from dbslmm_amd import BLOCK_NOT_CONVERGED
    prob = _build([150, 1030, 333], [0, 1, 2], pcg_maxit=2, pcg_tol=1e-14)
    o = _check(ctx, prob)
    assert np.all(o[2] == BLOCK_NOT_CONVERGED), o[2]
    assert np.all(np.isfinite(o[0])) and np.all(np.isfinite(o[1]))


@pytest.mark.gpu
def test_second_chunk_of_iterations(ctx):
    """The first chunk of a run is as long as the previous run of the plan needed.  A first run at a
    prior shift of 2000 needs few iterations; the same plan at a shift of 2 then needs more than
    that chunk, so the host's loop sees the event complete, has pcg_finish enqueue another chunk
    and polls again (dbslmm_pcg_final runs once per chunk)."""
    prob = _build([150, 1030, 333], [0, 1, 2])
    easy = [prob.sigma_s * f for f in (0.008, 0.01, 0.012)]
    hard = [prob.sigma_s * f for f in (8.0, 10.0, 12.0)]
    got = []
    for stream in (1, 0):
        plan = _plan(ctx, prob, stream)
        o1 = _outs(prob, 3)
        plan.run_multi(easy, out=o1)
        it1 = int(plan.block_iters()[1])                        # the chip-wide block: the chunk is its count
        o2 = _outs(prob, 3)
        plan.run_multi(hard, out=o2)
        it2 = int(plan.block_iters()[1])
        assert it2 > it1 > 0, (it1, it2)                        # more than the first chunk held
        assert _no_sentinel(o1) and _no_sentinel(o2)
        assert np.all(o1[2] == 0) and np.all(o2[2] == 0)
        assert _same([x[-1] for x in o2], plan.download())
        plan.close()
        got.append((o1, o2))
    assert _same(got[0][0], got[1][0]) and _same(got[0][1], got[1][1])


@pytest.mark.gpu
def test_same_and_fresh_out_buffers_and_repeatability(ctx):
    """Three runs into the same out buffers (re-filled with the sentinel before each), then three
    into fresh ones (new pointers): every run delivers the first run's bits, which are those of
    the download path."""
    prob = _build([200, 333, 1030, 0, 77], [0, 2, 1, 0, 0])
    sig = [prob.sigma_s * f for f in FACTORS3]
    ref = _check(ctx, prob)
    plan = _plan(ctx, prob, 1)
    o = _outs(prob, 3)
    keep = []
    for r in range(6):
        if r >= 3:
            keep.append(o)                                      # (kept alive: the next ones are new pages)
            o = _outs(prob, 3)
        else:
            o[0].fill(SENT), o[1].fill(SENT), o[2].fill(SENT_I)
        plan.run_multi(sig, out=o)
        assert _no_sentinel(o) and _same(o, ref), r
    assert _same([x[-1] for x in o], plan.download())
    plan.close()


@pytest.mark.gpu
def test_two_plans_on_one_context_run_alternately(ctx):
    """The mirror, the flags and the run numbers are per plan: two plans of different problems
    taking turns never see each other's results or flags."""
    pa = _build([200, 333, 1030], [0, 2, 1], seed=5)
    pb = _build([90, 300, 128, 257], [1, 0, 0, 0], seed=6)
    ra, rb = _check(ctx, pa), _check(ctx, pb)
    plan_a, plan_b = _plan(ctx, pa, 1), _plan(ctx, pb, 1)
    for _ in range(3):
        for plan, prob, ref in ((plan_a, pa, ra), (plan_b, pb, rb)):
            o = _outs(prob, 3)
            plan.run_multi([prob.sigma_s * f for f in FACTORS3], out=o)
            assert _no_sentinel(o) and _same(o, ref)
    plan_a.close()
    plan_b.close()


@pytest.mark.gpu
def test_plan_run_and_download_after_a_streamed_run(ctx):
    """plan.run() + download() keep the download path and still work on a plan that streamed."""
    prob = _build([200, 333], [0, 2])
    plan = _plan(ctx, prob, 1)
    o = _outs(prob, 1)
    plan.run_multi([prob.sigma_s], out=o)
    plan.run()
    plan.sync()
    assert _same([x[0] for x in o], plan.download())
    plan.close()
