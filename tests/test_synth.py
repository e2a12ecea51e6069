"""synth_panel (dbslmm_amd/csrc/synth/synth.hip) on the GPU, through dbslmm_synth_bed by ctypes as
synth._gpu_rows calls it, against the NumPy restatement tests/_synth_ref.py.

A case passes when
* the missing codes (01) sit exactly where the restatement puts them: integer hashing and one exact
  float32 comparison of (k + 0.5) / 2^16 with miss_rate, so no tolerance;
* the pad individuals of the last byte are 00, exactly;
* every other call decodes to the restatement's dosage, except for an individual with a haplotype whose
  reference margin |u - t| to the SNP's threshold is at most EPS = 2^-10: its dosage may differ by at
  most the number of its haplotypes in that band.

EPS is derived, not measured.  The kernel uses __logf and __sincosf and may contract rho u + a e into
an fma; the restatement takes log / sin / cos in float64 and rounds every float32 operation.  |e| is
at most sqrt(-2 log 2^-25) = 5.89.  A per-step error d of e reaches u as at most
a d (1 + rho + rho^2 + ...) = a d / (1 - rho), 14 d at rho = 0.99.  The fast intrinsics are float32
approximations over a bounded argument range here (log on (0, 1], sin / cos on [0, 2 pi]), so d should
be of the order of 1e-5 (a few float32 ulps of a value below 6); 2^-10 = 9.8e-4 leaves about two
decades above that and sits far below anything the model's statistics can see (at most 1e-3 of a
case's haplotypes lie in the band at all: tests/test_synth_host.py asserts that for every case, from
the restatement alone).  A mismatch outside
the band is a finding to trace in the code; EPS changes only with a derivation from documented
intrinsic error bounds, never from what the kernel returned.

Each case prints its mismatch count and the largest reference margin among its mismatches; DESIGN.md
section 5 records them."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import _synth_ref as SR
from _common import ROOT

gpu = pytest.mark.gpu
FILL = 0xA5                     # what the callers' buffers hold before a call


@functools.lru_cache(maxsize=None)
def _lib():
    L = C.CDLL(os.path.join(ROOT, "dbslmm_amd", "libdbslmm_synth.so"))
    L.dbslmm_synth_bed.argtypes = [C.c_int, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                                   C.c_uint64, C.c_float, C.c_float, C.c_void_p]
    L.dbslmm_synth_bed.restype = C.c_int
    L.dbslmm_synth_last_error.restype = C.c_char_p
    return L


def synth_bed(blk, thr, n_ref, seed, rho, miss, num_block=None, rows=None, null=()):
    """dbslmm_synth_bed into rows [blk[-1], nb] prefilled with FILL; returns (rc, rows).  null names
    the pointer arguments to pass as NULL."""
    L = _lib()
    ptr = np.ascontiguousarray(blk, dtype=np.int64)
    thr = np.ascontiguousarray(thr, dtype=np.float32)
    nb = (max(n_ref, 1) + 3) // 4
    if rows is None:
        rows = np.full((max(int(ptr.max()), 1), nb), FILL, dtype=np.uint8)
    arg = dict(blk=ptr.ctypes.data, thr=thr.ctypes.data, rows=rows.ctypes.data)
    for k in null:
        arg[k] = None
    rc = L.dbslmm_synth_bed(0, len(ptr) - 1 if num_block is None else num_block, arg["blk"], arg["thr"],
                            n_ref, seed, rho, miss, arg["rows"])
    return rc, rows


_GOT = {}


def case_rows(name):
    """the GPU's rows of a case of _synth_ref.CASES (whole image, rows below the first block
    included), generated once"""
    if name not in _GOT:
        c = SR.CASES[name]
        rc, rows = synth_bed(c["blk"], SR.case_thr(name), c["n_ref"], c["seed"], c["rho"], c["miss"])
        assert rc == 0, _lib().dbslmm_synth_last_error()
        rows.setflags(write=False)
        _GOT[name] = rows
    return _GOT[name]


def check(name, rows, ref):
    errors, n_bad, worst = SR.compare(rows, ref)
    print(f"synth {name}: {ref.u.shape[0]} SNPs x {ref.n_ref}: {n_bad} calls differ in the band, "
          f"largest margin {worst:.3e} (EPS {SR.EPS:.3e}); band share {SR.band_share(ref):.2e}")
    assert not errors, (name, errors)


@gpu
@pytest.mark.parametrize("name", list(SR.CASES))
def test_panel_is_the_restatement(name):
    """every shape, rho, missing rate, seed, the large SNP index and the three splits: missing codes
    and pads exact, dosages equal outside the band; rows below the first block stay the caller's"""
    c, ref, rows = SR.CASES[name], SR.case_ref(name), case_rows(name)
    first = c["blk"][0]
    assert rows.shape == (c["blk"][-1], ref.nb)
    assert np.all(rows[:first] == FILL)
    check(name, rows[first:], ref)
    if c["miss"] == 1.0:
        code = SR.decode(rows[first:], c["n_ref"])
        assert np.all(code[:, ref.real] == 1)                 # every call missing
    if c["miss"] == 0.0:
        assert not np.any(SR.decode(rows[first:], c["n_ref"]) == 1)


@gpu
def test_seeds_give_different_panels():
    """0, 1, 2^63 and 2^64 - 1 on one shape: no two panels share a row (64-bit seeds are not cut)"""
    got = [case_rows(n) for n in SR.SEED_CASES]
    for i in range(len(got)):
        for j in range(i):
            same = np.all(got[i] == got[j], axis=1)
            assert not np.any(same), (SR.SEED_CASES[i], SR.SEED_CASES[j], np.flatnonzero(same)[:5])


@gpu
def test_split_invariance():
    """byte for byte: a block boundary at SNP 100 leaves rows 0..99 alone and restarts the latent
    after it; the blocks from 100 on alone give the same rows 100..299; a repeated call is identical"""
    whole, split, tail = case_rows("whole"), case_rows("split"), case_rows("tail")
    assert np.array_equal(whole[:100], split[:100])
    # the restart: SNP 100 draws u = e in place of rho u + a e, and the difference decays as rho^k
    differ = np.any(whole[100:] != split[100:], axis=1)
    assert differ[0] and np.count_nonzero(differ[:20]) >= 15
    assert np.array_equal(tail[100:], split[100:])
    assert np.all(tail[:100] == FILL)
    c = SR.CASES["split"]
    rc, again = synth_bed(c["blk"], SR.case_thr("split"), c["n_ref"], c["seed"], c["rho"], c["miss"])
    assert rc == 0 and np.array_equal(again, split)


BAD = {
    "num_block 0": dict(num_block=0),
    "null blk_ptr": dict(null=("blk",)),
    "null thr": dict(null=("thr",)),
    "null rows": dict(null=("rows",)),
    "n_ref 0": dict(n_ref=0),
    "rho 1": dict(rho=1.0),
    "rho below 0": dict(rho=-0.1),
    "rho NaN": dict(rho=float("nan")),
    "falling blk_ptr": dict(blk=(0, 30, 20)),
    "falling to the end": dict(blk=(0, 30, 40, 10)),
    "start below 0": dict(blk=(-5, 10, 40)),
}


@gpu
@pytest.mark.parametrize("what", list(BAD))
def test_bad_arguments_return_minus_one(what):
    """-1 with a message, rows untouched (every one of these is refused before anything is launched)"""
    kw = dict(blk=(0, 10, 40), thr=np.zeros(40, np.float32), n_ref=9, seed=1, rho=0.9, miss=0.01)
    kw.update(BAD[what])
    rows = np.full((40, 3), FILL, dtype=np.uint8)
    rc, rows = synth_bed(rows=rows, **kw)
    assert rc == -1
    assert _lib().dbslmm_synth_last_error()
    assert np.all(rows == FILL)


@gpu
@pytest.mark.parametrize("blk", [(0, 0, 0), (7, 7, 7), (7, 7)])
def test_all_blocks_empty_writes_nothing(blk):
    """returns 0; no row is written, the rows below the (empty) blocks included"""
    rows = np.full((8, 3), FILL, dtype=np.uint8)
    rc, rows = synth_bed(blk, np.zeros(8, np.float32), 9, 1, 0.9, 0.01, rows=rows)
    assert rc == 0
    assert np.all(rows == FILL)


@gpu
def test_simulate_gpu_engine():
    """synth.simulate(engine="gpu"): the .bed is the magic and the restatement's panel for the
    thresholds ndtri(af).astype(float32) under the same band rule; everything but the genotypes
    equals engine="none" exactly; an unknown engine raises"""
    from dbslmm_amd import synth
    none, ptr, thr, ref = SR.sim_case()
    assert len(ptr) - 1 >= 3 and none.m >= 300
    p = synth.simulate(engine="gpu", **SR.SIM)
    assert p.bed.dtype == np.uint8 and p.bed.shape == none.bed.shape == (3 + none.m * ref.nb,)
    assert bytes(p.bed[:3]) == synth.BED_MAGIC
    check("simulate", p.bed[3:].reshape(none.m, ref.nb), ref)
    assert p.blocks == none.blocks and p.n_ref == none.n_ref
    for f in ("chrom", "ps", "block", "af", "z", "large"):
        assert np.array_equal(getattr(p, f), getattr(none, f)), f
    assert not np.any(none.bed[3:])
    with pytest.raises(ValueError):
        synth.simulate(engine="cuda", **SR.SIM)
