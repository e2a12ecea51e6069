"""A plain NumPy restatement of the GPU panel generator (dbslmm_amd/csrc/synth/synth.hip), written from
the model of dbslmm_amd/synth.py and the counter-hash scheme in the kernel's header comment:

* byte column g of SNP s draws from base = mix64(mix64(seed) ^ (s << 22) ^ g), in uint64;
* individual j of the byte (j = 0..3) takes its two haplotype innovations from one Box-Muller pair of
  mix64(base + j * 0xD1B54A32D192ED03): u1 from the hash's top 24 bits, u2 from bits 8..31, each
  (k + 0.5) / 2^24 in float32; e = sqrt(-2 log u1) (cos, sin)(2 pi u2);
* the latent value restarts at the first SNP of a block (u = e) and follows u = rho u + a e after it,
  a = sqrt(1 - rho^2); a haplotype carries the allele when u < thr[s]; dosage = h1 + h2;
* the missing calls of the byte come from mix64(base ^ 0x5851F42D4C957F2D): 16 bits per individual,
  (k + 0.5) / 2^16 < miss_rate, no hash at all when miss_rate is 0;
* PLINK codes, low bits first: dosage 2 -> 00, 1 -> 10, 0 -> 11, missing -> 01, pad individuals 00.

Arithmetic: the hash in uint64; the uniforms, the Box-Muller products and the AR(1) update in float32,
one rounding per operation (no fma); log, sin and cos in float64, rounded to float32.  The kernel's
__logf / __sincosf and a contracted fma differ from this by a few float32 ulps of u, which is why the
comparison of tests/test_synth.py has the band EPS around a SNP's threshold and nothing else."""
from __future__ import annotations

import numpy as np

F32 = np.float32
U64 = np.uint64
K_STRIDE = 0xD1B54A32D192ED03
MISS_XOR = 0x5851F42D4C957F2D
TWO_PI = F32(6.28318530718)
EPS = 2.0 ** -10            # band around the threshold inside which a haplotype may flip (test_synth.py)
BAND_MAX = 1e-3             # at most this share of a case's haplotypes may lie in the band


def mix64(z):
    """SplitMix64's output function of state z (the increment included), elementwise in uint64"""
    z = np.asarray(z, dtype=U64)
    with np.errstate(over="ignore"):
        z = z + U64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
    return z ^ (z >> U64(31))


def uniforms(h):
    """the two 24-bit uniforms of a hash, (k + 0.5) / 2^24 in float32 (k + 0.5 rounds to even from
    k = 2^23 on, so the top value is exactly 1)"""
    h = np.asarray(h, dtype=U64)
    k1 = (h >> U64(40)).astype(F32)
    k2 = ((h >> U64(8)) & U64(0xFFFFFF)).astype(F32)
    s = F32(1.0 / 16777216.0)
    return (k1 + F32(0.5)) * s, (k2 + F32(0.5)) * s


def normal2(h):
    """two N(0, 1) values of one hash: float32 Box-Muller with float64 log / sin / cos"""
    u1, u2 = uniforms(h)
    r = np.sqrt(F32(-2.0) * np.log(u1.astype(np.float64)).astype(F32))
    ang = (TWO_PI * u2).astype(np.float64)
    return r * np.cos(ang).astype(F32), r * np.sin(ang).astype(F32)


def decode(rows, n_ref):
    """packed rows [m, nb] -> PLINK codes [m, 4 nb] (pad individuals included)"""
    rows = np.asarray(rows, dtype=np.uint8)
    sh = np.arange(4, dtype=np.uint8) * 2
    return ((rows[:, :, None] >> sh) & 3).reshape(rows.shape[0], -1)


DOSAGE_OF_CODE = np.array([2, -1, 1, 0], dtype=np.int8)        # 00 -> 2, 01 -> missing, 10 -> 1, 11 -> 0
CODE_OF_DOSAGE = np.array([3, 2, 0], dtype=np.uint8)


class RefPanel:
    """first: the first SNP generated (blk_ptr[0]); everything below is indexed from it.
    rows [m, nb] uint8; u [m, 4 nb, 2] float32 latent values (pad individuals included, they are
    generated and dropped); margin [m, 4 nb, 2] float64 |u - thr|; hap [m, 4 nb, 2] bool; dosage
    [m, 4 nb] int8 before the missing mask; miss [m, 4 nb] bool; real [4 nb] bool (not a pad)."""


def panel(blk_ptr, thr, n_ref, seed, rho, miss_rate) -> RefPanel:
    blk_ptr = [int(x) for x in blk_ptr]
    first, last = blk_ptr[0], blk_ptr[-1]
    m, nb = last - first, (n_ref + 3) // 4
    thr = np.asarray(thr, dtype=F32)
    rho, miss_rate = F32(rho), F32(miss_rate)
    a = np.sqrt(F32(1.0) - rho * rho)
    key = mix64(U64(seed))
    g = np.arange(nb, dtype=U64)
    kk = np.arange(4, dtype=U64) * U64(K_STRIDE)
    u = np.zeros((m, nb * 4, 2), dtype=F32)
    miss = np.zeros((m, nb * 4), dtype=bool)
    sh = np.arange(4, dtype=U64) * U64(16)
    for s0, s1 in zip(blk_ptr[:-1], blk_ptr[1:]):
        assert s0 <= s1
        cur = None
        for s in range(s0, s1):
            base = mix64(key ^ (U64(s) << U64(22)) ^ g)                       # [nb]
            with np.errstate(over="ignore"):
                h = mix64(base[:, None] + kk[None, :])                         # [nb, 4]
            e0, e1 = normal2(h)
            e = np.stack([e0, e1], axis=-1).reshape(nb * 4, 2)
            cur = e if s == s0 else rho * cur + a * e
            assert cur.dtype == F32
            u[s - first] = cur
            if miss_rate > 0:
                mh = mix64(base ^ U64(MISS_XOR))
                k = ((mh[:, None] >> sh[None, :]) & U64(0xFFFF)).astype(F32)
                miss[s - first] = (((k + F32(0.5)) * F32(1.0 / 65536.0)) < miss_rate).reshape(-1)
    p = RefPanel()
    p.first, p.n_ref, p.nb = first, n_ref, nb
    p.u = u
    t = thr[first:last, None, None]
    p.hap = u < t
    p.margin = np.abs(u.astype(np.float64) - t.astype(np.float64))
    p.dosage = p.hap.sum(axis=2).astype(np.int8)
    p.real = np.arange(nb * 4) < n_ref
    p.miss = miss & p.real[None, :]
    code = CODE_OF_DOSAGE[p.dosage]
    code[p.miss] = 1
    code[:, ~p.real] = 0
    c4 = code.reshape(m, nb, 4)
    p.rows = (c4[:, :, 0] | (c4[:, :, 1] << 2) | (c4[:, :, 2] << 4) | (c4[:, :, 3] << 6)).astype(np.uint8)
    return p


def band_share(p: RefPanel, eps=EPS) -> float:
    """share of the real individuals' haplotypes within eps of their SNP's threshold"""
    mg = p.margin[:, p.real, :]
    return float(np.count_nonzero(mg <= eps)) / max(1, mg.size)


def compare(rows, p: RefPanel, eps=EPS):
    """The rule of tests/test_synth.py for rows [m, nb] generated for the SNPs of p.  Returns
    (errors, mismatches, worst margin): errors lists what the rule forbids; mismatches counts the
    calls that differ from the restatement inside the band, and worst margin is the largest band a
    mismatch needed (for a dosage off by d, the d-th smallest margin of the individual's two
    haplotypes)."""
    code = decode(rows, p.n_ref)
    errors = []
    if np.any(code[:, ~p.real] != 0):
        errors.append(f"{np.count_nonzero(code[:, ~p.real])} pad codes are not 00")
    got_miss = (code == 1) & p.real[None, :]
    if np.any(got_miss != p.miss):
        errors.append(f"{np.count_nonzero(got_miss != p.miss)} missing codes differ from the restatement")
    live = p.real[None, :] & ~p.miss & ~got_miss
    diff = np.abs(DOSAGE_OF_CODE[code].astype(np.int16) - p.dosage)
    bad = live & (diff > 0)
    mg = np.sort(p.margin, axis=2)
    need = np.where(diff == 2, mg[:, :, 1], mg[:, :, 0])
    out = bad & (need > eps)
    if np.any(out):
        s, i = np.argwhere(out)[0]
        errors.append(f"{np.count_nonzero(out)} calls differ outside the band, first SNP {p.first + s} "
                      f"individual {i}: margin {need[s, i]:.3e}")
    n_bad = int(np.count_nonzero(bad))
    return errors, n_bad, float(need[bad].max()) if n_bad else 0.0


# ------------------------------------------------------------------------------------------------
# the GPU cases of tests/test_synth.py (tests/test_synth_host.py asserts the band condition of each)
# ------------------------------------------------------------------------------------------------
BLK = (0, 1, 1, 38, 40, 300)        # a one-SNP block, an empty block, five grid.y rows
BLK_THIN = (0, 1, 1, 38, 40, 120)   # the same at n_ref >= 1023 (nb 256: one workgroup column, 257 / 258: two)
BIG_M = 1_000_000
SIM = dict(m_total=400, n_ref=1029, block_limit=4, seed=3, rho=0.9, miss_rate=0.01)


def _cases():
    c = {}
    for n in (1, 3, 4, 5, 1023, 1024, 1025, 1029):
        c[f"n{n}"] = dict(blk=BLK if n < 1023 else BLK_THIN, n_ref=n, seed=1, rho=0.9, miss=0.01)
    for rho in (0.0, 0.5, 0.99):                            # 0.9: the cases above
        c[f"rho{rho}"] = dict(blk=BLK_THIN, n_ref=1029, seed=1, rho=rho, miss=0.01)
    for miss in (0.0, 0.5, 1.0):                            # 0.01: the cases above
        c[f"miss{miss}"] = dict(blk=BLK_THIN, n_ref=1029, seed=1, rho=0.9, miss=miss)
    for name, seed in (("seed0", 0), ("seed2p63", 2 ** 63), ("seedmax", 2 ** 64 - 1)):   # 1: above
        c[name] = dict(blk=BLK_THIN, n_ref=1029, seed=seed, rho=0.9, miss=0.01)
    # s << 22 and s * nb at the scale configurations' indices; 80 calls, so a missing rate that leaves
    # some twenty codes for the missing hash to place
    c["big"] = dict(blk=(BIG_M - 10, BIG_M), n_ref=8, seed=1, rho=0.9, miss=0.25)
    c["whole"] = dict(blk=(0, 300), n_ref=1029, seed=1, rho=0.9, miss=0.01)
    c["split"] = dict(blk=(0, 100, 300), n_ref=1029, seed=1, rho=0.9, miss=0.01)
    c["tail"] = dict(blk=(100, 300), n_ref=1029, seed=1, rho=0.9, miss=0.01)
    return c


CASES = _cases()
SEED_CASES = ("seed0", "n1029", "seed2p63", "seedmax")      # one shape, four seeds
_CACHE = {}


def case_thr(name):
    """thresholds Phi^-1(af), af ~ U(0.05, 0.5) as synth.simulate draws them, from a fixed generator;
    one value per SNP index up to the case's last block"""
    from scipy.special import ndtri
    n = CASES[name]["blk"][-1]
    key = ("thr", n)
    if key not in _CACHE:
        _CACHE[key] = ndtri(np.random.default_rng(0).uniform(0.05, 0.5, size=n)).astype(F32)
        _CACHE[key].setflags(write=False)
    return _CACHE[key]


def case_ref(name) -> RefPanel:
    """the restatement's panel of a case, computed once per process"""
    if name not in _CACHE:
        c = CASES[name]
        _CACHE[name] = panel(c["blk"], case_thr(name), c["n_ref"], c["seed"], c["rho"], c["miss"])
    return _CACHE[name]


def sim_case():
    """the synth.simulate(engine="gpu") case: (engine="none" panel, blk_ptr as simulate forms it,
    thresholds, the restatement's panel)"""
    if "sim" not in _CACHE:
        from scipy.special import ndtri
        from dbslmm_amd import synth
        none = synth.simulate(engine="none", **SIM)
        bounds = np.flatnonzero(np.diff(none.block)) + 1
        ptr = np.concatenate([[0], bounds, [none.m]]).astype(np.int64)
        thr = ndtri(none.af).astype(F32)
        _CACHE["sim"] = (none, ptr, thr,
                         panel(ptr, thr, SIM["n_ref"], SIM["seed"], SIM["rho"], SIM["miss_rate"]))
    return _CACHE["sim"]
