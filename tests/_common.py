"""Shared fixtures / problem builders for the tests (test infrastructure: may use oracle/)."""
from __future__ import annotations

import json
import math
import os

import numpy as np

import ref_numpy as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
TD = os.path.join(GOLD, "test_dat")
BLOCKS_EUR1 = os.path.join(ROOT, "dbslmm_amd", "data", "block_data", "EUR", "chr1.bed")


def load_bed(path) -> np.ndarray:
    return np.fromfile(path, dtype=np.uint8)


# dbslmm_options.cheb_tol default: the normwise bound of the h2f copies the Chebyshev iteration
# solves on the base copy's factor (include/dbslmm_hip.h); direct solves are held to 1e-10
CHEB_TOL = 1e-9


def normwise(a, ref) -> float:
    a = np.asarray(a, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    if ref.size == 0:
        return 0.0
    return float(np.max(np.abs(a - ref)) / np.max(np.abs(ref)))


def csr_from_infos(infos, num_block):
    ptr = np.zeros(num_block + 1, dtype=np.int64)
    for e in infos:
        ptr[e["block"] + 1] += 1
    ptr = np.cumsum(ptr)
    pos = np.array([e["pos"] for e in infos], dtype=np.int32)
    z = np.array([e["z"] for e in infos], dtype=np.float64)
    return ptr, pos, z


def l_snps():
    return [l.strip() for l in open(os.path.join(GOLD, "l_snps.txt")) if l.strip()]


def td_problem(lmm_only=False, nsnp=996, tau=0.8, maf_max=0.2):
    """test_dat run through the reference host pipeline (BatchRun) -> CSR arrays."""
    n_ref = R.get_row(os.path.join(TD, "ref_chr1.fam"))
    bim = R.read_bim(os.path.join(TD, "ref_chr1"), n_ref, abs(maf_max - 1.0) >= 1e-10)
    blocks = R.read_block(BLOCKS_EUR1)
    summ = R.read_summ(os.path.join(TD, "summary_gemma_chr1.assoc.txt"))
    L = l_snps()
    ss = summ if lmm_only else [s for s in summ if s.snp not in L]
    sl = [] if lmm_only else [s for s in summ if s.snp in L]
    info_s = R.add_block(R.match_ref(ss, bim, maf_max)[0], blocks)
    info_l = R.add_block(R.match_ref(sl, bim, maf_max)[0], blocks)
    nb = len(blocks)
    s_ptr, s_pos, z_s = csr_from_infos(info_s, nb)
    d = dict(bed=load_bed(os.path.join(TD, "ref_chr1.bed")), n_ref=n_ref, n_obs=2400,
             sigma_s=0.5 / nsnp, tau=tau, s_ptr=s_ptr, s_pos=s_pos, z_s=z_s,
             info_s=info_s, info_l=info_l, num_block=nb)
    if not lmm_only:
        d["l_ptr"], d["l_pos"], d["z_l"] = csr_from_infos(info_l, nb)
    return d


def synth_small_problem(lmm_only=False):
    d = os.path.join(GOLD, "synth_small")
    meta = json.load(open(os.path.join(d, "meta.json")))
    gold = json.load(open(os.path.join(d, "golden.json")))
    key = "lmm" if lmm_only else "dbslmm"
    g = gold[f"{key}_pcg"]
    blk = np.array(meta["block"])
    z = np.array(meta["z"])
    nb = meta["num_block"]

    def csr(pos):
        pos = np.array(pos, dtype=np.int32)
        ptr = np.zeros(nb + 1, dtype=np.int64)
        np.add.at(ptr, blk[pos] + 1, 1)
        return np.cumsum(ptr), pos, z[pos]

    s_ptr, s_pos, z_s = csr(g["pos_s"])
    out = dict(bed=load_bed(os.path.join(d, "ref.bed")), n_ref=meta["n_ref"], n_obs=meta["n_obs"],
               sigma_s=meta["h2"] / meta["nsnp"], tau=0.8, s_ptr=s_ptr, s_pos=s_pos, z_s=z_s,
               num_block=nb, gold_pcg=gold[f"{key}_pcg"], gold_direct=gold[f"{key}_direct"])
    if not lmm_only:
        out["l_ptr"], out["l_pos"], out["z_l"] = csr(g["pos_l"])
    return out


def eff_lines(info_s, info_l, beta_s, beta_l):
    res = R.EstResult(np.asarray(beta_s), np.asarray(beta_l), info_s, info_l)
    return R.format_eff(res)


def rows_close(a: str, b: str, ulps: int = 1) -> bool:
    """Output rows equal, allowing +-ulps in the 6th significant digit of numeric fields."""
    ta, tb = a.split(), b.split()
    if len(ta) != len(tb) or ta[0] != tb[0] or ta[1] != tb[1] or ta[-1] != tb[-1]:
        return False
    for x, y in zip(ta[2:4], tb[2:4]):
        fx, fy = float(x), float(y)
        if fx == fy:
            continue
        scale = 10 ** (math.floor(math.log10(max(abs(fx), abs(fy)))) - 5)
        if abs(fx - fy) > ulps * scale * 1.0000001:
            return False
    return True


# ----------------------------------------------------------------------------- PCG-route panels
# One block of each kind the PCG route treats differently (pcg.hip): whole-block multi-shift blocks
# without large SNPs (70, 600), a whole-block block with large SNPs (200), chip-wide blocks (more
# than 1024 slots) without and with large SNPs (1030, 1100), an empty block, a block under 64 SNPs.
PCG_SIZES = (70, 600, 200, 1030, 1100, 0, 40)
PCG_LARGE = (0, 0, 2, 0, 3, 0, 0)


class PcgCase:
    """prob (a fresh BlockProblem), the matching test panel (tbed, ind) and the test rows of the
    small / large SNPs (ts_pos, tl_pos; permuted), sizes."""


_PANELS = {}


def _pcg_panels(total, n_ref, n_total, seed):
    from dbslmm_amd import synth
    key = (total, n_ref, n_total, seed)
    if key not in _PANELS:
        p = synth.simulate(total + 50, n_ref, pop="EUR", chroms=[1, 2], seed=seed, miss_rate=0.0, large_every=0)
        t = synth.simulate(total + 50, n_total, pop="EUR", chroms=[1, 2], seed=seed + 100, miss_rate=0.0,
                           large_every=0)
        _PANELS[key] = (p.bed, t.bed)
    return _PANELS[key]


def pcg_case(sizes=PCG_SIZES, n_large=PCG_LARGE, n_ref=128, n_obs=100000, sigma_s=0.5 / 1e6, tau=0.8,
             lmm=False, miss_block=None, mono_block=None, zero_blocks=(), n_total=150, seed=5, **opts):
    """Blocks of sizes[b] SNPs (0: an empty block), the first n_large[b] of each large (z = +-6).
    The defaults give a prior shift 1 / (sigma_s n_obs) = 20, as the flagship configurations: the
    auto rule takes the PCG route with no solver option.  miss_block gets one missing call (its
    products then read the fp64 Sigma and the whole-block kernel hands it back), mono_block one
    zero-variance SNP, zero_blocks a right-hand side that is exactly zero; lmm: the large SNPs
    stay small ones (LMM-only, no l_ptr).  The test panel holds the same SNPs at permuted rows."""
    from dbslmm_amd import BlockProblem
    sizes, n_large = np.asarray(sizes), np.asarray(n_large)
    total = int(sizes.sum())
    ref_bed, test_bed = _pcg_panels(total, n_ref, n_total, seed)
    bed = ref_bed.copy()
    rng = np.random.default_rng(seed)
    bid = np.repeat(np.arange(len(sizes)), sizes)
    first = np.concatenate([[0], np.cumsum(sizes)])[:-1]
    large = (np.arange(total) - first[bid]) < n_large[bid]
    z = rng.standard_normal(total)
    z[large] = 6.0 * np.sign(z[large])
    for b in zero_blocks:
        z[bid == b] = 0.0
    if lmm:
        large[:] = False
    nb = (n_ref + 3) // 4
    if miss_block is not None:
        j = int(first[miss_block]) + 3
        bed[3 + j * nb] = (bed[3 + j * nb] & 0xFC) | 0x01          # PLINK code 01: a missing call
    if mono_block is not None:
        j = int(first[mono_block]) + 5
        bed[3 + j * nb: 3 + (j + 1) * nb] = 0xFF                   # every call homozygous: zero variance

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
    c = PcgCase()
    c.prob = BlockProblem(bed=bed, n_ref=n_ref, n_obs=n_obs, sigma_s=sigma_s, tau=tau, s_ptr=s_ptr, s_pos=s_pos,
                          z_s=z_s, opts=dict(opts), **kw)
    c.sizes = sizes
    # the test panel: SNP r sits at test row perm[r]
    rows = total + 50
    perm = rng.permutation(rows).astype(np.int32)
    tb = (n_total + 3) // 4
    c.tbed = np.zeros(3 + rows * tb, dtype=np.uint8)
    c.tbed[:3] = test_bed[:3]
    c.tbed[3:].reshape(rows, tb)[perm] = test_bed[3:].reshape(rows, tb)
    c.ind = (rng.random(n_total) < 0.75).astype(np.int32)
    c.ts_pos = perm[s_pos]
    c.tl_pos = None if lmm else perm[l_pos]
    return c


def blockwise(prob, got, ref, skip=()):
    """The per-block bar: the worst over the blocks of max |got - ref| / max |ref| on the joint
    vector [beta_s of the block | beta_l of the block]; got / ref are (beta_s, beta_l) pairs or
    their concatenation.  A block whose reference is not finite (the oracle's 0/0 column of a
    monomorphic SNP) or that is listed in skip is left to the caller."""
    def pair(x):
        if isinstance(x, (tuple, list)):
            return np.asarray(x[0]), np.asarray(x[1])
        x = np.asarray(x)
        return x[:prob.n_s], x[prob.n_s:]
    (gs, gl), (rs, rl) = pair(got), pair(ref)
    assert gs.shape == rs.shape == (prob.n_s,) and gl.shape == rl.shape == (prob.n_l,)
    worst = 0.0
    for b in range(prob.num_block):
        s = slice(prob.s_ptr[b], prob.s_ptr[b + 1])
        g, r = gs[s], rs[s]
        if prob.l_ptr is not None:
            l = slice(prob.l_ptr[b], prob.l_ptr[b + 1])
            g, r = np.concatenate([g, gl[l]]), np.concatenate([r, rl[l]])
        if r.size == 0 or b in skip or not np.all(np.isfinite(r)):
            continue
        scale = np.max(np.abs(r))
        if scale == 0.0:
            assert np.all(g == 0.0), b
            continue
        err = float(np.max(np.abs(g - r)) / scale)
        if not np.isfinite(err):                                   # (max() would drop a NaN)
            return float("inf")
        worst = max(worst, err)
    return worst
