"""gpu_ms of dbslmm_r2_tiles (mask mode, dbslmm_clump) on test_dat and on a config-3-size synthetic
panel with ~5 % of its rows as candidates, next to dbslmm_gram_i8 on plans with a comparable tile
count in the same session (profiles/r13).

    python tools/clump_probe.py [OUT.json]     # one JSON line per case on stdout
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import _clump_ref as CR                                     # noqa: E402
from dbslmm_amd import BlockProblem, Context, Plan, clump, synth   # noqa: E402
from dbslmm_amd._lib import K_GRAM                           # noqa: E402


def band_tiles(chrom, bp, window):
    """tile count of build_clump_layout, restated"""
    order = np.lexsort((np.arange(len(bp)), bp, chrom))
    c, b = np.asarray(chrom)[order], np.asarray(bp)[order]
    n = len(b)
    hi = np.zeros(n, dtype=np.int64)
    q = 0
    for p in range(n):
        q = max(q, p)
        while q + 1 < n and c[q + 1] == c[p] and b[q + 1] - b[p] <= window:
            q += 1
        hi[p] = q
    tiles = 0
    for I in range((n + 31) // 32):
        p0, p1 = 32 * I, min(n, 32 * I + 32)
        tiles += int(np.any(hi[p0:p1 - 1] > np.arange(p0, p1 - 1))) + int(hi[p1 - 1] // 32 - I)
    return tiles


def time_clump(ctx, bed, n_ref, rows, chrom, bp, r2, kb, reps=5):
    ms = []
    for _ in range(reps + 1):
        clump(ctx, bed, n_ref, rows, chrom, bp, r2=r2, kb=kb)
        ms.append(ctx.clump_gpu_ms)
    return ms[1:]


def time_gram_i8(ctx, bed, n_ref, rows, reps=5, m=64):
    """blocks of m of the given rows, every block on dbslmm_gram_i8 (the 32 x 32 tiles of its lower
    triangle: three at m = 64, 528 at m = 1023), the run stopped after the Gram"""
    nb = len(rows) // m
    rows = np.asarray(rows[:m * nb], dtype=np.int32)
    prob = BlockProblem(bed=bed, n_ref=n_ref, n_obs=100000, sigma_s=0.5 / max(1, len(rows)),
                        s_ptr=m * np.arange(nb + 1), s_pos=rows, z_s=np.zeros(len(rows)),
                        opts=dict(gram_big_min=2 ** 31 - 1, gram_huge_min=2 ** 31 - 1, debug_stop=1, solver=1))
    plan = Plan(ctx, prob)
    plan.run()
    plan.sync()
    plan.enable_timing(True)
    for _ in range(reps):
        plan.run()
        plan.sync()
    ms, n = plan.kernel_ms()
    tiles = plan.workload()["gram_tiles"]
    plan.close()
    return float(ms[K_GRAM]), int(tiles), n


def report(name, ms, tiles, kpad):
    ops = tiles * 2.0 * 32 * 32 * kpad
    best = min(ms) if isinstance(ms, list) else ms
    out = dict(case=name, tiles=tiles, kpad=kpad, ops_per_tile=2 * 32 * 32 * kpad, gpu_ms=ms,
               tops=ops / (best * 1e-3) / 1e12 if best > 0 else None)
    print(json.dumps(out), flush=True)
    return out


def main():
    res = []
    ctx = Context(0)
    # test_dat
    td = os.path.join(ROOT, "tests", "golden", "test_dat")
    bed = np.fromfile(os.path.join(td, "ref_chr1.bed"), dtype=np.uint8)
    c = CR.summary_candidates(os.path.join(td, "summary_gemma_chr1.assoc.txt"), os.path.join(td, "ref_chr1.bim"), 1e-6)
    ctx.cache_bed(bed)
    for kb in (1000, 50):
        ms = time_clump(ctx, bed, 400, c["row"], c["chrom"], c["bp"], 0.2, kb)
        res.append(report(f"r2_tiles test_dat 444 candidates, {kb} kb", ms, band_tiles(c["chrom"], c["bp"], kb * 1000), 512))
    gms, gt, _ = time_gram_i8(ctx, bed, 400, c["row"])
    res.append(report("gram_i8 test_dat, blocks of 64 candidates", gms, gt, 512))
    ctx.cache_bed(None)
    # config-3 size: 500k SNPs x 5000 individuals, ~5 % of the rows as candidates
    t0 = time.time()
    panel = synth.simulate(500000, 5000, pop="EUR", seed=1, engine="gpu", device=0)
    print(f"panel: {panel.m} SNPs, {time.time() - t0:.1f} s", flush=True)
    rng = np.random.default_rng(5)
    rows = np.sort(rng.choice(panel.m, size=panel.m // 20, replace=False))
    prio = rng.permutation(len(rows))
    rows = rows[prio].astype(np.int32)
    chrom, bp = panel.chrom[rows].astype(np.int32), panel.ps[rows].astype(np.int64)
    ctx.cache_bed(panel.bed)
    kpad = 5120
    for kb in (1000, 250):
        t0 = time.time()
        ms = time_clump(ctx, panel.bed, 5000, rows, chrom, bp, 0.2, kb)
        wall = (time.time() - t0) / 6
        idx = clump(ctx, panel.bed, 5000, rows, chrom, bp, r2=0.2, kb=kb)
        out = report(f"r2_tiles config-3 size, {len(rows)} candidates, {kb} kb", ms, band_tiles(chrom, bp, kb * 1000), kpad)
        out["index_snps"] = int((idx == np.arange(len(idx))).sum())
        out["wall_ms_per_call"] = 1e3 * wall
        print(json.dumps(dict(index_snps=out["index_snps"], wall_ms_per_call=out["wall_ms_per_call"])), flush=True)
        res.append(out)
    pos_rows = np.sort(rows)
    for nblk_rows in (len(pos_rows), len(pos_rows) // 4):
        gms, gt, _ = time_gram_i8(ctx, panel.bed, 5000, pos_rows[:nblk_rows])
        res.append(report(f"gram_i8 config-3 size, {nblk_rows // 64} blocks of 64 candidate rows", gms, gt, kpad))
    # a dense list: 8192 consecutive rows as one chromosome inside one window, every tile J >= I
    dense = np.arange(20000, 20000 + 8192, dtype=np.int32)
    dprio = rng.permutation(8192)
    ms = time_clump(ctx, panel.bed, 5000, dense[dprio], np.ones(8192, dtype=np.int32), dprio.astype(np.int64), 0.2, 1000)
    res.append(report("r2_tiles config-3 size, 8192 consecutive rows, all pairs", ms,
                      band_tiles(np.ones(8192, dtype=np.int32), dprio, 10 ** 6), kpad))
    gms, gt, _ = time_gram_i8(ctx, panel.bed, 5000, np.arange(20000, 20000 + 62 * 1023), m=1023)
    res.append(report("gram_i8 config-3 size, 62 blocks of 1023 consecutive rows", gms, gt, kpad))
    if len(sys.argv) > 1:
        json.dump(res, open(sys.argv[1], "w"), indent=1)


if __name__ == "__main__":
    main()
