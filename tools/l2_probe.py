"""gpu_ms of the LD score kernels (dbslmm_l2_tiles + dbslmm_l2_reduce, dbslmm_ld_scores) on a config-3-size
synthetic panel, next to dbslmm_gram_big on plans with the same number of 128 x 128 tiles and the same
kpad in the same session, and to dbslmm_r2_tiles (the route LD scores had before: 32 x 32 tiles) on
the dense case (profiles/r14).

    python tools/l2_probe.py band  [OUT.json]   # every row of the panel, and of its largest chromosome: 1000 / 250 kb
    python tools/l2_probe.py dense [OUT.json]   # 8192 consecutive rows inside one window

One JSON line per case on stdout.  Best of five timed calls after one warm-up, the panel image cached
on the context.  Rate = tiles * 2 * 128 * 128 * kpad ops / best gpu_ms (diagonal tiles counted whole)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

from dbslmm_amd import BlockProblem, Context, Plan, clump, ld_r2, ld_scores, synth   # noqa: E402
from dbslmm_amd._lib import K_GRAM                                                   # noqa: E402

N_REF, KPAD = 5000, 5120


def band_tiles128(chrom, bp, window):
    """tile count of build_ldsc_layout, restated (rows already in position order)"""
    n = len(bp)
    hi = np.zeros(n, dtype=np.int64)
    q = 0
    for p in range(n):
        q = max(q, p)
        while q + 1 < n and chrom[q + 1] == chrom[p] and bp[q + 1] - bp[p] <= window:
            q += 1
        hi[p] = q
    return sum(int(hi[min(n, 128 * (I + 1)) - 1] // 128 - I) + 1 for I in range((n + 127) // 128))


def time_l2(ctx, bed, rows, chrom, bp, kb, reps=5):
    ms = []
    for _ in range(reps + 1):
        ld_scores(ctx, bed, N_REF, rows, chrom, bp, kb=kb)
        ms.append(ctx.l2_gpu_ms)
    return ms[1:]


def time_gram_big(ctx, bed, first_row, n_blocks, m, reps=5):
    """n_blocks blocks of m consecutive rows, every block on dbslmm_gram_big (T (T + 1) / 2 tiles of 128 x
    128 per block, T = ceil(m / 128)), the run stopped after the Gram: (ms per run, tiles)"""
    rows = np.arange(first_row, first_row + m * n_blocks, dtype=np.int32)
    prob = BlockProblem(bed=bed, n_ref=N_REF, n_obs=100000, sigma_s=0.5 / len(rows),
                        s_ptr=m * np.arange(n_blocks + 1), s_pos=rows, z_s=np.zeros(len(rows)),
                        opts=dict(gram_big_min=128, gram_huge_min=2 ** 31 - 1, debug_stop=1, solver=1))
    plan = Plan(ctx, prob)
    plan.run()
    plan.sync()
    plan.enable_timing(True)
    for _ in range(reps):
        plan.run()
        plan.sync()
    ms, _ = plan.kernel_ms()
    w = plan.workload()
    plan.close()
    T = (m + 127) // 128
    return float(ms[K_GRAM]), n_blocks * T * (T + 1) // 2, w["gram_ops_exec"]


def report(res, name, ms, tiles, **extra):
    best = min(ms) if isinstance(ms, list) else ms
    out = dict(case=name, tiles=tiles, kpad=KPAD, ops_per_tile=2 * 128 * 128 * KPAD, gpu_ms=ms,
               tops=tiles * 2.0 * 128 * 128 * KPAD / (best * 1e-3) / 1e12 if best > 0 else None, **extra)
    print(json.dumps(out), flush=True)
    res.append(out)


def main():
    case = sys.argv[1] if len(sys.argv) > 1 else "band"
    res = []
    ctx = Context(0)
    t0 = time.time()
    panel = synth.simulate(500000, N_REF, pop="EUR", seed=1, engine="gpu", device=0)
    print(f"panel: {panel.m} SNPs, {time.time() - t0:.1f} s", flush=True)
    ctx.cache_bed(panel.bed)
    chrom_all, bp_all = panel.chrom.astype(np.int32), panel.ps.astype(np.int64)
    if case == "band":
        big = np.bincount(chrom_all).argmax()
        for name, rows in (("every row of the panel", np.arange(panel.m, dtype=np.int32)),
                           (f"the rows of chromosome {big}", np.flatnonzero(chrom_all == big).astype(np.int32))):
            order = np.lexsort((rows, bp_all[rows], chrom_all[rows]))
            rows = rows[order]
            chrom, bp = chrom_all[rows], bp_all[rows]
            for kb in (1000, 250):
                t0 = time.time()
                ms = time_l2(ctx, panel.bed, rows, chrom, bp, kb)
                wall = (time.time() - t0) / 6
                tiles = band_tiles128(chrom, bp, kb * 1000)
                report(res, f"l2_tiles {name} ({len(rows)}), {kb} kb", ms, tiles, wall_ms_per_call=1e3 * wall)
                # the same number of tiles on gram_big: blocks of 256 consecutive rows, three tiles each
                # (at most the panel's rows: the rate is what is compared)
                nb = max(1, min(tiles // 3, panel.m // 256))
                gms, gt, gops = time_gram_big(ctx, panel.bed, 0, nb, 256)
                report(res, f"gram_big {nb} blocks of 256 rows", gms, gt, gram_ops_exec=gops)
    else:
        dense = np.arange(20000, 20000 + 8192, dtype=np.int32)
        ones, pos = np.ones(8192, dtype=np.int32), np.arange(8192, dtype=np.int64)
        ms = time_l2(ctx, panel.bed, dense, ones, pos, 1000)
        report(res, "l2_tiles 8192 consecutive rows inside one window", ms, 64 * 65 // 2)
        # 2080 tiles on gram_big: 208 blocks of 512 rows (ten tiles each), and 26 of 1536 (78 each: 2028)
        for nb, m in ((208, 512), (26, 1536)):
            gms, gt, gops = time_gram_big(ctx, panel.bed, 20000, nb, m)
            report(res, f"gram_big {nb} blocks of {m} rows", gms, gt, gram_ops_exec=gops)
        # the route before: dbslmm_r2_tiles over the same pairs (32 x 32 tiles, in 128-tile units here) --
        # mask mode through dbslmm_clump (event time of the kernel), value mode through ld_r2 (wall time:
        # it returns 512 MiB of r2, which the caller still has to sum)
        cms = []
        for _ in range(6):
            clump(ctx, panel.bed, N_REF, dense, ones, pos, r2=0.2, kb=1000)
            cms.append(ctx.clump_gpu_ms)
        report(res, "r2_tiles (clump, mask mode) the same 8192 rows", cms[1:], 64 * 65 // 2, tiles32=256 * 257 // 2)
        t0 = time.time()
        r2 = ld_r2(ctx, panel.bed, N_REF, dense)
        t1 = time.time()
        s = np.nansum(r2, axis=1)
        t2 = time.time()
        l2, _ = ld_scores(ctx, panel.bed, N_REF, dense, ones, pos, kb=1000, unbiased=False)
        print(json.dumps(dict(case="ld_r2 8192 rows + host row sums", wall_ms=1e3 * (t1 - t0), sum_ms=1e3 * (t2 - t1),
                              max_rel_diff_to_ld_scores=float(np.nanmax(np.abs(s - l2) / l2)))), flush=True)
    if len(sys.argv) > 2:
        json.dump(res, open(sys.argv[2], "w"), indent=1)


if __name__ == "__main__":
    main()
