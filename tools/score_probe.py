"""Time dbslmm_plan_score (the gpu_ms event time of its kernels) on a synthetic panel.

    python tools/score_probe.py [--snps 500000] [--n-ref 5000] [--n-test 10000] [--copies 1,3]
                                [--chunk-slots 0] [--reps 3] [--cpu-snps 8192]

Panel: synth at the config-3 SNP count, a second synthetic panel of --n-test individuals as the
target (same SNP rows).  Prints one JSON line per (copies, mode): the best of --reps gpu_ms, codes
per second (SNPs x individuals, every copy served by the same pass), panel bytes per second (2 bits
per code) and fp64 FMAs per second (one per code and copy).  For context only, the same product
on the CPU: NumPy / BLAS on --cpu-snps decoded SNPs (fp64 dosages, the threads the environment
allows), scaled to the panel.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dbslmm_amd import Context, Plan, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--snps", type=int, default=500000)
    ap.add_argument("--n-ref", type=int, default=5000)
    ap.add_argument("--n-test", type=int, default=10000)
    ap.add_argument("--copies", default="1,3")
    ap.add_argument("--chunk-slots", type=int, default=0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cpu-snps", type=int, default=8192)
    ap.add_argument("--subset", action="store_true", help="drop one individual: the compaction feeder")
    a = ap.parse_args()
    panel = synth.simulate(a.snps, a.n_ref, pop="EUR", seed=1, engine="gpu", device=0)
    prob = synth.make_problem(panel)
    target = synth.simulate(a.snps, a.n_test, pop="EUR", seed=2, engine="gpu", device=0)
    ind = None
    if a.subset:
        ind = np.ones(a.n_test, dtype=np.int32)
        ind[a.n_test // 3] = 0
    n_test = a.n_test - (1 if a.subset else 0)
    M = prob.n_s + prob.n_l
    ctx = Context(0)
    plan = Plan(ctx, prob)
    factors = {1: (1.0,), 2: (0.8, 1.2), 3: (0.8, 1.0, 1.2), 4: (0.7, 0.9, 1.0, 1.2)}
    for nc in [int(x) for x in a.copies.split(",")]:
        f = factors.get(nc) or tuple(np.linspace(0.7, 1.3, nc))
        plan.run_multi([prob.sigma_s * x for x in f])
        for mode in ("counts", "std"):
            ms, wall = [], []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                sc, dr = plan.score(target.bed, ind, prob.s_pos, prob.l_pos, mode=mode, n_total=a.n_test,
                                    chunk_slots=a.chunk_slots)
                wall.append(time.perf_counter() - t0)
                ms.append(plan.score_gpu_ms)
            best = min(ms) * 1e-3
            codes = float(M) * n_test
            print(json.dumps(dict(copies=nc, mode=mode, snps=M, n_test=n_test, feeder="compact" if a.subset else "image",
                                  gpu_ms=[round(x, 3) for x in ms], call_s=round(min(wall), 3),
                                  codes_per_s=codes / best, panel_bytes_per_s=codes / 4 / best,
                                  fma_per_s=codes * nc / best, dropped=dr.tolist(),
                                  score_absmax=float(np.abs(sc).max()))), flush=True)
    # context: the same product by BLAS on decoded fp64 dosages
    k = min(a.cpu_snps, M)
    rng = np.random.default_rng(0)
    G = rng.integers(0, 3, size=(k, n_test)).astype(np.float64)
    B = rng.standard_normal((3, k))
    t0 = time.perf_counter()
    for _ in range(3):
        (B @ G).sum()
    dt = (time.perf_counter() - t0) / 3
    print(json.dumps(dict(cpu_blas_3copies_s_per_panel=dt * M / k, cpu_snps_timed=k,
                          threads=os.environ.get("OMP_NUM_THREADS", "default"),
                          note="product only: decoding the 2-bit panel to fp64 is not included")), flush=True)
    plan.close()
    ctx.close()


if __name__ == "__main__":
    main()
