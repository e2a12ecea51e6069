"""dbslmm_pcg_block without the chip-wide path beside it: a units plan of one bench config that keeps
only the blocks the whole-block kernel takes (at most 8 tile rows; every larger block goes to a
second, untimed device), so the launch's HIP-event span is the kernel alone.  Prints ms per run,
the GB/s per CU its algorithmic bytes (iterations x lower-triangle uint16 bytes, plan workload
[21]) amount to, and the iteration counts.  GPU; usage:
python tools/pcg_block_probe.py [config] [OUT_JSON] [runs]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dbslmm_amd import Context, KERNEL_NAMES, Plan, synth      # noqa: E402
from r06_dev import CFG                                          # noqa: E402

N_CU = 256
MAX_ROWS = 8 * 128 - 1     # kFTb tile rows of 128, one row kept free


def main(cfg=4, out=None, runs=10):
    snps, n_ref, pop, lmm, f = CFG[cfg]
    pan = synth.simulate(snps, n_ref, pop=pop, seed=1, engine="gpu")
    prob = synth.make_problem(pan, lmm_only=lmm)
    del pan
    sig = [prob.sigma_s * x for x in f]
    K = len(sig)
    m = np.diff(prob.s_ptr) + (np.diff(prob.l_ptr) if prob.l_ptr is not None else 0)
    keep = (m > 0) & (m <= MAX_ROWS)
    ud = np.ones((prob.num_block, K), dtype=np.int32)
    ud[keep, :] = 0
    plan = Plan.units(Context(0), prob, ud, 0)
    o = (np.zeros((K, prob.n_s)), np.zeros((K, prob.n_l)), np.zeros((K, prob.num_block), dtype=np.int32))
    for _ in range(3):
        plan.run_multi(sig, out=o)
    plan.sync()
    plan.enable_timing(True)
    t0 = time.perf_counter()
    for _ in range(runs):
        plan.run_multi(sig, out=o)
    plan.sync()
    wall = (time.perf_counter() - t0) / runs * 1e3
    ms, nl = plan.kernel_ms()
    ms = ms * nl / runs                       # per run, as bench.py counts
    wl = plan.workload()
    it = plan.block_iters()[keep]
    kms = float(ms[KERNEL_NAMES.index("dbslmm_pcg_block")])
    b = float(wl.get("pcg_block_bytes", 0.0))
    r = dict(config=cfg, blocks=int(keep.sum()), snps=int(m[keep].sum()), copies=K, wall_ms=wall,
             pcg_block_ms=kms, pcg_ms=float(ms[KERNEL_NAMES.index("dbslmm_pcg")]),
             gram_ms=float(ms[KERNEL_NAMES.index("dbslmm_gram")]), algorithmic_bytes=b,
             gbs=b / kms / 1e6 if kms > 0 else 0.0, gbs_per_cu=b / kms / 1e6 / N_CU if kms > 0 else 0.0,
             iters_max=int(it.max()), iters_mean=float(it.mean()),
             status_nonzero=int(np.sum(o[2][:, keep] != 0)))
    print(json.dumps(r), flush=True)
    if out:
        json.dump(r, open(out, "w"), indent=1)


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 4, sys.argv[2] if len(sys.argv) > 2 else None,
         int(sys.argv[3]) if len(sys.argv) > 3 else 10)
