"""Times dbslmm_assoc: the HIP event time of the kernels of one call,
ctx.assoc_gpu_ms, at ASSOC_ROWS x ASSOC_N (default 100 000 rows x 10 000 individuals) with 4 covariates
and 1, 12 and 13 traits, on a panel with 1 % missing calls and on one without, for three chunk sizes.
One JSON line per configuration: the warm-up call and the sorted times of five more.

    python tools/assoc_probe.py [OUT.json]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dbslmm_amd import Context, assoc  # noqa: E402

N_ROWS, N = int(os.environ.get("ASSOC_ROWS", 100_000)), int(os.environ.get("ASSOC_N", 10_000))
REPS = 5


def make_bed(rng, miss):
    bps = (N + 3) // 4
    body = np.empty((N_ROWS, bps), dtype=np.uint8)
    for r0 in range(0, N_ROWS, 5000):
        r1 = min(N_ROWS, r0 + 5000)
        f = rng.uniform(0.05, 0.5, size=(r1 - r0, 1))
        u = rng.random((r1 - r0, 4 * bps), dtype=np.float32)
        code = np.full(u.shape, 3, dtype=np.uint8)               # 11: dosage 0
        code[u < 2 * f * (1 - f) + f * f] = 2                    # 10: dosage 1
        code[u < f * f] = 0                                      # 00: dosage 2
        if miss > 0:
            code[rng.random(u.shape, dtype=np.float32) < miss] = 1
        code[:, N:] = 0
        c = code.reshape(r1 - r0, bps, 4)
        body[r0:r1] = c[:, :, 0] | (c[:, :, 1] << 2) | (c[:, :, 2] << 4) | (c[:, :, 3] << 6)
    return np.concatenate([np.array([0x6C, 0x1B, 0x01], dtype=np.uint8), body.reshape(-1)])


def main():
    rng = np.random.default_rng(1)
    ctx = Context(0)
    out = dict(rows=N_ROWS, individuals=N, reps=REPS, runs=[])
    for miss in (0.01, 0.0):
        t0 = time.time()
        bed = make_bed(rng, miss)
        print(f"panel miss {miss}: {bed.size / 1e6:.0f} MB in {time.time() - t0:.1f} s", flush=True)
        ctx.cache_bed(bed)
        for c1, P in ((4, 1), (4, 12), (4, 13)):
            y = rng.standard_normal((N, P))
            w = rng.standard_normal((N, c1))
            for chunk in (0, 1024, 10240):
                ms = []
                for rep in range(REPS + 1):                      # the first call warms up
                    r = assoc(ctx, bed, N, y, w, chunk_indiv=chunk)
                    ms.append(ctx.assoc_gpu_ms)
                rec = dict(miss=miss, columns=c1 + P, chunk_indiv=chunk, warm_ms=ms[0], ms=sorted(ms[1:]),
                           ok_rows=int(np.sum(r["status"] == 0)), mean_n_mis=float(np.mean(r["n_mis"])))
                print(json.dumps(rec), flush=True)
                out["runs"].append(rec)
        ctx.cache_bed(None)
    if len(sys.argv) > 1:
        json.dump(out, open(sys.argv[1], "w"), indent=1)


if __name__ == "__main__":
    main()
