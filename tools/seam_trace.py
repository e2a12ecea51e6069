"""The seams of the PCG route's step in a rocprofv3 kernel trace of bench.py (--kernel-trace, csv):
per timed step (every run of dbslmm_gram_huge but the first `skip`), in microseconds,
  front    first GPU work of the step (after the previous dbslmm_pcg_final's copies) -> Gram start
  n_front  kernels and fills in that span
  seam     Gram end (the last dbslmm_gram_*) -> dbslmm_pcg_init end
  init     dbslmm_pcg_init alone
  block    dbslmm_pcg_block
  tail     dbslmm_pcg_block end -> dbslmm_pcg_final end
  pcg      dbslmm_pcg_init start -> dbslmm_pcg_final end
  step     first GPU work -> dbslmm_pcg_final end
usage: python tools/seam_trace.py TRACE_kernel_trace.csv [skip]"""
import csv
import statistics
import sys


def main(path, skip=2):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    name = [r["Kernel_Name"].split("(")[0] for r in rows]
    st = [int(r["Start_Timestamp"]) for r in rows]
    en = [int(r["End_Timestamp"]) for r in rows]
    finals = [i for i, n in enumerate(name) if n == "dbslmm_pcg_final"]
    out = []
    for a, b in zip(finals[:-1], finals[1:]):
        seg = range(a + 1, b + 1)
        gram = [i for i in seg if name[i].startswith("dbslmm_gram")]
        if not gram or not any(name[i] == "dbslmm_gram_huge" for i in gram):
            continue
        init = next(i for i in seg if name[i] == "dbslmm_pcg_init")
        blk = [i for i in seg if name[i] == "dbslmm_pcg_block"]
        # the step's first work: what follows the previous step's device-to-host copies
        first = next(i for i in seg if "copyBuffer" not in name[i])
        g0, g1 = st[gram[0]], max(en[i] for i in gram)
        out.append(dict(front=g0 - st[first], n_front=gram[0] - first, seam=en[init] - g1, init=en[init] - st[init],
                        block=en[blk[0]] - st[blk[0]] if blk else 0, tail=en[b] - en[blk[0]] if blk else 0,
                        pcg=en[b] - st[init], step=en[b] - st[first]))
    out = out[skip:] if len(out) > skip else out
    for k in out[0]:
        v = [o[k] / (1.0 if k == "n_front" else 1e3) for o in out]
        print(f"{k:8s} median {statistics.median(v):9.1f}   " + " / ".join(f"{x:.1f}" for x in v))


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 2)
