#!/usr/bin/env python3
"""niqki_query_collapsed at the index shape of bench.py: the 100 000 synthetic genomes in 500 families and the 4096
mixture queries of tools/bench_cover.py (S = 15, W = 12, -J 0.1), labels = what niqki_cluster returns at the same
threshold.  Everything in device memory.  JSON lines:

  labels      the labelling: distinct labels, the time of niqki_cluster and of niqki_set_labels (host clock)
  baseline    a plain niqki_query of the batch (top_k = 0) on the same handle, by HIP events: the existing call the
              collapsed one is compared with, never the new call against itself
  collapsed   niqki_query_collapsed of the same batch, by HIP events; entries in and out, queries on the global-table
              route, splits; "ratio" = median collapsed / median baseline
  phases      one more call while profiling is on: stats collapse_us_hits / _first / _emit
  lds_cap     the same call at other values of option "collapse_lds_cap"

    python tools/bench_collapse.py [--genomes 100000] [--queries 4096] [--repeats 5] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def median(x):
    return sorted(x)[len(x) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", type=int, default=100000)
    ap.add_argument("--queries", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from bench_cover import events_ms, make_index
    e, q = make_index(args, torch)
    nq = q.shape[0]
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    t0 = time.perf_counter()
    labels, n_clusters = e.cluster(e.min_score)
    t1 = time.perf_counter()
    e.set_labels(labels)
    t2 = time.perf_counter()
    emit({"case": "labels", "genomes": args.genomes, "queries": nq, "labels": e.stat("labels"), "clusters": n_clusters,
          "cluster_s": round(t1 - t0, 3), "set_labels_s": round(t2 - t1, 4)})
    # the full lists once through host memory (that path checks the capacity), for the size of the device arrays
    total = int(e.query(q.cpu().numpy(), capacity=nq * 512)[0][nq])
    ho = torch.zeros(nq + 1, dtype=torch.int64, device="cuda")
    cap = max(total, 1)
    hc, hg, hm = (torch.zeros(cap, dtype=torch.int32, device="cuda") for _ in range(3))
    e.query_dev(q, nq, ho, hc, hg, cap)
    torch.cuda.synchronize()
    base = [events_ms(torch, lambda: e.query_dev(q, nq, ho, hc, hg, cap)) for _ in range(args.repeats)]
    emit({"case": "baseline", "query_ms": base, "hits": total})

    def collapsed():
        assert e.query_collapsed_dev(q, nq, ho, hc, hg, hm, cap) == 0

    collapsed()                                               # warm-up: workspace allocations
    torch.cuda.synchronize()
    wall = [events_ms(torch, collapsed) for _ in range(args.repeats)]
    kept = int(ho[nq].item())
    emit({"case": "collapsed", "collapsed_ms": wall, "entries_in": total, "entries_out": kept, "lds_cap": 1024,
          "long_lists": e.stat("collapse_long_lists"), "splits": e.stat("collapse_splits"),
          "ratio": round(median(wall) / median(base), 4)})
    e.profile(True)
    collapsed()
    torch.cuda.synchronize()
    emit({"case": "phases", "hits_ms": e.stat("collapse_us_hits") / 1e3, "first_ms": e.stat("collapse_us_first") / 1e3,
          "emit_ms": e.stat("collapse_us_emit") / 1e3})
    for cap_l in (64, 256, 4096):
        e.set_option("collapse_lds_cap", cap_l)
        collapsed()
        torch.cuda.synchronize()
        emit({"case": "lds_cap", "lds_cap": cap_l, "long_lists": e.stat("collapse_long_lists"),
              "first_ms": e.stat("collapse_us_first") / 1e3, "emit_ms": e.stat("collapse_us_emit") / 1e3})
    e.profile(False)
    e.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
