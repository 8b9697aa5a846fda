#!/usr/bin/env python3
"""The label audit (niqki_audit) at the index shape of bench.py: 100 000 genomes, S = 15, W = 12, -J 0.1, on the
synthetic indexes of tools/bench_selfjoin.py.  The yardstick is niqki_cluster on the SAME handle in the same process at
the same threshold: the read and hits phases are the same work, the scan of the lists stands beside the link kernel.
Every case runs in a child process of its own under its own time limit, one after the other; the first that fails
ends the run.  One JSON line per case:

  audit             the families index; the labels are its own single-linkage clusters at the threshold with 2 % of the
                    genomes moved to another genome's label; --k neighbours vote
  audit_one         --extreme identical genomes under ONE label: every list holds every genome and no entry is
                    foreign, so every wavefront walks its whole list -- the longest scan there is
  audit_singletons  unrelated genomes at a threshold nothing reaches: every list holds the genome itself only

    python tools/bench_audit.py [--genomes 100000] [--extreme 20000] [--k 5] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_selfjoin import F, make_index  # noqa: E402

CASES = {"audit": "families", "audit_one": "one", "audit_singletons": "singletons"}


def case_audit(args, case):
    import numpy as np
    import torch
    from niqki_amd import capi
    kind = CASES[case]
    e, N = make_index(args, kind)
    thr = e.min_score if kind != "singletons" else F // 2
    labels, n_cl = e.cluster(thr)                      # (also the warm-up of the shared workspaces)
    if kind == "families":
        rng = np.random.default_rng(args.seed)
        moved = rng.choice(N, N // 50, replace=False)
        labels[moved] = labels[rng.integers(0, N, moved.size)]
    e.set_labels(labels)
    e.audit(thr, args.k)                               # warm-up: workspace allocations
    t = time.time()
    rows = e.audit(thr, args.k)
    wall = time.time() - t
    t = time.time()
    e.cluster(thr)
    wall_cl = time.time() - t
    e.profile(True)
    e.audit(thr, args.k)
    us = {k: e.stat("audit_us_" + k) for k in ("read", "hits", "scan")}
    pairs, splits = e.stat("audit_pairs"), e.stat("audit_splits")
    e.cluster(thr)
    e.profile(False)
    cl = {k: e.stat("cluster_us_" + k) for k in ("read", "hits", "link", "flatten")}
    verdicts = np.bincount(rows[0], minlength=5).tolist()
    res = {"case": case, "genomes": N, "threshold": int(thr), "k": args.k, "labels": e.stat("labels"), "clusters": n_cl,
           "verdicts": dict(zip(capi.AUDIT_VERDICTS, verdicts)), "wall_s": round(wall, 3), "cluster_wall_s": round(wall_cl, 3),
           "phases_ms": {k: round(v / 1e3, 3) for k, v in us.items()},
           "cluster_phases_ms": {k: round(v / 1e3, 3) for k, v in cl.items()}, "hits": pairs, "splits": splits,
           "audit_us_hits": us["hits"], "audit_us_scan": us["scan"], "cluster_us_hits_plus_link": cl["hits"] + cl["link"],
           "scan_over_gather_plus_hits": round(us["scan"] / max(us["hits"], 1), 4),
           "link_over_gather_plus_hits": round(cl["link"] / max(cl["hits"], 1), 4)}
    e.close()
    torch.cuda.synchronize()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", type=int, default=100000)
    ap.add_argument("--extreme", type=int, default=20000)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per case")
    ap.add_argument("--only", default=None, help="comma-separated cases instead of all of them")
    ap.add_argument("--out", default=None)
    ap.add_argument("--case", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.case:
        print(json.dumps(case_audit(args, args.case)), flush=True)
        return 0
    lines = []
    for case in CASES:
        if args.only and case not in args.only.split(","):
            continue
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--case", case,
               "--genomes", str(args.genomes), "--extreme", str(args.extreme), "--k", str(args.k), "--seed", str(args.seed)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:                          # nothing more on the GPU after a failure
            print("case %s failed with exit status %d\n%s" % (case, r.returncode, r.stderr[-2000:]), flush=True)
            return 1
        lines.append(r.stdout.strip().split("\n")[-1])
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "a" if args.only else "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
