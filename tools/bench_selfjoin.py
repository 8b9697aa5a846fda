#!/usr/bin/env python3
"""The self-join (niqki_cluster, niqki_dereplicate, niqki_linkage) at the index shape of bench.py: 100 000 genomes, S = 15, W = 12, -J 0.1.  The index
is made of synthetic sketches (families of related genomes, made and inserted on the device, as tools/bench_topk.py
does).  Every case runs in a child process of its own under its own time limit, one after the other; the first that
fails ends the run.  One JSON line per case:

  cluster     niqki_cluster: wall time, and by HIP events (profiling on: one synchronisation per batch) the store
              read, gather + hits, link and flatten phases, hits linked per second
  host        the only alternative without niqki_cluster: the same hits fetched with niqki_get_sketches +
              niqki_query to the host and united by numpy, on a SLICE of --slice genomes; "extrapolated_s" is that
              time x genomes / slice -- an extrapolation, not a measurement
  one         the link kernel's contention case: --extreme identical genomes, ONE component, every hit redundant
  singletons  unrelated genomes at a threshold nothing reaches: every list holds the genome itself only
  derep, derep_one, derep_singletons
              niqki_dereplicate on the indexes of cluster / one / singletons, and niqki_cluster on the SAME handle in
              the same process as the yardstick: the read and hits phases are the same work, the decide + assign
              phases stand beside the link + flatten phases
  derep_path  the decide rounds' worst case: --path genomes, each linked to its two index neighbours only, inside
              one batch; microseconds per round
  linkage, linkage_one, linkage_singletons
              niqki_linkage(floor) on the indexes of cluster / one / singletons, floor = the cluster case's threshold,
              and niqki_cluster(floor) on the SAME handle in the same process as the yardstick: the read and hits
              phases are the same work, the forest + finish phases stand beside the link + flatten phases; a cut of
              the hierarchy at the floor is compared with the cluster labels

    python tools/bench_selfjoin.py [--genomes 100000] [--slice 4096] [--extreme 20000] [--path 1024] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
K, S, W, H = 31, 15, 12, 4
F = 1 << S


def make_index(args, kind):
    import torch
    import niqki_amd
    from niqki_amd import capi
    dev = torch.device("cuda")
    g = torch.Generator(device=dev)
    g.manual_seed(args.seed)
    N = args.genomes if kind == "families" else args.extreme
    n_fam = 500
    fam = torch.randint(0, 1 << W, (n_fam, F), dtype=torch.int32, device=dev, generator=g)
    e = niqki_amd.Engine(K=K, S=S, W=W, H=H, min_score_value=capi.min_score(0.1, S))
    e.set_stream(torch.cuda.current_stream().cuda_stream)
    for a in range(0, N, 4096):
        n = min(4096, N - a)
        if kind == "families":      # members with 20-90 % of their cells replaced: pairs from 0.64 down to chance
            sk = fam[torch.randint(0, n_fam, (n,), device=dev, generator=g)].clone()
            m = torch.rand(sk.shape, device=dev, generator=g) < 0.2 + 0.7 * torch.rand((n, 1), device=dev, generator=g)
            sk[m] = torch.randint(0, 1 << W, (int(m.sum().item()),), dtype=torch.int32, device=dev, generator=g)
        elif kind == "one":
            sk = fam[:1].expand(n, F).contiguous()
        else:
            sk = torch.randint(0, 1 << W, (n, F), dtype=torch.int32, device=dev, generator=g)
        e.insert_dev(sk, n)
    e.build()
    torch.cuda.synchronize()
    return e, N


def case_cluster(args, kind):
    import torch
    e, N = make_index(args, kind)
    thr = e.min_score if kind != "singletons" else F // 2
    e.cluster(thr)                                     # warm-up: workspace allocations
    t = time.time()
    labels, n = e.cluster(thr)
    wall = time.time() - t
    e.profile(True)
    e.cluster(thr)
    e.profile(False)
    us = {k: e.stat("cluster_us_" + k) for k in ("read", "hits", "link", "flatten")}
    pairs = e.stat("cluster_pairs")
    res = {"case": "cluster" if kind == "families" else kind, "genomes": N, "threshold": int(thr), "clusters": n,
           "wall_s": round(wall, 3), "phases_ms": {k: round(v / 1e3, 3) for k, v in us.items()}, "hits": pairs,
           "splits": e.stat("cluster_splits"), "hits_linked_per_s": round(pairs / max(us["link"], 1) * 1e6),
           "link_plus_flatten_over_gather_plus_hits": round((us["link"] + us["flatten"]) / max(us["hits"], 1), 4)}
    e.close()
    torch.cuda.synchronize()
    return res


def make_path_index(args):
    """--path genomes in index order, each the one before with 20 % of its cells drawn again: consecutive ones share
    0.8, two apart 0.64; the threshold lies between"""
    import torch
    import niqki_amd
    dev = torch.device("cuda")
    g = torch.Generator(device=dev)
    g.manual_seed(args.seed)
    n = args.path
    rows = [torch.randint(0, 1 << W, (F,), dtype=torch.int32, device=dev, generator=g)]
    for _ in range(n - 1):
        s = rows[-1].clone()
        m = torch.rand((F,), device=dev, generator=g) < 0.2
        s[m] = torch.randint(0, 1 << W, (int(m.sum().item()),), dtype=torch.int32, device=dev, generator=g)
        rows.append(s)
    e = niqki_amd.Engine(K=K, S=S, W=W, H=H, min_score_value=int(0.72 * F))
    e.set_stream(torch.cuda.current_stream().cuda_stream)
    e.set_option("query_batch", max(n, 1))
    e.insert_dev(torch.stack(rows).contiguous(), n)
    e.build()
    torch.cuda.synchronize()
    return e, n


def case_derep(args, kind):
    import torch
    if kind == "path":
        e, N = make_path_index(args)
        thr = e.min_score
    else:
        e, N = make_index(args, kind)
        thr = e.min_score if kind != "singletons" else F // 2
    e.dereplicate(thr)                                 # warm-up: workspace allocations
    t = time.time()
    labels, n = e.dereplicate(thr)
    wall = time.time() - t
    e.cluster(thr)
    t = time.time()
    _, n_cl = e.cluster(thr)
    wall_cl = time.time() - t
    e.profile(True)
    e.dereplicate(thr)
    us = {k: e.stat("derep_us_" + k) for k in ("read", "hits", "decide", "assign")}
    pairs, rounds, splits = e.stat("derep_pairs"), e.stat("derep_rounds"), e.stat("derep_splits")
    e.cluster(thr)
    e.profile(False)
    cl = {k: e.stat("cluster_us_" + k) for k in ("read", "hits", "link", "flatten")}
    res = {"case": "derep" if kind == "families" else "derep_" + kind, "genomes": N, "threshold": int(thr),
           "representatives": n, "clusters": n_cl, "wall_s": round(wall, 3), "cluster_wall_s": round(wall_cl, 3),
           "phases_ms": {k: round(v / 1e3, 3) for k, v in us.items()},
           "cluster_phases_ms": {k: round(v / 1e3, 3) for k, v in cl.items()}, "hits": pairs, "rounds": rounds,
           "splits": splits,
           "decide_plus_assign_over_gather_plus_hits": round((us["decide"] + us["assign"]) / max(us["hits"], 1), 4),
           "link_plus_flatten_over_gather_plus_hits": round((cl["link"] + cl["flatten"]) / max(cl["hits"], 1), 4)}
    if kind == "path":
        res["decide_us_per_round"] = round(us["decide"] / max(rounds, 1), 2)
    e.close()
    torch.cuda.synchronize()
    return res


def case_linkage(args, kind):
    import numpy as np
    import torch
    import niqki_amd
    e, N = make_index(args, kind)
    thr = e.min_score if kind != "singletons" else F // 2
    e.linkage(thr)                                     # warm-up: workspace allocations
    t = time.time()
    into, cnt, edges, roots = e.linkage(thr)
    wall = time.time() - t
    e.cluster(thr)
    t = time.time()
    labels, n_cl = e.cluster(thr)
    wall_cl = time.time() - t
    same = bool(np.array_equal(niqki_amd.cut_linkage(into, cnt, thr), labels)) and roots == n_cl
    e.profile(True)
    e.linkage(thr)
    us = {k: e.stat("linkage_us_" + k) for k in ("read", "hits", "forest", "finish")}
    pairs, rounds, splits = e.stat("linkage_pairs"), e.stat("linkage_rounds"), e.stat("linkage_splits")
    e.cluster(thr)
    e.profile(False)
    cl = {k: e.stat("cluster_us_" + k) for k in ("read", "hits", "link", "flatten")}
    res = {"case": "linkage" if kind == "families" else "linkage_" + kind, "genomes": N, "floor": int(thr),
           "roots": roots, "clusters": n_cl, "cut_at_floor_equals_cluster": same, "wall_s": round(wall, 3),
           "cluster_wall_s": round(wall_cl, 3), "wall_over_cluster_wall": round(wall / max(wall_cl, 1e-9), 3),
           "phases_ms": {k: round(v / 1e3, 3) for k, v in us.items()},
           "cluster_phases_ms": {k: round(v / 1e3, 3) for k, v in cl.items()}, "hits": pairs, "rounds": rounds,
           "splits": splits,
           "forest_plus_finish_over_gather_plus_hits": round((us["forest"] + us["finish"]) / max(us["hits"], 1), 4),
           "link_plus_flatten_over_gather_plus_hits": round((cl["link"] + cl["flatten"]) / max(cl["hits"], 1), 4)}
    e.close()
    torch.cuda.synchronize()
    return res


def case_host(args):
    import numpy as np
    e, N = make_index(args, "families")
    n = min(args.slice, N)
    e.query(e.get_sketches(0, 64))                     # warm-up
    t = time.time()
    off, _, hg = e.query(e.get_sketches(0, n))
    t_fetch = time.time() - t
    a = np.repeat(np.arange(n), np.diff(off.astype(np.int64)))
    b = hg.astype(np.int64)
    parent = np.arange(N, dtype=np.int64)
    while True:                                        # union-find in numpy: compress, hook larger roots under smaller
        while True:
            pp = parent[parent]
            if np.array_equal(pp, parent):
                break
            parent = pp
        ra, rb = parent[a], parent[b]
        m = ra != rb
        if not m.any():
            break
        np.minimum.at(parent, np.maximum(ra[m], rb[m]), np.minimum(ra[m], rb[m]))
    t_all = time.time() - t
    e.close()
    return {"case": "host", "genomes": N, "slice": n, "hits": int(off[-1]), "fetch_s": round(t_fetch, 3),
            "slice_s": round(t_all, 3), "extrapolated_s": round(t_all * N / n, 1),
            "note": "extrapolated_s = slice_s x genomes / slice: an extrapolation"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", type=int, default=100000)
    ap.add_argument("--slice", type=int, default=4096)
    ap.add_argument("--extreme", type=int, default=20000)
    ap.add_argument("--path", type=int, default=1024)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per case")
    ap.add_argument("--only", default=None, help="comma-separated cases instead of all of them")
    ap.add_argument("--out", default=None)
    ap.add_argument("--case", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.case:
        if args.case.startswith("derep"):
            res = case_derep(args, args.case[6:] or "families")
        elif args.case.startswith("linkage"):
            res = case_linkage(args, args.case[8:] or "families")
        else:
            res = case_host(args) if args.case == "host" else case_cluster(args, args.case)
        print(json.dumps(res), flush=True)
        return 0
    lines = []
    for case in ("families", "host", "one", "singletons", "derep", "derep_one", "derep_singletons", "derep_path",
                 "linkage", "linkage_one", "linkage_singletons"):
        if args.only and case not in args.only.split(","):
            continue
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--case", case,
               "--genomes", str(args.genomes), "--slice", str(args.slice), "--extreme", str(args.extreme),
               "--path", str(args.path), "--seed", str(args.seed)]
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
