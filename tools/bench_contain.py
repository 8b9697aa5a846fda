#!/usr/bin/env python3
"""Containment search (niqki_query_contained) at the index shape of bench.py: 100 000 genomes of random cells, S = 15,
W = 12, a batch of 4096 query sketches on the device, sizes drawn between 10^6 and 10^7.  Times the call at a low
floor with top_k = 10 against niqki_query at the same floor with top_k = 10 on the same handle -- the path a caller
had before, which cuts by count -- and reports the bytes each returns and the contained call's phases (stats
"contain_us_hits", "contain_us_share", "contain_us_order", while profiling is on).  Prints one JSON line per case:
medians over --runs runs of --steps calls each, with the range of the runs.

    python tools/bench_contain.py [--genomes 100000] [--nq 4096] [--floor 14] [--k 10] [--runs 3] [--steps 3]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", type=int, default=100000)
    ap.add_argument("--nq", type=int, default=4096)
    ap.add_argument("--floor", type=int, default=14, help="min_score: random cells share F / 2^W = 8 slots on average")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--mode", type=int, default=0)
    ap.add_argument("--min-share", type=float, default=0.001)
    ap.add_argument("--seed", type=int, default=7)
    args = ap.parse_args()
    import torch
    import niqki_amd
    from niqki_amd import capi

    K, S, W, H = 31, 15, 12, 4
    F, N, nq, k = 1 << S, args.genomes, args.nq, args.k
    dev = torch.device("cuda")
    g = torch.Generator(device=dev)
    g.manual_seed(args.seed)
    e = niqki_amd.Engine(K=K, S=S, W=W, H=H, min_score_value=args.floor, top_k=k)
    e.set_stream(torch.cuda.current_stream().cuda_stream)
    t0 = time.time()
    for a in range(0, N, 4096):
        n = min(4096, N - a)
        e.insert_dev(torch.randint(0, 1 << W, (n, F), dtype=torch.int32, device=dev, generator=g), n)
    q = torch.randint(0, 1 << W, (nq, F), dtype=torch.int32, device=dev, generator=g)
    e.build()
    sizes = torch.randint(10 ** 6, 10 ** 7, (N,), dtype=torch.int64, device=dev, generator=g)
    qsizes = torch.randint(10 ** 6, 10 ** 7, (nq,), dtype=torch.int64, device=dev, generator=g)
    e.set_sizes(sizes)
    torch.cuda.synchronize()
    min_share = min(int(args.min_share * 2 ** 32), capi.CONTAIN_ONE)
    cap = nq * k
    off = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
    hs, hc, hg = (torch.empty(cap, dtype=torch.int32, device=dev) for _ in range(3))
    nu = torch.empty(nq, dtype=torch.int32, device=dev)
    print(json.dumps({"genomes": N, "nq": nq, "S": S, "W": W, "floor": args.floor, "top_k": k, "mode": args.mode, "min_share": min_share,
                      "build_s": round(time.time() - t0, 1)}), flush=True)

    def plain():
        e.query_dev(q, nq, off, hc, hg, cap)

    def contained():
        e.query_contained_dev(q, qsizes, nq, args.mode, min_share, off, hs, hc, hg, nu, cap)

    def timed(call):
        call()                                             # warm-up (workspace allocations)
        torch.cuda.synchronize()
        runs = []
        for _ in range(args.runs):
            t = time.time()
            for _ in range(args.steps):
                call()
            torch.cuda.synchronize()
            runs.append((time.time() - t) / args.steps * 1e3)
        return {"ms_median": round(statistics.median(runs), 3), "ms_min": round(min(runs), 3), "ms_max": round(max(runs), 3)}

    res_plain = dict(case="niqki_query top_k", **timed(plain))
    res_plain.update(entries=int(off[-1].item()), bytes_returned=int(off[-1].item()) * 8 + (nq + 1) * 8)
    print(json.dumps(res_plain), flush=True)
    # the full lists the contained call selects from: the batch at top_k = 0, counted only (nothing written)
    e.set_option("top_k", 0)
    one = torch.zeros(1, dtype=torch.int32, device=dev)
    e.query_dev(q, nq, off, one, one, 0)
    full_hits = int(off[-1].item())
    e.set_option("top_k", k)
    res = dict(case="niqki_query_contained", **timed(contained))
    res.update(entries=int(off[-1].item()), bytes_returned=int(off[-1].item()) * 12 + (nq + 1) * 8 + nq * 4, full_list_hits=full_hits,
               full_list_bytes=full_hits * 8, unsized=int(nu.sum().item()), long_lists=e.stat("contain_long_lists"), splits=e.stat("contain_splits"))
    e.profile(True)
    phases = []
    for _ in range(args.runs):
        contained()
        torch.cuda.synchronize()
        phases.append([e.stat("contain_us_" + p) for p in ("hits", "share", "order")])
    e.profile(False)
    for i, p in enumerate(("hits", "share", "order")):
        v = [x[i] for x in phases]
        res["us_" + p] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
    res["ratio_to_plain"] = round(res["ms_median"] / res_plain["ms_median"], 3)
    print(json.dumps(res), flush=True)
    e.close()


if __name__ == "__main__":
    main()
