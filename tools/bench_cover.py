#!/usr/bin/env python3
"""niqki_cover at the index shape of bench.py: 100 000 synthetic genomes in 500 families (members with 20-90 % of their
cells replaced, as tools/bench_selfjoin.py), S = 15, W = 12, -J 0.1, and 4096 queries that are the per-slot minima of
1, 2, 4 and 8 genomes of different families (a quarter each, interleaved).  Everything in device memory.  JSON lines:

  yardstick   a plain niqki_query of the batch with top_k = 1, by HIP events: what one round's hits cost at least, and
              what the parent of niqki_cover can run as well
  rounds      niqki_cover with max_picks = 1 .. --rounds while profiling is on; the call's four phases (stats
              cover_us_hits / _pick / _compact / _finish) are sums over its rounds, so a round's share is the difference
              between consecutive calls.  "active" = the rows the round ran on.
  cover       the unbounded call without profiling: wall time by HIP events, rounds, picks, picks per query kind

    python tools/bench_cover.py [--genomes 100000] [--queries 4096] [--rounds 10] [--repeats 3] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
K, S, W, H = 31, 15, 12, 4
F = 1 << S
N_FAM = 500
MIX = (1, 2, 4, 8)


def make_index(args, torch):
    import niqki_amd
    from niqki_amd import capi
    dev = torch.device("cuda")
    g = torch.Generator(device=dev)
    g.manual_seed(args.seed)
    N = args.genomes
    fam = torch.randint(0, 1 << W, (N_FAM, F), dtype=torch.int32, device=dev, generator=g)
    fam_of = torch.randint(0, N_FAM, (N,), device=dev, generator=g)
    e = niqki_amd.Engine(K=K, S=S, W=W, H=H, min_score_value=capi.min_score(0.1, S))
    e.set_stream(torch.cuda.current_stream().cuda_stream)
    # the queries' genomes: for query i, MIX[i % 4] genomes of different families
    fam_cpu = fam_of.cpu().numpy()
    import numpy as np
    rng = np.random.default_rng(args.seed)
    members = []
    for i in range(args.queries):
        fams = rng.choice(N_FAM, MIX[i % 4], replace=False)
        members.append([int(rng.choice(np.nonzero(fam_cpu == f)[0])) for f in fams])
    wanted = {m: None for ms in members for m in ms}
    for a in range(0, N, 4096):
        n = min(4096, N - a)
        sk = fam[fam_of[a:a + n]].clone()
        m = torch.rand(sk.shape, device=dev, generator=g) < 0.2 + 0.7 * torch.rand((n, 1), device=dev, generator=g)
        sk[m] = torch.randint(0, 1 << W, (int(m.sum().item()),), dtype=torch.int32, device=dev, generator=g)
        e.insert_dev(sk, n)
        for gid in wanted:
            if a <= gid < a + n:
                wanted[gid] = sk[gid - a].clone()
    e.build()
    q = torch.stack([torch.stack([wanted[m] for m in ms]).min(0).values for ms in members]).contiguous()
    torch.cuda.synchronize()
    return e, q


def events_ms(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return round(a.elapsed_time(b), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", type=int, default=100000)
    ap.add_argument("--queries", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    e, q = make_index(args, torch)
    nq = q.shape[0]
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    cap = nq * 64
    ho = torch.zeros(nq + 1, dtype=torch.int64, device="cuda")
    hc, hg, ht = (torch.zeros(cap, dtype=torch.int32, device="cuda") for _ in range(3))
    # yardstick: the query path at top_k = 1
    e.set_option("top_k", 1)
    e.query_dev(q, nq, ho, hc, hg, cap)
    torch.cuda.synchronize()
    yard = [events_ms(torch, lambda: e.query_dev(q, nq, ho, hc, hg, cap)) for _ in range(args.repeats)]
    e.set_option("top_k", 0)
    emit({"case": "yardstick", "genomes": args.genomes, "queries": nq, "query_top1_ms": yard})
    # the unbounded call
    assert e.cover_dev(q, nq, 0, ho, hc, hg, ht, cap) == 0       # warm-up: workspace allocations
    torch.cuda.synchronize()
    wall = [events_ms(torch, lambda: e.cover_dev(q, nq, 0, ho, hc, hg, ht, cap)) for _ in range(args.repeats)]
    off = ho.cpu().numpy()
    n_picks = np.diff(off)
    emit({"case": "cover", "cover_ms": wall, "rounds": e.stat("cover_rounds"), "picks": e.stat("cover_picks"),
          "recount_mismatches": e.stat("cover_recount_mismatches"),
          "mean_picks_by_mixture": {str(m): round(float(n_picks[k::4].mean()), 3) for k, m in enumerate(MIX)}})
    # per round: calls bounded to 1 .. R picks, profiled
    e.profile(True)
    prev = {k: 0.0 for k in ("hits", "pick", "compact", "finish")}
    prev_picks = 0
    for r in range(1, args.rounds + 1):
        assert e.cover_dev(q, nq, r, ho, hc, hg, ht, cap) == 0
        torch.cuda.synchronize()
        if e.stat("cover_rounds") < r:
            break
        us = {k: e.stat("cover_us_" + k) / 1e3 for k in prev}
        picks = e.stat("cover_picks")
        emit({"case": "round", "round": r, "active": int((n_picks >= r - 1).sum()) if r > 1 else nq, "picks": picks - prev_picks,
              "hits_ms": round(us["hits"] - prev["hits"], 3), "pick_ms": round(us["pick"] - prev["pick"], 3),
              "compact_ms": round(us["compact"] - prev["compact"], 3), "finish_ms_of_the_call": round(us["finish"], 3)})
        prev, prev_picks = us, picks
    e.profile(False)
    e.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
