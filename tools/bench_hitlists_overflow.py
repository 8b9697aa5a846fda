#!/usr/bin/env python3
"""Hit lists against counter rows when queries overflow hit_list_cap, at the index shape of bench.py: 100 000 genomes
(two striped tiles), S = 15, W = 12, batches of 4096 query sketches on the device (synthetic families of sketches, as
tools/bench_topk.py makes them).  For each case -- min_score and hit_list_cap -- the same batch runs with option
hit_lists = 1 and 0 (0: the counter-row path every query of such an index took before hit lists had several tiles); one
JSON line per run: the hits phase (kernel class "hits"), the gather launch, the whole call, and how many queries have
more hits than the cap.  Both forms must give the same bytes (checked).

    python tools/bench_hitlists_overflow.py [--genomes 100000] [--nq 4096] [--steps 3]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", type=int, default=100000)
    ap.add_argument("--nq", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=7)
    args = ap.parse_args()
    import torch
    import niqki_amd
    from niqki_amd import capi

    K, S, W, H = 31, 15, 12, 4
    F, N, nq = 1 << S, args.genomes, args.nq
    dev = torch.device("cuda")
    g = torch.Generator(device=dev)
    g.manual_seed(args.seed)
    n_fam = 500
    fam = torch.randint(0, 1 << W, (n_fam, F), dtype=torch.int32, device=dev, generator=g)

    def members(ids, rate):   # family sketches with a fraction `rate` of their cells replaced
        sk = fam[ids].clone()
        m = torch.rand(sk.shape, device=dev, generator=g) < rate
        sk[m] = torch.randint(0, 1 << W, (int(m.sum().item()),), dtype=torch.int32, device=dev, generator=g)
        return sk

    e = niqki_amd.Engine(K=K, S=S, W=W, H=H, min_score_value=0)
    e.set_stream(torch.cuda.current_stream().cuda_stream)
    for a in range(0, N, 4096):
        n = min(4096, N - a)
        ids = torch.randint(0, n_fam, (n,), device=dev, generator=g)
        rate = 0.2 + 0.7 * torch.rand((n, 1), device=dev, generator=g)
        e.insert_dev(members(ids, rate), n)
    q = members(torch.randint(0, n_fam, (nq,), device=dev, generator=g), 0.5)
    e.build()
    torch.cuda.synchronize()
    print(json.dumps({"genomes": N, "nq": nq, "tiles": e.stat("tiles")}), flush=True)

    def run(min_score, cap, lists):
        e.set_option("min_score", min_score)
        e.set_option("hit_list_cap", cap)
        e.set_option("hit_lists", lists)
        off = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
        one = torch.zeros(1, dtype=torch.int32, device=dev)
        e.query_dev(q, nq, off, one, one, 0)       # sizes first (device outputs: nothing written)
        total = int(off[-1].item())
        hc = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
        hg = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
        e.query_dev(q, nq, off, hc, hg, total)      # warm-up (workspace allocations)
        torch.cuda.synchronize()
        e.profile(True)
        e.profile_reset()
        t = time.time()
        for _ in range(args.steps):
            e.query_dev(q, nq, off, hc, hg, total)
        torch.cuda.synchronize()
        wall = (time.time() - t) / args.steps * 1e3
        hits_ms, n_hits = e.profile_read(capi.KC_HITS)
        gather_ms, n_g = e.profile_read(capi.KC_GATHER)
        e.profile(False)
        sizes = (off[1:] - off[:-1]).cpu()
        res = {"min_score": min_score, "hit_list_cap": cap, "hit_lists": lists, "form": e.stat("last_hits_form"),
               "query_ms": round(wall, 3), "hits_ms": round(hits_ms / max(n_hits, 1), 3),
               "gather_ms": round(gather_ms / max(n_g, 1), 3), "total_hits": total,
               "queries_over_cap": int((sizes > cap).sum().item()), "max_hits": int(sizes.max().item())}
        print(json.dumps(res), flush=True)
        return off.cpu(), hc[:total].cpu(), hg[:total].cpu()

    same = True
    for ms, cap in ((capi.min_score(0.1, S), 256), (capi.min_score(0.1, S), 4), (2500, 256), (1500, 256), (0, 256)):
        a = run(ms, cap, 1)
        b = run(ms, cap, 0)
        same = same and all(torch.equal(x, y) for x, y in zip(a, b))
    print(json.dumps({"same_bytes": same}), flush=True)
    e.close()
    if not same:
        sys.exit(1)


if __name__ == "__main__":
    main()
