#!/usr/bin/env python3
"""Top-k queries (niqki_params.top_k) at the index shape of bench.py: 100 000 genomes, S = 15, W = 12, batches of
4096 query sketches on the device.  The index is made of synthetic sketches (families of related genomes, made and
inserted on the device: the hits phase depends on the counter rows, not on where the sketches came from).  Prints one
JSON line per case: the hits phase (kernel class "hits") and the whole niqki_query call per batch, top-k 10 against
the existing path at min_score 0 (-J 0) and at the default -J 0.1, and the HBM bytes per query the threshold / select
passes read.

    python tools/bench_topk.py [--genomes 100000] [--nq 4096] [--steps 3] [--k 10]
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
    ap.add_argument("--k", type=int, default=10)
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
    t0 = time.time()
    for a in range(0, N, 4096):
        n = min(4096, N - a)
        ids = torch.randint(0, n_fam, (n,), device=dev, generator=g)
        rate = 0.2 + 0.7 * torch.rand((n, 1), device=dev, generator=g)
        sk = members(ids, rate)
        e.insert_dev(sk, n)
    q = members(torch.randint(0, n_fam, (nq,), device=dev, generator=g), 0.5)
    e.build()
    torch.cuda.synchronize()
    build_s = time.time() - t0
    stride = capi.row_stride(N)
    ms_default = capi.min_score(0.1, S)

    def case(min_score, k):
        e.set_option("min_score", min_score)
        e.set_option("top_k", k)
        cap = nq * min(k, N) if k else None
        res = {"min_score": min_score, "top_k": k}
        try:
            if cap is None:   # the existing path: the batch's hits counted first (device outputs: nothing written)
                off = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
                one = torch.zeros(1, dtype=torch.int32, device=dev)
                e.query_dev(q, nq, off, one, one, 0)
                cap = int(off[-1].item())
            hc = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
            hg = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
            off = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
            e.query_dev(q, nq, off, hc, hg, cap)       # warm-up (workspace allocations)
            torch.cuda.synchronize()
            e.profile(True)
            e.profile_reset()
            t = time.time()
            for _ in range(args.steps):
                e.query_dev(q, nq, off, hc, hg, cap)
            torch.cuda.synchronize()
            wall = (time.time() - t) / args.steps * 1e3
            hits_ms, n_hits = e.profile_read(capi.KC_HITS)
            gather_ms, n_g = e.profile_read(capi.KC_GATHER)
            e.profile(False)
            res.update(query_ms=round(wall, 3), hits_ms=round(hits_ms / max(n_hits, 1), 3),
                       gather_ms=round(gather_ms / max(n_g, 1), 3), total_hits=int(off[-1].item()),
                       output_bytes=int(off[-1].item()) * 8 * 2)   # hit arrays + the sort's scratch of the same size
        except Exception as ex:   # (the existing path at -J 0 may not get its memory)
            res["error"] = str(ex)[:200]
        print(json.dumps(res), flush=True)
        return res

    row = stride * 2
    print(json.dumps({"genomes": N, "nq": nq, "S": S, "W": W, "build_s": round(build_s, 1), "row_bytes": row,
                      "hits_path_reads_per_query": 2 * row,
                      "select_reads_per_query": {"n <= k": 2 * row, "n > k": 3 * row}}), flush=True)
    case(0, args.k)
    case(0, 0)
    case(ms_default, args.k)
    case(ms_default, 0)
    e.close()


if __name__ == "__main__":
    main()
