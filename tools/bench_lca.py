#!/usr/bin/env python3
"""niqki_query_lca at the reads shape of BASELINE.json configs[4]: one batch of 65 536 reads of 150 bases against the
10 000-genome index of tools/bench_reads.py (K = 31, S = 12, W = 10, -J 0.1), a synthetic five-level taxonomy (genome,
group of 10, family of 100, order of 1000, one root) and top_permille 100.  Everything in device memory.  JSON lines:

  index       genomes, the time to build the index, taxa and depth of the taxonomy, the time of niqki_set_taxonomy
  baseline    a plain niqki_query of the batch (top_k = 0) on the same handle, by HIP events: the yardstick is the
              query itself, an existing call whose code the LCA calls leave untouched -- never the new call against
              itself
  lca         niqki_query_lca of the same batch, by HIP events; queries without a hit, without a common taxon, folded
              by the whole workgroup, splits; taxa by depth; "ratio" = median lca / median baseline
  phases      further calls while profiling is on: stats lca_us_hits / lca_us_fold, the median of each, at option
              "lca_wave_cap" 1024 and 64 and at top_permille 100 and 1000 (every hit considered)
At -J 0.1 (410 of 4096 slots) no 150-base read has a hit -- its 120 k-mers cannot share that many slots -- so the three
cases are repeated at low thresholds (--also-min-score, slots; 2 is the threshold of tests/test_gpu_reads_config.py),
where a read's list holds up to a few hundred genomes.

    python tools/bench_lca.py [--genomes 10000] [--batch 65536] [--repeats 7] [--also-min-score 4 2] [--out FILE]
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


def five_levels(n):
    """(genome_taxon, parent): genome g is taxon g under group g // 10 under family g // 100 under order g // 1000
    under the root"""
    import numpy as np
    g = np.arange(n)
    n10, n100, n1000 = (n + 9) // 10, (n + 99) // 100, (n + 999) // 1000
    o10, o100, o1000 = n, n + n10, n + n10 + n100
    root = o1000 + n1000
    parent = np.empty(root + 1, np.uint32)
    parent[:n] = o10 + g // 10
    parent[o10:o100] = o100 + np.arange(n10) // 10
    parent[o100:o1000] = o1000 + np.arange(n100) // 10
    parent[o1000:root] = root
    parent[root] = root
    return g.astype(np.uint32), parent


def events_ms(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", type=int, default=10000)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--len", type=int, default=5_000_000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--also-min-score", type=int, nargs="*", default=[4, 2],
                    help="thresholds (slots) to measure beside the configuration's -J 0.1, which no 150-base read reaches")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import niqki_amd
    K, S, W, H, J = 31, 12, 10, 4, 0.1
    F = 1 << S
    dev = torch.device("cuda", 0)
    e = niqki_amd.Engine(K=K, S=S, W=W, H=H, J=J, device=0)
    e.set_stream(torch.cuda.current_stream().cuda_stream)
    N, L, B = args.genomes, args.len, args.batch
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    def dev_u32(a):
        return torch.from_numpy(a.astype(np.int64)).to(torch.int32).to(dev)

    # the index and the reads of tools/bench_reads.py
    GB = 256
    seqbuf = torch.zeros(GB * L + 64, dtype=torch.uint8, device=dev)
    skbuf = torch.empty((GB, F), dtype=torch.int32, device=dev)
    t0 = time.perf_counter()
    for g0 in range(0, N, GB):
        n = min(GB, N - g0)
        g = np.arange(g0, g0 + n)
        e.synth_dev(7, dev_u32(g // 100), dev_u32(g % 100), dev_u32(np.where(g % 100 == 0, 0, 16 + (g % 100) * 8)), n, L, L, seqbuf)
        e.sketch_dev(seqbuf, torch.from_numpy(np.arange(n + 1, dtype=np.int64) * L).to(dev), n, skbuf)
        e.insert_dev(skbuf, n)
    e.build()
    e.synchronize()
    t_index = time.perf_counter() - t0
    del seqbuf, skbuf
    gt, parent = five_levels(N)
    t0 = time.perf_counter()
    e.set_taxonomy(gt, parent)
    t_tax = time.perf_counter() - t0
    emit({"case": "index", "genomes": N, "index_build_s": round(t_index, 2), "taxa": e.stat("taxa"), "taxonomy_depth": e.stat("taxonomy_depth"),
          "set_taxonomy_s": round(t_tax, 4)})
    rng = np.random.default_rng(5)
    src = [niqki_amd.synth_genome_host(7, g // 100, g % 100, 0 if g % 100 == 0 else 16 + (g % 100) * 8, 200_000) for g in range(64)]
    which = rng.integers(0, 64, B)
    start = rng.integers(0, 200_000 - 150, B)
    reads = np.stack([src[w][s:s + 150] for w, s in zip(which[:4096], start[:4096])])
    reads = np.tile(reads, (B // 4096 + 1, 1))[:B].copy()
    sub = rng.random((B, 150)) < 0.01
    reads[sub] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(sub.sum()))]
    d_reads = torch.cat([torch.from_numpy(reads.reshape(-1)).to(dev), torch.zeros(64, dtype=torch.uint8, device=dev)])
    ro = torch.from_numpy(np.arange(B + 1, dtype=np.int64) * 150).to(dev)
    sk = torch.empty((B, F), dtype=torch.int32, device=dev)
    e.set_option("record_len_hint", 150)
    e.sketch_dev(d_reads, ro, B, sk)
    e.synchronize()

    out = [torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(4)]
    depth_of = np.zeros(parent.size, np.int64)
    for t in range(parent.size - 2, -1, -1):                  # (a parent's id is above its children's)
        depth_of[t] = depth_of[parent[t]] + 1
    h_sk = sk.cpu().numpy()

    def measure(min_score):
        """the batch at one threshold: the plain query and the LCA query in turn, then the phases"""
        e.set_option("min_score", min_score)
        e.set_option("lca_wave_cap", 1024)
        # the full lists once through host memory (that path checks the capacity), for the size of the device arrays
        total = int(e.query(h_sk, capacity=B * 64)[0][B])
        cap = max(total, 1)
        ho = torch.zeros(B + 1, dtype=torch.int64, device=dev)
        hc = torch.zeros(cap, dtype=torch.int32, device=dev)
        hg = torch.zeros(cap, dtype=torch.int32, device=dev)

        def plain():
            e.query_dev(sk, B, ho, hc, hg, cap)

        def lca(p=100):
            e.query_lca_dev(sk, B, p, *out)

        plain()                                               # warm-up: code objects, workspace allocations
        lca()
        torch.cuda.synchronize()
        base, wall = [], []
        for _ in range(args.repeats):                         # alternating: both see the same neighbours on the machine
            base.append(events_ms(torch, plain))
            wall.append(events_ms(torch, lca))
        taxon, considered = (out[k].cpu().numpy().view(np.uint32) for k in (0, 3))
        some = taxon != 0xFFFFFFFF
        emit({"case": "baseline", "min_score": min_score, "query_ms": [round(x, 3) for x in base], "median_ms": round(median(base), 3),
              "hits": total})
        emit({"case": "lca", "min_score": min_score, "top_permille": 100, "lca_ms": [round(x, 3) for x in wall],
              "median_ms": round(median(wall), 3), "no_hit": int((considered == 0).sum()), "no_common": e.stat("lca_no_common"),
              "long_lists": e.stat("lca_long_lists"), "splits": e.stat("lca_splits"), "considered_mean": round(float(considered.mean()), 2),
              "considered_max": int(considered.max()), "taxa_by_depth": np.bincount(depth_of[taxon[some]], minlength=5).tolist(),
              "ratio": round(median(wall) / median(base), 4)})
        e.profile(True)
        for cap_w, p in ((1024, 100), (64, 100), (1024, 1000), (64, 1000)):
            e.set_option("lca_wave_cap", cap_w)
            hits_us, fold_us = [], []
            for _ in range(args.repeats):
                lca(p)
                torch.cuda.synchronize()
                hits_us.append(e.stat("lca_us_hits"))
                fold_us.append(e.stat("lca_us_fold"))
            emit({"case": "phases", "min_score": min_score, "lca_wave_cap": cap_w, "top_permille": p, "long_lists": e.stat("lca_long_lists"),
                  "no_common": e.stat("lca_no_common"), "lca_us_hits": hits_us, "lca_us_fold": fold_us, "median_us_hits": median(hits_us),
                  "median_us_fold": median(fold_us)})
        e.profile(False)

    for ms in [e.min_score] + args.also_min_score:            # -J 0.1 of the configuration first
        measure(ms)
    e.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
