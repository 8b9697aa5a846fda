#!/usr/bin/env python3
"""The taxon tally beside niqki_query_lca at the reads shape of BASELINE.json configs[4]: one batch of 65 536 reads of
150 bases against the 10 000-genome index of tools/bench_lca.py, its five-level taxonomy of 11 111 taxa, min_score 2,
top_permille 100, everything in device memory.  JSON lines:

  lca         niqki_query_lca of the batch without and with an open tally, alternating on the same handle, by HIP
              events, medians of --repeats: the call without a tally is code the tally leaves untouched, so it is the
              yardstick; "added_ms" = the difference of the medians
  phases      while profiling is on: stats tally_us_add of the LCA call and tally_us_clade of one niqki_tally_read
  totals      the totals of one batch, and the largest direct count (how skewed the batch is)
Both cases twice: the five-level taxonomy, and "skewed": genome_taxon all one taxon, so that every classified row hits
one accumulator -- the case the on-chip combine of tally_rows_kernel exists for.

    python tools/bench_tally.py [--genomes 10000] [--batch 65536] [--repeats 7] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_lca import events_ms, five_levels, median  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", type=int, default=10000)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--len", type=int, default=5_000_000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--min-score", type=int, default=2)
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

    # the index and the reads of tools/bench_lca.py
    GB = 256
    seqbuf = torch.zeros(GB * L + 64, dtype=torch.uint8, device=dev)
    skbuf = torch.empty((GB, F), dtype=torch.int32, device=dev)
    for g0 in range(0, N, GB):
        n = min(GB, N - g0)
        g = np.arange(g0, g0 + n)
        e.synth_dev(7, dev_u32(g // 100), dev_u32(g % 100), dev_u32(np.where(g % 100 == 0, 0, 16 + (g % 100) * 8)), n, L, L, seqbuf)
        e.sketch_dev(seqbuf, torch.from_numpy(np.arange(n + 1, dtype=np.int64) * L).to(dev), n, skbuf)
        e.insert_dev(skbuf, n)
    e.build()
    e.synchronize()
    del seqbuf, skbuf
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
    e.set_option("min_score", args.min_score)
    out = [torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(4)]

    def lca():
        e.query_lca_dev(sk, B, 100, *out)

    gt, parent = five_levels(N)
    for case, genome_taxon in (("five_levels", gt), ("skewed", np.full(N, 4321, np.uint32))):
        e.set_taxonomy(genome_taxon, parent)
        lca()                                                 # warm-up without a tally ...
        e.tally_begin()
        lca()                                                 # ... and with one
        totals = e.tally_read_dev()
        direct = e.tally_read()[0]
        emit({"case": "totals", "taxonomy": case, "taxa": e.stat("taxa"), "min_score": args.min_score, **totals, "largest_direct": int(direct.max())})
        without, with_tally = [], []
        for _ in range(args.repeats):                         # alternating: both see the same neighbours on the machine
            e.tally_end()
            without.append(events_ms(torch, lca))
            e.tally_begin()
            with_tally.append(events_ms(torch, lca))
        emit({"case": "lca", "taxonomy": case, "without_tally_ms": [round(x, 3) for x in without], "with_tally_ms": [round(x, 3) for x in with_tally],
              "median_without_ms": round(median(without), 3), "median_with_ms": round(median(with_tally), 3),
              "added_ms": round(median(with_tally) - median(without), 3)})
        e.profile(True)
        add_us, clade_us, fold_us = [], [], []
        for _ in range(args.repeats):
            e.tally_begin()
            lca()
            add_us.append(e.stat("tally_us_add"))
            fold_us.append(e.stat("lca_us_fold"))
            e.tally_read_dev()
            clade_us.append(e.stat("tally_us_clade"))
        e.profile(False)
        emit({"case": "phases", "taxonomy": case, "tally_us_add": add_us, "tally_us_clade": clade_us, "lca_us_fold": fold_us,
              "median_us_add": median(add_us), "median_us_clade": median(clade_us), "median_us_fold": median(fold_us)})
        e.tally_end()
    e.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
