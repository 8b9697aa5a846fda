#!/usr/bin/env python3
"""The short-read sketch kernel alone (nq::sketch_reads_kernel: ~120 k-mers, then ~420 densification passes per
150-base read, src/niqki_index.cpp:313-331) on configs[4]'s reads, S=12 W=10: ms per 65 536 reads (best of --reps)
and a CRC-32 of all the sketches of the last batch.  NIQKI_EXP_LIB=path times another build of the library, so two
builds can be compared.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1 << 20)
    ap.add_argument("--len", type=int, default=150)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("-S", type=int, default=12)
    ap.add_argument("-W", type=int, default=10)
    args = ap.parse_args()
    import torch
    import bench
    import niqki_amd
    if os.environ.get("NIQKI_EXP_LIB"):      # A/B against another build of the library (tools/bin/, never the product's path)
        from niqki_amd import capi
        capi._LIB = os.path.abspath(os.environ["NIQKI_EXP_LIB"])
    K, S, W, H = 31, args.S, args.W, 4
    F, L, RL, RB, NR = 1 << S, 5_000_000, args.len, 65536, args.reads
    dev = torch.device("cuda", 0)
    t32 = lambda a: torch.from_numpy(np.asarray(a).astype(np.int64)).to(torch.int32).to(dev)  # noqa: E731
    t64 = lambda a: torch.from_numpy(np.asarray(a).astype(np.int64)).to(dev)  # noqa: E731
    e = niqki_amd.Engine(K=K, S=S, W=W, H=H, J=0.1, device=0)
    e.set_stream(torch.cuda.current_stream().cuda_stream)
    e.set_option("record_len_hint", RL)
    rng = np.random.default_rng(20261003)
    N = 1000
    src_g = rng.integers(0, N, NR)
    src_off = rng.integers(0, L - RL, NR).astype(np.uint64)
    reads = torch.zeros(NR * RL + niqki_amd.SEQ_PAD, dtype=torch.uint8, device=dev)
    CH = 1 << 20
    for a in range(0, NR, CH):
        gch = src_g[a:a + CH]
        fam, mem, rate = bench.genome_spec(gch, N // 100, 100)
        e.synth_reads_dev(20261005, t32(fam), t32(mem), t32(rate), t64(src_off[a:a + CH]), t32(np.arange(a, a + len(gch))),
                          164, len(gch), RL, RL, reads[a * RL:])
    rro = t64(np.arange(RB + 1, dtype=np.int64) * RL)
    rsk = torch.empty((RB, F), dtype=torch.int32, device=dev)
    e.sketch_dev(reads, rro, RB, rsk)
    e.synchronize()
    best = 1e9
    for _ in range(args.reps):
        t0 = time.perf_counter()
        for a in range(0, NR, RB):
            e.sketch_dev(reads[a * RL:], rro, RB, rsk)
        e.synchronize()
        best = min(best, time.perf_counter() - t0)
    print(json.dumps({"reads": NR, "read_len": RL, "S": S, "W": W, "lib": niqki_amd.capi._LIB,
                      "ms_per_65536_reads": best / (NR / RB) * 1e3, "reads_per_s": NR / best,
                      "last_batch_crc32": zlib.crc32(rsk.cpu().numpy().tobytes())}))


if __name__ == "__main__":
    main()
