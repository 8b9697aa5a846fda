#!/usr/bin/env python3
"""niqki_registers at the index shape of bench.py: 100 000 genomes of random cells, S = 15, W = 12, H = 4, inserted on
the device.  Every case runs in a child process of its own under its own time limit, one after the other; the first
that fails ends the run.  One JSON line per case:

  store       the store pass over all genomes into a device array (stat registers_us_store, profiling on: HIP events
              around the kernel) and the call's wall time; the histograms of a few genomes are checked against numpy
              over their sketches
  rows        the row pass over a batch of 4096 query sketches on the device (stat registers_us_rows)
  copy        the yardstick, same events: a device-to-device hipMemcpy2DAsync of a buffer with the store's shape -- it
              reads the same bytes (and writes as many, which the store pass does not)

The ratio store pass / copy is printed last, from the best of each.

    python tools/bench_sizes.py [--genomes 100000] [--repeats 3] [--out FILE]
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
S, W, H = 15, 12, 4
F = 1 << S
B = (1 << H) + 1


def make_index(args):
    import torch
    import niqki_amd
    from niqki_amd import capi
    g = torch.Generator(device="cuda")
    g.manual_seed(args.seed)
    e = niqki_amd.Engine(K=31, S=S, W=W, H=H, min_score_value=capi.min_score(0.1, S))
    e.set_stream(torch.cuda.current_stream().cuda_stream)
    for a in range(0, args.genomes, 4096):
        n = min(4096, args.genomes - a)
        e.insert_dev(torch.randint(0, 1 << W, (n, F), dtype=torch.int32, device="cuda", generator=g), n)
    torch.cuda.synchronize()
    return e


def hist_numpy(np, sk):
    return np.stack([np.bincount(np.where(r >= 0, r >> (W - H), 1 << H), minlength=B) for r in sk]).astype(np.uint32)


def case_store(args):
    import numpy as np
    import torch
    N = args.genomes
    e = make_index(args)
    hist = torch.empty(N * B, dtype=torch.int32, device="cuda")
    res = {"case": "store", "genomes": N, "store_ms": [], "call_wall_ms": [], "bytes_read": F * N * 2}
    e.profile(True)
    for rep in range(args.repeats + 1):                        # the first round warms up and is not reported
        torch.cuda.synchronize()
        t = time.time()
        e.registers_dev(hist, 0, N)
        torch.cuda.synchronize()
        if rep:
            res["call_wall_ms"].append(round((time.time() - t) * 1e3, 3))
            res["store_ms"].append(round(e.stat("registers_us_store") / 1e3, 3))
    e.profile(False)
    got = hist.cpu().numpy().view(np.uint32).reshape(N, B)
    assert (got.sum(axis=1) == F).all()
    for g in sorted({0, 63, 64, N // 2, N - 1}):
        assert np.array_equal(got[g], hist_numpy(np, e.get_sketches(g, 1))[0]), g
    res["store_read_GBps"] = round(res["bytes_read"] / min(res["store_ms"]) / 1e6, 1)
    e.close()
    return res


def case_rows(args):
    import numpy as np
    import torch
    n = 4096
    e = make_index(argparse.Namespace(genomes=64, seed=args.seed))
    g = torch.Generator(device="cuda")
    g.manual_seed(args.seed + 1)
    sk = torch.randint(-1, 1 << W, (n, F), dtype=torch.int32, device="cuda", generator=g)
    hist = torch.empty(n * B, dtype=torch.int32, device="cuda")
    res = {"case": "rows", "sketches": n, "rows_ms": [], "bytes_read": F * n * 4}
    e.profile(True)
    for rep in range(args.repeats + 1):
        torch.cuda.synchronize()
        e.registers_dev(hist, sketches=sk, n=n)
        torch.cuda.synchronize()
        if rep:
            res["rows_ms"].append(round(e.stat("registers_us_rows") / 1e3, 3))
    e.profile(False)
    got = hist.cpu().numpy().view(np.uint32).reshape(n, B)
    assert np.array_equal(got[:8], hist_numpy(np, sk[:8].cpu().numpy()))
    res["rows_read_GBps"] = round(res["bytes_read"] / min(res["rows_ms"]) / 1e6, 1)
    e.close()
    return res


def case_copy(args):
    import torch
    import bench_retain
    pitch = (args.genomes + 63) // 64 * 64
    return {"case": "copy", "genomes": args.genomes, "store_copy_ms": bench_retain.store_copy_ms(torch, args.genomes, pitch, args.repeats),
            "bytes_read": F * args.genomes * 2, "bytes_written": F * args.genomes * 2}


CASES = {"store": case_store, "rows": case_rows, "copy": case_copy}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", type=int, default=100000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per case")
    ap.add_argument("--out", default=None)
    ap.add_argument("--case", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.case:
        print(json.dumps(CASES[args.case](args)), flush=True)
        return 0
    lines, best = [], {}
    for case in CASES:
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--case", case,
               "--genomes", str(args.genomes), "--repeats", str(args.repeats), "--seed", str(args.seed)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:                                  # nothing more on the GPU after a failure
            print("case %s failed with exit status %d\n%s" % (case, r.returncode, r.stderr[-2000:]), flush=True)
            return 1
        lines.append(r.stdout.strip().split("\n")[-1])
        print(lines[-1], flush=True)
        res = json.loads(lines[-1])
        best[case] = min(res["store_ms"] if case == "store" else res["rows_ms"] if case == "rows" else res["store_copy_ms"])
    lines.append(json.dumps({"case": "ratios", "store_pass_over_store_copy": round(best["store"] / best["copy"], 3)}))
    print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
