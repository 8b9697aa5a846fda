#!/usr/bin/env python3
"""niqki_unite at the index shape of bench.py: 100 000 genomes of random cells, S = 15, W = 12, inserted on the device.
Every case runs in a child process of its own under its own time limit, one after the other; the first that fails ends
the run.  One JSON line per case:

  runs10, scattered10, giant   three labellings: runs of 10 consecutive genomes; 10 members per label scattered over
              the index (g % (N / 10)); one label of half the genomes plus singletons.  Per repeat (a fresh index each
              time: the call changes it): the host's preparation and the minimum pass (stats unite_us_prepare /
              unite_us_min, profiling on; the pass by HIP events) and the call's wall time.  A few labels are checked
              against the minimum numpy takes over their members' sketches, read before the call.
  retain      yardstick (a): niqki_retain of every tenth genome on the same index (stat retain_us_compact): it reads
              the same store once and writes a store of the runs10 / scattered10 size
  copy        yardstick (b), same events: a device-to-device hipMemcpy2DAsync of a buffer with the store's shape

The three ratios min / retain compaction and min / copy are printed last, from the best of each.

    python tools/bench_unite.py [--genomes 100000] [--repeats 3] [--out FILE]
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
S, W = 15, 12
F = 1 << S
LABELLINGS = ("runs10", "scattered10", "giant")


def make_index(args):
    import torch
    import niqki_amd
    from niqki_amd import capi
    g = torch.Generator(device="cuda")
    g.manual_seed(args.seed)
    e = niqki_amd.Engine(K=31, S=S, W=W, H=4, min_score_value=capi.min_score(0.1, S))
    e.set_stream(torch.cuda.current_stream().cuda_stream)
    for a in range(0, args.genomes, 4096):
        n = min(4096, args.genomes - a)
        e.insert_dev(torch.randint(0, 1 << W, (n, F), dtype=torch.int32, device="cuda", generator=g), n)
    torch.cuda.synchronize()
    return e


def labelling(np, kind, N):
    g = np.arange(N, dtype=np.uint32)
    if kind == "runs10":
        return g // 10
    if kind == "scattered10":
        return g % (N // 10)
    half = np.random.default_rng(1).permutation(N)[:N // 2]
    lab = g.copy()
    lab[half] = N + 1
    return lab


def case_unite(args, kind):
    import numpy as np
    import torch
    N = args.genomes
    lab = labelling(np, kind, N)
    sizes = np.unique(lab, return_counts=True)[1]
    res = {"case": kind, "genomes": N, "labels": int(sizes.size), "largest_label": int(sizes.max()),
           "prepare_ms": [], "min_ms": [], "call_wall_ms": []}
    for rep in range(args.repeats + 1):                        # the first round warms up and is not reported
        e = make_index(args)
        # labels 0 and 1 (by first appearance: those of genomes 0 and the first genome outside label 0), at most 64 members
        first = [0, int(np.nonzero(lab != lab[0])[0][0])]
        expect = []
        for f0 in first:
            members = np.nonzero(lab == lab[f0])[0][:64]
            whole = members.size == int((lab == lab[f0]).sum())
            expect.append((whole, np.stack([e.get_sketches(int(m), 1)[0] for m in members]).min(axis=0)))
        e.profile(True)
        t = time.time()
        n_labels, ids = e.unite(lab)
        wall = (time.time() - t) * 1e3
        prepare, mn = e.stat("unite_us_prepare") / 1e3, e.stat("unite_us_min") / 1e3
        e.profile(False)
        assert n_labels == res["labels"] == e.n_genomes and ids[first[0]] == 0 and ids[first[1]] == 1
        got = e.get_sketches(0, 2)
        for (whole, exp), row in zip(expect, got):
            assert np.array_equal(row, exp) if whole else (row <= exp).all()
        if rep:
            res["prepare_ms"].append(round(prepare, 3))
            res["min_ms"].append(round(mn, 3))
            res["call_wall_ms"].append(round(wall, 3))
        res["store_bytes_after"] = int(e.stat("store_bytes"))
        e.close()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    res["bytes_read"] = F * N * 2
    res["bytes_written"] = F * res["labels"] * 2
    res["min_read_GBps"] = round(res["bytes_read"] / min(res["min_ms"]) / 1e6, 1)
    return res


def case_retain(args):
    import numpy as np
    import torch
    N = args.genomes
    keep = np.arange(N) % 10 == 0
    res = {"case": "retain", "genomes": N, "kept": int(keep.sum()), "compact_ms": []}
    for rep in range(args.repeats + 1):
        e = make_index(args)
        e.profile(True)
        e.retain(keep)
        compact = e.stat("retain_us_compact") / 1e3
        e.profile(False)
        if rep:
            res["compact_ms"].append(round(compact, 3))
        e.close()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    return res


def case_copy(args):
    import torch
    import bench_retain
    pitch = (args.genomes + 63) // 64 * 64
    return {"case": "copy", "genomes": args.genomes, "store_copy_ms": bench_retain.store_copy_ms(torch, args.genomes, pitch, args.repeats),
            "bytes_read": F * args.genomes * 2, "bytes_written": F * args.genomes * 2}


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
        res = case_retain(args) if args.case == "retain" else case_copy(args) if args.case == "copy" else case_unite(args, args.case)
        print(json.dumps(res), flush=True)
        return 0
    lines, best = [], {}
    for case in LABELLINGS + ("retain", "copy"):
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--case", case,
               "--genomes", str(args.genomes), "--repeats", str(args.repeats), "--seed", str(args.seed)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:                                  # nothing more on the GPU after a failure
            print("case %s failed with exit status %d\n%s" % (case, r.returncode, r.stderr[-2000:]), flush=True)
            return 1
        lines.append(r.stdout.strip().split("\n")[-1])
        print(lines[-1], flush=True)
        res = json.loads(lines[-1])
        best[case] = min(res["min_ms"] if case in LABELLINGS else res["compact_ms"] if case == "retain" else res["store_copy_ms"])
    ratios = {"case": "ratios", "min_over_retain_compact": {k: round(best[k] / best["retain"], 3) for k in LABELLINGS},
              "min_over_store_copy": {k: round(best[k] / best["copy"], 3) for k in LABELLINGS}}
    lines.append(json.dumps(ratios))
    print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
