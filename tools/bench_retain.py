#!/usr/bin/env python3
"""niqki_retain at the index shape of bench.py: 100 000 synthetic genomes, S = 15, W = 12, -J 0.1 (the index of
tools/bench_selfjoin.py: families of related genomes, made and inserted on the device).  Every case runs in a child
process of its own under its own time limit, one after the other; the first that fails ends the run.  One JSON line
per case:

  derep, half, most   three keep sets: the representatives niqki_dereplicate gives at the threshold, every second
              genome, all but 1 %.  Per repeat (a fresh index each time: the call changes it), by HIP events: the rank
              pass and the compaction (stats retain_us_rank / retain_us_compact, profiling on) and the rebuild that the
              next query triggers (the build kernel class of the profile); the call's wall time beside them.
              Yardstick (a), same process, same events: a device-to-device hipMemcpy2DAsync of a buffer with the old
              store's shape (rows of `genomes` cells, the store's pitch) -- what the store's growth does, and at least
              the bytes the compaction moves.
  host        yardstick (b), the only path without the call: niqki_get_sketches to the host and niqki_insert into a
              second handle, on a SLICE of --slice genomes; "extrapolated_s" is that time x genomes / slice -- an
              extrapolation, not a measurement
  paged       a paged handle of --paged genomes (resident_mib 1024, the store in page-locked host memory): the wall time
              of a call that keeps every second genome -- one pass of the host over the store

    python tools/bench_retain.py [--genomes 100000] [--slice 4096] [--paged 20000] [--repeats 3] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
F = 1 << 15


def hip_runtime():
    """the HIP runtime this process has loaded already (PyTorch's)"""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return ctypes.CDLL(line.split()[-1])
    raise RuntimeError("no HIP runtime loaded")


def events_ms(torch, fn, repeats):
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(round(a.elapsed_time(b), 3))
    return out


def store_copy_ms(torch, n, pitch_cells, repeats):
    """hipMemcpy2DAsync, device to device, F rows of n cells: source rows pitch_cells apart, destination rows
    round-up-64(n) apart (reserve_store's copy)"""
    hip = hip_runtime()
    hip.hipMemcpy2DAsync.restype = ctypes.c_int
    hip.hipMemcpy2DAsync.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t,
                                     ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    dst_cells = (n + 63) // 64 * 64
    src = torch.zeros((F, pitch_cells), dtype=torch.int16, device="cuda")
    dst = torch.empty((F, dst_cells), dtype=torch.int16, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def copy():
        rc = hip.hipMemcpy2DAsync(dst.data_ptr(), dst_cells * 2, src.data_ptr(), pitch_cells * 2, n * 2, F, 3, stream)   # 3 = device to device
        assert rc == 0, rc
    copy()
    torch.cuda.synchronize()
    ms = events_ms(torch, copy, repeats)
    del src, dst
    torch.cuda.empty_cache()
    return ms


def keep_set(np, e, kind, N):
    if kind == "derep":
        labels, _ = e.dereplicate(e.min_score)
        return labels == np.arange(N)
    if kind == "half":
        return np.arange(N) % 2 == 0
    return np.random.default_rng(1).random(N) >= 0.01


def case_retain(args, kind):
    import numpy as np
    import torch
    from niqki_amd import capi
    import bench_selfjoin
    res = {"case": kind, "genomes": args.genomes, "rank_ms": [], "compact_ms": [], "rebuild_ms": [], "call_wall_ms": []}
    for rep in range(args.repeats + 1):                        # the first round warms up and is not reported
        e, N = bench_selfjoin.make_index(args, "families")
        q = e.get_sketches(0, 8)
        e.query(q)
        keep = keep_set(np, e, kind, N)
        pitch = e.stat("store_bytes") // (2 * F)
        if rep == 0:
            res["kept"] = int(keep.sum())
            res["store_pitch_cells"] = int(pitch)
            res["store_copy_ms"] = store_copy_ms(torch, N, int(pitch), args.repeats)
        first = np.nonzero(keep)[0][:8]
        expect = np.stack([e.get_sketches(int(g), 1)[0] for g in first])
        e.profile(True)
        t = time.time()
        n_kept, _ = e.retain(keep)
        wall = (time.time() - t) * 1e3
        rank, compact = e.stat("retain_us_rank") / 1e3, e.stat("retain_us_compact") / 1e3
        e.profile_reset()
        e.query(q)                                             # the rebuild of what is left
        torch.cuda.synchronize()
        rebuild = e.profile_read(capi.KC_BUILD)[0]
        e.profile(False)
        assert n_kept == res["kept"] and e.n_genomes == n_kept
        assert np.array_equal(e.get_sketches(0, first.size), expect)
        if rep:
            res["rank_ms"].append(round(rank, 3))
            res["compact_ms"].append(round(compact, 3))
            res["rebuild_ms"].append(round(rebuild, 3))
            res["call_wall_ms"].append(round(wall, 3))
        res["store_bytes_after"] = int(e.stat("store_bytes"))
        e.close()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    best = min(res["compact_ms"])
    res["bytes_written"] = F * res["kept"] * 2
    res["old_store_bytes"] = F * args.genomes * 2
    res["compact_written_GBps"] = round(res["bytes_written"] / best / 1e6, 1)
    res["compact_over_store_copy"] = round(best / min(res["store_copy_ms"]), 3)
    return res


def case_host(args):
    import numpy as np
    import niqki_amd
    import bench_selfjoin
    e, N = bench_selfjoin.make_index(args, "families")
    n = min(args.slice, N)
    second = niqki_amd.Engine(K=31, S=15, W=12, H=4, min_score_value=e.min_score)
    second.insert(e.get_sketches(0, 64))                       # warm-up: staging buffers of both handles
    times = []
    for _ in range(args.repeats):
        t = time.time()
        sk = e.get_sketches(0, n)
        second.insert(sk)
        second.synchronize()
        times.append(time.time() - t)
    best = min(times)
    e.close()
    second.close()
    return {"case": "host", "genomes": N, "slice": n, "slice_s": [round(x, 4) for x in times],
            "bytes_through_the_host": int(n) * F * 4 * 2, "extrapolated_s": round(best * N / n, 2),
            "note": "EXTRAPOLATED: extrapolated_s = the best slice_s x genomes / slice"}


def case_paged(args):
    """a paged handle (the store in page-locked host memory): the host compacts every row in place"""
    import numpy as np
    import torch
    import niqki_amd
    from niqki_amd import capi
    N = args.paged
    g = torch.Generator(device="cuda")
    g.manual_seed(args.seed)
    e = niqki_amd.Engine(K=31, S=15, W=12, H=4, min_score_value=capi.min_score(0.1, 15), resident_mib=1024)
    e.set_stream(torch.cuda.current_stream().cuda_stream)
    for a in range(0, N, 4096):
        n = min(4096, N - a)
        e.insert_dev(torch.randint(0, 1 << 12, (n, F), dtype=torch.int32, device="cuda", generator=g), n)
    torch.cuda.synchronize()
    keep = np.arange(N) % 2 == 0
    first = np.nonzero(keep)[0][:8]
    expect = np.stack([e.get_sketches(int(x), 1)[0] for x in first])
    t = time.time()
    n_kept, _ = e.retain(keep)
    wall = time.time() - t
    assert n_kept == int(keep.sum()) and np.array_equal(e.get_sketches(0, first.size), expect)
    res = {"case": "paged", "genomes": N, "kept": n_kept, "host_store_bytes": int(e.stat("store_bytes")),
           "row_bytes_read_and_written": F * n_kept * 4, "call_wall_s": round(wall, 3)}
    e.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", type=int, default=100000)
    ap.add_argument("--slice", type=int, default=4096)
    ap.add_argument("--paged", type=int, default=20000, help="genomes of the paged case")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per case")
    ap.add_argument("--only", default=None, help="comma-separated cases instead of all of them")
    ap.add_argument("--out", default=None)
    ap.add_argument("--case", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    args.extreme = args.genomes                                # (bench_selfjoin.make_index reads it for its other kinds)
    if args.case:
        res = case_host(args) if args.case == "host" else case_paged(args) if args.case == "paged" else case_retain(args, args.case)
        print(json.dumps(res), flush=True)
        return 0
    lines = []
    for case in ("derep", "half", "most", "host", "paged"):
        if args.only and case not in args.only.split(","):
            continue
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--case", case,
               "--genomes", str(args.genomes), "--slice", str(args.slice), "--paged", str(args.paged), "--repeats", str(args.repeats), "--seed", str(args.seed)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:                                  # nothing more on the GPU after a failure
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
