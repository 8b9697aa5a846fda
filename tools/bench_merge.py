#!/usr/bin/env python3
"""niqki_append_dump and niqki_dereplicate_from at the index shape of bench.py: a 100 000-genome index (S = 15, W = 12,
-J 0.1; the families of tools/bench_selfjoin.py, made and inserted on the device) plus a dump of 10 000 more genomes of
the same families.  Every case runs in a child process of its own under its own time limit, one after the other; the
first that fails ends the run.  One JSON line per case:

  append      alternating, --repeats times after a warm-up round: niqki_import_dump of the dump's bytes into a fresh
              handle, and niqki_append_dump of the same bytes to the 100 000-genome index (put back to 100 000 genomes
              with niqki_retain between the rounds, outside the timing).  Wall seconds and bytes per second of each; the
              expectation to test: the append is no slower per byte (both are bound by the host's walk over the size
              words and by PCIe).  The append also grows the store (reserve_store: a new allocation and a device copy of
              the old columns) and is followed by a rebuild or a delta segment at the next use, which is timed apart.
  import_lib  with --lib FILE: the same niqki_import_dump rounds through ANOTHER build of the library (the parent
              commit's), in a process of its own, for the comparison across commits
  derep       on the merged index of 110 000 genomes, alternating: niqki_dereplicate_from(first = 100 000) and
              niqki_dereplicate, profiling on: wall seconds and the phases (stats derep_us_*).  The expectation to test:
              the hits phase of the first near 10 000 / 110 000 of the second's.

    python tools/bench_merge.py [--genomes 100000] [--added 10000] [--repeats 3] [--lib FILE] [--out FILE]
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


def added_dump(args):
    """the dump bytes of the --added genomes (deterministic: every process makes the same bytes)"""
    import bench_selfjoin
    sub = argparse.Namespace(**vars(args))
    sub.genomes, sub.seed = args.added, args.seed + 1
    e, _ = bench_selfjoin.make_index(sub, "families")
    data = e.export_dump()
    e.close()
    return data


def timed_import(capi, torch, data):
    t = time.time()
    b = capi.Engine.import_dump(data)
    b.synchronize()
    s = time.time() - t
    assert b.n_genomes > 0
    b.close()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return s


def case_append(args):
    import numpy as np
    import torch
    from niqki_amd import capi
    import bench_selfjoin
    data = added_dump(args)
    e, N = bench_selfjoin.make_index(args, "families")
    q = e.get_sketches(0, 8)
    e.query(q)
    res = {"case": "append", "genomes": N, "added": args.added, "dump_bytes": len(data), "import_s": [], "append_s": [],
           "next_query_after_append_ms": [], "delta_genomes_after": []}
    probe = capi.Engine.import_dump(data)
    expect = probe.get_sketches(args.added - 4, 4)
    probe.close()
    for rep in range(args.repeats + 1):                        # the first round warms up and is not reported
        s_import = timed_import(capi, torch, data)
        t = time.time()
        e.append_dump(data)
        e.synchronize()
        s_append = time.time() - t
        assert e.n_genomes == N + args.added and np.array_equal(e.get_sketches(N + args.added - 4, 4), expect)
        t = time.time()
        e.query(q)                                             # the delta segment or the rebuild
        torch.cuda.synchronize()
        ms_query = (time.time() - t) * 1e3
        delta = int(e.stat("delta_genomes"))
        e.retain(np.arange(N + args.added) < N)                # back to the old genomes: a new store of the old size
        e.query(q)
        torch.cuda.synchronize()
        if rep:
            res["import_s"].append(round(s_import, 4))
            res["append_s"].append(round(s_append, 4))
            res["next_query_after_append_ms"].append(round(ms_query, 2))
            res["delta_genomes_after"].append(delta)
    res["import_GBps"] = round(len(data) / min(res["import_s"]) / 1e9, 3)
    res["append_GBps"] = round(len(data) / min(res["append_s"]) / 1e9, 3)
    res["append_over_import"] = round(min(res["append_s"]) / min(res["import_s"]), 3)
    e.close()
    return res


def case_import_lib(args):
    from niqki_amd import capi
    import ctypes
    capi._LIB = os.path.abspath(args.lib)                      # before the first call loads the library
    import torch  # noqa: F401  (its HIP runtime first, as capi.lib() does)
    older = ctypes.CDLL(capi._LIB)
    capi.ABI = [x for x in capi.ABI if hasattr(older, x[0])]   # an older build lacks the newest entry points
    data = added_dump(args)
    times = [timed_import(capi, torch, data) for _ in range(args.repeats + 1)][1:]
    return {"case": "import_lib", "lib": args.lib, "added": args.added, "dump_bytes": len(data),
            "import_s": [round(x, 4) for x in times], "import_GBps": round(len(data) / min(times) / 1e9, 3)}


def case_derep(args):
    import numpy as np
    import torch
    import bench_selfjoin
    sub = argparse.Namespace(**vars(args))
    sub.genomes = args.genomes + args.added
    e, N = bench_selfjoin.make_index(sub, "families")
    first, thr = args.genomes, e.min_score
    e.dereplicate(thr)                                         # warm-up: workspace allocations
    e.dereplicate_from(first, thr)
    keys = ("read", "hits", "decide", "assign")
    res = {"case": "derep", "genomes": N, "first": first, "threshold": int(thr), "from": [], "full": []}
    e.profile(True)
    for _ in range(args.repeats):
        for name, call in (("from", lambda: e.dereplicate_from(first, thr)), ("full", lambda: e.dereplicate(thr))):
            t = time.time()
            labels, n_rep = call()
            wall = time.time() - t
            row = {"wall_s": round(wall, 4), "representatives": n_rep, "pairs": int(e.stat("derep_pairs")),
                   "rounds": int(e.stat("derep_rounds"))}
            row.update({k + "_ms": round(e.stat("derep_us_" + k) / 1e3, 3) for k in keys})
            res[name].append(row)
            if name == "from":
                assert np.array_equal(labels[:first], np.arange(first))
    e.profile(False)
    torch.cuda.synchronize()
    hits = [min(r["hits_ms"] for r in res[k]) for k in ("from", "full")]
    res["hits_from_over_full"] = round(hits[0] / hits[1], 4)
    res["new_over_all"] = round((N - first) / N, 4)
    res["wall_from_over_full"] = round(min(r["wall_s"] for r in res["from"]) / min(r["wall_s"] for r in res["full"]), 4)
    e.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", type=int, default=100000)
    ap.add_argument("--added", type=int, default=10000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--lib", default=None, help="another build of libniqki_hip.so for the import_lib case")
    ap.add_argument("--timeout", type=int, default=420, help="seconds per case")
    ap.add_argument("--only", default=None, help="comma-separated cases instead of all of them")
    ap.add_argument("--out", default=None)
    ap.add_argument("--case", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    args.extreme = args.genomes                                # (bench_selfjoin.make_index reads it for its other kinds)
    if args.case:
        res = {"append": case_append, "import_lib": case_import_lib, "derep": case_derep}[args.case](args)
        print(json.dumps(res), flush=True)
        return 0
    lines = []
    for case in ("append", "import_lib", "derep"):
        if (args.only and case not in args.only.split(",")) or (case == "import_lib" and not args.lib):
            continue
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--case", case,
               "--genomes", str(args.genomes), "--added", str(args.added), "--repeats", str(args.repeats), "--seed", str(args.seed)]
        if args.lib:
            cmd += ["--lib", args.lib]
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
