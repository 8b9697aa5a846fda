#!/usr/bin/env python3
"""A recorded sweep of the REAL reference (oracle/_ref) over the parameter space: designed rows at the edges of
K, S, W, H, J and -G, then seeded random cases.  TEST INFRASTRUCTURE ONLY; run in the build container:
    make -C oracle && python oracle/make_goldens_sweep.py
Writes tests/golden/reference_sweep.npz (+ .json).  Data only: per case the parameters, the input records (up to
4 KB verbatim, longer ones by their niqki_synth_genome_host arguments and the fnv1a64 of their bytes) and what the
reference's own Index produced for them -- min_score, H after select_best_H, every record's sketch (F > 1024: its
fnv1a64 and first 8 cells), the hits of each sketch against the index of all of them, the dump's length and md5.

The reference runs in a child process under a time limit (tests/reference_sweep_worker.py): it never returns from a
record whose sketch it cannot finish densifying.  Records on which the oracle predicts that are left out and counted
(at most 15 % of all).  Cases whose constructor H is >= 7 hold clean upper-case ACGT records without A x K / T x K
only: get_fingerprint(0) runs bsr on 0 there, whose result is undefined, and shows for 2^H - 1 > 63."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import pyoracle as po  # noqa: E402
import niqki_amd  # noqa: E402  (host-side synthetic generator only)
import reference_sweep_worker as rsw  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
SEED = 20261018
N_CASES = 150
HUGE_K = (31, 21, 17, 9)          # the four cases with a record of 300 000 bases


def designed_cases():
    c = []

    def add(K, S, W, H, J=0.1, G=0.0, huge=False):
        c.append(dict(K=K, S=S, W=W, H=H, J=J, G=G, huge=huge))
    # K: 1..3, the kernel's loop boundary at 16 / 17, even K (a k-mer can equal its reverse complement), 30 / 31
    for K in (1, 2, 3, 15, 16, 17, 30, 31):
        add(K, min(K, 6), 8, 3)
        add(K, min(K + 1, 9), 11, 4, J=0.0)
    # H in {0, 1, W-1, W} at W in {1, 2, 13, 14, 15}
    for W, Ss in ((1, (3, 1)), (2, (2, 4, 1)), (13, (1, 2, 3, 7)), (14, (5, 1, 6, 2)), (15, (2, 3, 1, 5))):
        for H, S in zip(sorted({0, 1, W - 1, W}), Ss):
            add(21 if H < 7 else 19, S, W, H, J=0.33)
    # H in {7, 8, 11, 15}, W up to 15
    for (W, H), S in zip(((7, 7), (9, 7), (15, 7), (8, 8), (12, 8), (15, 8), (11, 11), (14, 11), (15, 11), (15, 15)),
                         (4, 10, 5, 9, 8, 3, 6, 2, 4, 5)):
        add(31 if S % 2 else 15, S, W, H, J=0.1 if S % 3 else 0.0)
    # S in {1, 2, 3} and 10
    for S in (1, 2, 3, 10):
        add(31, S, 10, 4)
        add(12, S, 10, 4, J=0.33)
    # J
    for J in (0.0, 0.1, 0.33, 0.9):
        add(31, 8, 12, 4, J=J)
        add(17, 7, 9, 2, J=J)
    # -G: select_best_H after the constructor; mask_M and maximal_remainder keep the constructor's values
    for G in (3.0, 150.0, 1e4, 5e6):
        add(31, 10, 10, 4, G=G)
        add(21, 8, 12, 2, G=G)
        add(27, 6, 12, 5, J=0.33, G=G)
    add(23, 5, 12, 8, G=150.0)
    add(31, 7, 13, 9, G=5e6)
    # one record of 300 000 bases
    for K, (S, W, H) in zip(HUGE_K, ((10, 10, 4), (9, 11, 5), (8, 12, 3), (10, 8, 4))):
        add(K, S, W, H, J=0.0, huge=True)
    return c


def main():
    os.makedirs(GOLD, exist_ok=True)
    po.build()
    assert po.have_ref(), "oracle/_ref missing: run make -C oracle (needs /root/reference)"
    designed = designed_cases()
    n_designed = len(designed)
    rng = np.random.default_rng(SEED)
    cases, jobs, kept_all, generated, left_out, drawn = [], [], [], 0, 0, 0
    while len(cases) < N_CASES:
        c = designed[drawn] if drawn < n_designed else dict(rsw.random_case(rng), huge=False)
        assert c["S"] + c["W"] <= 20 and c["H"] <= c["W"] <= 15 and 1 <= c["K"] <= 31
        kept, n, out = rsw.case_records(niqki_amd, po, c, SEED + drawn, huge=c["huge"])
        drawn += 1
        generated += n
        left_out += out
        if not kept:              # a random case none of whose records the reference can finish: its records count as left out
            assert drawn > n_designed, ("no record left in a designed case", c)
            continue
        c["seed"] = SEED + drawn - 1
        cases.append(c)
        kept_all.append(kept)
        jobs.append(dict(c, records=[s for s, _ in kept]))
    assert 120 <= len(cases) <= 200
    assert left_out <= rsw.MAX_LEFT_OUT * generated, (left_out, generated)
    results = rsw.run_reference(jobs, timeout=900)

    vec, meta_cases = {}, []
    seqs, seq_off = [], [0]
    hit_n, hit_counts, hit_gids = [], [], []
    q0 = h0 = 0
    for i, (c, kept, r) in enumerate(zip(cases, kept_all, results)):
        recs = []
        for s, args in kept:
            if s.size <= rsw.VERBATIM_MAX:
                recs.append({"len": int(s.size), "verbatim": len(seq_off) - 1})
                seqs.append(s)
                seq_off.append(seq_off[-1] + s.size)
            else:
                recs.append({"len": int(s.size), "synth": args, "fnv": "%016x" % po.fnv1a64(s)})
        sk = r["sketches"]
        m = dict(seed=c["seed"], K=c["K"], S=c["S"], W=c["W"], H=c["H"], J=c["J"], G=c["G"], min_score=r["min_score"],
                 H_final=r["H_final"], records=recs, q0=q0, h0=h0, dump_len=r["dump_len"], dump_md5=r["dump_md5"])
        if sk.shape[1] > 1024:
            m["sketch_fnv"] = ["%016x" % po.fnv1a64(s) for s in sk]
            vec["head_%03d" % i] = sk[:, :8].astype(np.int32)
        else:
            vec["sk_%03d" % i] = sk.astype(np.int16 if -1 <= sk.min() and sk.max() < 32768 else np.int32)
        hit_n.append(r["hit_n"])
        hit_counts.append(r["hit_counts"])
        hit_gids.append(r["hit_gids"])
        q0 += len(kept)
        h0 += int(r["hit_n"].sum())
        meta_cases.append(m)
    vec["seqs"] = np.concatenate(seqs)
    vec["seq_off"] = np.array(seq_off, np.uint64)
    vec["hit_n"] = np.concatenate(hit_n).astype(np.uint32)
    vec["hit_counts"] = np.concatenate(hit_counts).astype(np.uint32)
    vec["hit_gids"] = np.concatenate(hit_gids).astype(np.uint16)
    meta = {"seed": SEED, "n_designed": n_designed, "records_generated": generated, "records_left_out": left_out,
            "records_recorded": generated - left_out, "cases_drawn": drawn,
            "left_out_reason": "the oracle's densify predicts that the reference never returns on them",
            "cases": meta_cases}
    np.savez_compressed(os.path.join(GOLD, "reference_sweep.npz"), **vec)
    with open(os.path.join(GOLD, "reference_sweep.json"), "w") as f:
        json.dump(meta, f, separators=(",", ":"))
        f.write("\n")
    print("cases %d (%d designed), records %d, left out %d (%.1f %%), hits %d, npz %d bytes" % (
        len(cases), n_designed, generated - left_out, left_out, 100.0 * left_out / generated, h0,
        os.path.getsize(os.path.join(GOLD, "reference_sweep.npz"))))


if __name__ == "__main__":
    main()
