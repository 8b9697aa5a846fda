"""The designs of tests/sketch_chunks.py, on the CPU: the launch shape they restate against the compiled rule
(niqki_amd/csrc/nq_sketch_plan.h, as test_sketch_plan_cpu.py compiles it), the lines of the kernels they restate
against the source text, and every condition of tests/test_gpu_sketch_chunks.py that rests on the oracle alone."""
import os
import re
import subprocess

import numpy as np
import pytest

import sketch_chunks as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "niqki_amd", "csrc")

SRC = r"""
#include <cstdio>
#include <cstring>
#include "nq_sketch_plan.h"

// one row per line of stdin: request K S W H H_after avg_len splits densify filter_mode
int main() {
  char req[32];
  unsigned K, S, W, H, H2, splits, dens, fmode;
  unsigned long long avg;
  while (scanf("%31s %u %u %u %u %u %llu %u %u %u", req, &K, &S, &W, &H, &H2, &avg, &splits, &dens, &fmode) == 10) {
    nq::Derived d{};
    d.K = K; d.S = S; d.W = W; d.H = H; d.M = W - H; d.F = 1u << S; d.R = 1u << W;
    d.mask_m = (1u << d.M) - 1u; d.max_rem = (1u << H) - 1u;
    d.slot_begin = 0; d.slot_end = d.F; d.kmer_mask = (1ull << (2 * K)) - 1;
    d.H = H2; d.M = W - H2;   // niqki_select_best_H changes H and M only
    const nq::SketchSwitches sw{true, fmode};
    nq::SketchPlan p;
    if (!strcmp(req, "rule")) p = nq::sketch_plan(d, avg, splits, true, false, dens != 0, sw);
    else if (!strcmp(req, "densify_only")) p = nq::sketch_plan_densify_only(d, sw);
    else return 2;
    printf("%u %u %u %u %u %u %zu %d\n", (unsigned)p.shape, p.halves, p.distinct, p.filter, (unsigned)p.late_distinct,
           (unsigned)p.form, p.lds_bytes, (int)nq::sketch_needs_merge(d));
  }
  return 0;
}
"""


def _squash(s):
    return re.sub(r"\s+", " ", s)


def _source(name):
    return _squash(open(os.path.join(CSRC, name)).read())


def test_shape_of_names_the_plan_of_the_header(tmp_path):
    """For every designed batch and filter mode: the shape the design asserts is the one shape_of names, and the
    compiled rule, asked with the split count that shape_of restates from sketch_dev, names the same shape, halves,
    distinct form, filter, late form, LDS bytes and reported densify form."""
    src = tmp_path / "plan.cpp"
    src.write_text(SRC)
    exe = tmp_path / "plan"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)])
    rows, want = [], []
    for b in sc.ALL:
        for mode in b.modes:
            p = b.check_shape(mode)
            H2 = b.H if b.H_after is None else b.H_after
            merged = p["splits"] > 1 or p["halves"] > 1
            rows.append("rule %d %d %d %d %d %d %d %d %s" % (b.K, b.S, b.W, b.H, H2, p["avg_len"], p["splits"], 0 if merged else 1, mode))
            own = sc.NONE if merged else p["form"]
            want.append((b.name, mode, (sc.SHAPE_NAMES[(p["block"], p["groups"])], p["halves"], p["distinct"], p["filter"], int(p["late"]),
                                        own, p["lds"], int(p["halves"] > 1))))
            if merged:
                rows.append("densify_only %d %d %d %d %d 0 1 1 %s" % (b.K, b.S, b.W, b.H, H2, mode))
                want.append((b.name, mode + " merge", p["form"]))
    out = subprocess.run([str(exe)], input="\n".join(rows) + "\n", capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.strip().split("\n")
    assert len(lines) == len(want)
    bad = []
    for w, line in zip(want, lines):
        got = tuple(int(x) for x in line.split())
        if isinstance(w[2], tuple):
            if got != w[2]:
                bad.append((w, got))
        elif got[5] != w[2]:
            bad.append((w, got))
    assert not bad, "\n".join("%r: got %r" % x for x in bad)


def test_restated_lines_stand_in_the_source():
    """The lines that the designs restate outside the plan header stand in the kernels as they were read: sketch_dev's
    cut into parts, the chunk rule at the head of roll_records' record loop, the part boundaries and the filter
    strength of sketch_kernel.  A change to one of them has to come with a change to tests/sketch_chunks.py."""
    build = _source("nq_api_build.hip")
    assert _squash("""if (avg >= 16384 && !entry_rec && n_entry < 128 && avg >= (1u << 20))
                      a.splits = std::min<uint32_t>(32, 512 / n_entry);""") in build
    assert "nq::sketch_plan(ix->d, avg / a.splits, a.splits, true, false, false, sw)" in build
    assert "nq::sketch_plan(ix->d, avg, 1, true, false, true, sw)" in build
    sketch = _source("nq_sketch.hip")
    for line in ("""const uint64_t share = n_kmers / a.splits + 1u;""",
                 """const uint64_t rounds = (share + (uint64_t)BLOCK * 16u * GROUPS - 1u) / ((uint64_t)BLOCK * 16u * GROUPS);""",
                 """groups = (uint32_t)((share + rounds * BLOCK * 16u - 1u) / (rounds * BLOCK * 16u));""",
                 """groups = groups < 1u ? 1u : groups > (uint32_t)GROUPS ? (uint32_t)GROUPS : groups;""",
                 """const uint32_t CHUNK = 16u * groups; const uint64_t n_chunks = (n_kmers + CHUNK - 1) / CHUNK;""",
                 """const uint64_t c_lo = n_chunks * part / a.splits; const uint64_t c_hi = n_chunks * (part + 1) / a.splits;""",
                 """const uint64_t per_slot = (n / a.splits) >> d.S;""",
                 """uint32_t T = per_slot >= 240 ? 4u : per_slot >= 115 ? 3u : per_slot >= 55 ? 2u : 0u;""",
                 """if (a.filter >= 2) T = a.filter - 1;""",
                 """if (T > d.max_rem || T > 16) T = 0;""",
                 """constexpr uint32_t kFastKMin = 17;"""):
        assert _squash(line) in sketch, line
    assert "constexpr uint32_t kStack = 192;" in _source("nq_sketch_plan.h")


def test_records_are_what_the_designs_say():
    """Sizes: no input above 40 MiB; the record lengths of the table batches are the tables' k-mers plus K."""
    for b in sc.ALL:
        assert b.total() <= 40 << 20, b.name
    for b in sc.LENGTH_EDGES:
        table = {"edges-1024x2": sc.T2, "edges-1024x8": sc.T8, "groups-1024x8": sc.T8_GROUPS, "edges-256x1": sc.T1}[b.name.rsplit("-", 1)[0]]
        assert [r.size - b.K for r in b.records()[:len(table)]] == [n for n, _ in table], b.name
    # the dirty records are dirty where the design says: at least one byte outside ACGT on both sides of a chunk edge
    for b in sc.DIRTY:
        a = b.records()[0]
        _, CHUNK, _, _ = sc.chunk_geometry(b.block, b.groups, a.size - b.K)
        edge = 4 * CHUNK + b.K - 1
        assert bytes(a[edge - 1:edge + 1]) == b"Na", b.name


@pytest.mark.parametrize("b", sc.STACK, ids=lambda b: b.name)
def test_runs_reach_the_zero_hash(po, b):
    """Stack pressure: every k-mer inside a run of N, A or T has the canonical word 0 and the hash 0, so the oracle's
    sketch holds fingerprint(0) and, the records being long, no empty cell."""
    p, ref = sc.reference(po, b)
    fp0 = po.fingerprint(0, b.W, b.H)
    for i in range(ref.shape[0]):
        assert (ref[i] == fp0).any(), (b.name, i)
        assert not (ref[i] == -1).any(), (b.name, i)


def test_select_best_h_leaves_cells_above_the_range(po):
    """After select_best_H the oracle has another H and its sketches hold cells of 2^W and above."""
    for b in sc.SELECTED:
        p, ref = sc.reference(po, b)
        assert p.H != b.H and p.H == b.H_after, (b.name, p.H)
        assert (ref >= (1 << b.W)).any(), b.name


def test_forced_strength_six_leaves_slots_without_candidate(po):
    """Mode "7" asks six leading zeros: the batch's first record has fewer such k-mers than slots, so some slot's
    smallest fingerprint (before densification) is one the filter drops, and the kernel must take the exact re-run."""
    b = next(x for x in sc.STRENGTH if "7" in x.modes)
    p, _ = sc.reference(po, b)
    acc = po.sketch_accumulate(p, b.records()[0])
    T, M, max_rem = 6, b.W - b.H, (1 << b.H) - 1
    assert sc.strength(b.S, b.H, b.entry_kmers()[0], 1, 7) == T
    # get_fingerprint: the HyperLogLog part is max_rem - leading zeros (0 once saturated), above the M low bits
    assert ((acc == -1) | ((acc >> M) > max_rem - T)).any()
