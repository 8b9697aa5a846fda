"""The sketch launch rule (niqki_amd/csrc/nq_sketch_plan.h), on the CPU: the header is the code sketch_dev, niqki_densify
and launch_sketch run, compiled here with g++ and asked for the plan of every row of the table below.  The expected
plans are typed in, read off the rule as launch_sketch stated it before the plan was a value (thresholds on the average
length 200 / 415 / 16384 / 2^18 / 2^19 / 2^21; the LDS sums worked out per row group); nothing here computes them."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r"""
#include <cstdio>
#include <cstring>
#include "nq_sketch_plan.h"

// one row per line of stdin: request S W H H_after avg_len splits seqs accumulate densify wave filter_mode
int main() {
  char req[32];
  unsigned S, W, H, H2, splits, seqs, acc, dens, wave, fmode;
  unsigned long long avg;
  while (scanf("%31s %u %u %u %u %llu %u %u %u %u %u %u", req, &S, &W, &H, &H2, &avg, &splits, &seqs, &acc, &dens, &wave, &fmode) == 12) {
    nq::Derived d{};
    d.K = 31; d.S = S; d.W = W; d.H = H; d.M = W - H; d.F = 1u << S; d.R = 1u << W;
    d.mask_m = (1u << d.M) - 1u; d.max_rem = (1u << H) - 1u;
    d.slot_begin = 0; d.slot_end = d.F; d.kmer_mask = (1ull << 62) - 1;
    // niqki_select_best_H changes H and M only; mask_m and max_rem stay as the constructor left them
    d.H = H2; d.M = W - H2;
    const nq::SketchSwitches sw{wave != 0, fmode};
    nq::SketchPlan p;
    if (!strcmp(req, "rule")) p = nq::sketch_plan(d, avg, splits, seqs != 0, acc != 0, dens != 0, sw);
    else if (!strcmp(req, "long_list")) p = nq::sketch_plan_long_list(d, seqs != 0, acc != 0, dens != 0, sw);
    else if (!strcmp(req, "workgroup")) p = nq::sketch_plan_workgroup(d, dens != 0, sw);
    else if (!strcmp(req, "densify_only")) p = nq::sketch_plan_densify_only(d, sw);
    else if (!strcmp(req, "densify_rows")) p = nq::sketch_plan_densify_rows(d, sw);
    else return 2;
    printf("%u %u %u %u %u %u %u %zu\n", (unsigned)p.shape, p.read_entries, p.halves, p.distinct, p.filter,
           (unsigned)p.late_distinct, (unsigned)p.form, p.lds_bytes);
  }
  printf("needs_merge");
  for (unsigned S = 12; S <= 16; ++S) { nq::Derived d{}; d.S = S; d.F = 1u << S; printf(" %d", (int)nq::sketch_needs_merge(d)); }
  printf("\n");
  return 0;
}
"""

# shapes and forms as the header numbers them
REFUSED, WAVE, WG256, WG2, WG8, WG32, GLOBAL = range(7)
NONE, F_WAVE, PLAIN, DISTINCT, LATE, F_GLOBAL = range(6)

# LDS bytes.  Workgroup kernel: cells + 2320 (code tables, flags) [+ 12 R distinct tables] [+ 4 or 16 stacks of 1536, and
# 576 of leveling words behind 16].  One-wavefront kernel: cells + 8 bytes per list entry.
A_PLAIN = 131072 + 2320                  # S = 15: 133392
A_FILTER = A_PLAIN + 16 * 1536 + 576     # 158544
A_W192, A_W384 = 131072 + 1536, 131072 + 3072
B_PLAIN = 16384 + 2320                   # S = 12: 18704
B_DISTINCT = B_PLAIN + 12 * 1024         # W = 10: 30992
B_FILTER = B_PLAIN + 16 * 1536 + 576     # 43856
B_W192, B_W384 = 16384 + 1536, 16384 + 3072
C_PLAIN, C_W384 = 65536 + 2320, 65536 + 3072   # S = 14

A = (15, 12, 4, 4)   # the reference's defaults: late distinct form (S = 15, W = 12)
B = (12, 10, 4, 4)   # in-kernel distinct form (S <= 13, 4 * 2^W <= 2^S)
C = (14, 12, 4, 4)   # late distinct form at S = 14
D = (16, 12, 4, 4)   # halves = 2: the cells do not fit LDS
E = (1, 12, 4, 4)    # F = 2
G = (15, 12, 4, 6)   # after niqki_select_best_H: no longer regular
GB = (12, 10, 4, 3)

# (request, (S, W, H, H after select_best_H), avg_len, splits, seqs, accumulate, densify, wave switch, filter mode)
#   -> (shape, list capacity, halves, distinct, filter, late_distinct, form, LDS bytes)
TABLE = [
    # ---- the defaults, records sketched and densified in one call: both sides of every length threshold ----
    (("rule", A, 150, 1, 1, 0, 1, 1, 1), (WAVE, 192, 1, 0, 0, 0, F_WAVE, A_W192)),
    (("rule", A, 200, 1, 1, 0, 1, 1, 1), (WAVE, 192, 1, 0, 0, 0, F_WAVE, A_W192)),
    (("rule", A, 201, 1, 1, 0, 1, 1, 1), (WAVE, 384, 1, 0, 0, 0, F_WAVE, A_W384)),
    (("rule", A, 415, 1, 1, 0, 1, 1, 1), (WAVE, 384, 1, 0, 0, 0, F_WAVE, A_W384)),
    (("rule", A, 416, 1, 1, 0, 1, 1, 1), (WG256, 0, 1, 0, 0, 1, LATE, A_PLAIN)),
    (("rule", A, 16383, 1, 1, 0, 1, 1, 1), (WG256, 0, 1, 0, 0, 1, LATE, A_PLAIN)),
    (("rule", A, 16384, 1, 1, 0, 1, 1, 1), (WG2, 0, 1, 0, 1, 1, LATE, A_FILTER)),
    (("rule", A, 2**18 - 1, 1, 1, 0, 1, 1, 1), (WG2, 0, 1, 0, 1, 1, LATE, A_FILTER)),
    (("rule", A, 2**18, 1, 1, 0, 1, 1, 1), (WG8, 0, 1, 0, 1, 1, LATE, A_FILTER)),
    (("rule", A, 2**19 - 1, 1, 1, 0, 1, 1, 1), (WG8, 0, 1, 0, 1, 1, LATE, A_FILTER)),
    (("rule", A, 2**19, 1, 1, 0, 1, 1, 1), (WG8, 0, 1, 0, 1, 0, PLAIN, A_FILTER)),
    (("rule", A, 2**21 - 1, 1, 1, 0, 1, 1, 1), (WG8, 0, 1, 0, 1, 0, PLAIN, A_FILTER)),
    (("rule", A, 2**21, 1, 1, 0, 1, 1, 1), (WG32, 0, 1, 0, 1, 0, PLAIN, A_FILTER)),
    # ---- the switches: no one-wavefront kernel; filter off, forced strength (long records only) ----
    (("rule", A, 150, 1, 1, 0, 1, 0, 1), (WG256, 0, 1, 0, 0, 1, LATE, A_PLAIN)),
    (("rule", A, 5000000, 1, 1, 0, 1, 1, 0), (WG32, 0, 1, 0, 0, 0, PLAIN, A_PLAIN)),
    (("rule", A, 5000000, 1, 1, 0, 1, 1, 4), (WG32, 0, 1, 0, 4, 0, PLAIN, A_FILTER)),
    (("rule", A, 1000, 1, 1, 0, 1, 1, 4), (WG256, 0, 1, 0, 0, 1, LATE, A_PLAIN)),
    # ---- accumulate (the cells are not the launch's own: no distinct form), no densification ----
    (("rule", A, 1000, 1, 1, 1, 1, 1, 1), (WG256, 0, 1, 0, 0, 0, PLAIN, A_PLAIN)),
    (("rule", A, 150, 1, 1, 1, 1, 1, 1), (WAVE, 192, 1, 0, 0, 0, F_WAVE, A_W192)),
    (("rule", A, 1000, 1, 1, 0, 0, 1, 1), (WG256, 0, 1, 0, 0, 0, NONE, A_PLAIN)),
    (("rule", A, 150, 1, 1, 0, 0, 1, 1), (WAVE, 192, 1, 0, 0, 0, NONE, A_W192)),
    # ---- splits = 2: parts are merged in global memory, never densified, never the one-wavefront kernel ----
    (("rule", A, 2**20, 2, 1, 0, 0, 1, 1), (WG8, 0, 1, 0, 1, 0, NONE, A_FILTER)),
    (("rule", A, 300, 2, 1, 0, 1, 1, 1), (WG256, 0, 1, 0, 0, 0, NONE, A_PLAIN)),
    # ---- the named requests at the defaults: granted, and the long list refused by the wave switch ----
    (("long_list", A, 0, 1, 1, 0, 1, 1, 1), (WAVE, 384, 1, 0, 0, 0, F_WAVE, A_W384)),
    (("long_list", A, 0, 1, 1, 0, 1, 0, 1), (WG256, 0, 1, 0, 0, 1, LATE, A_PLAIN)),
    (("workgroup", A, 0, 1, 1, 0, 1, 1, 1), (WG256, 0, 1, 0, 0, 1, LATE, A_PLAIN)),
    (("densify_only", A, 0, 1, 0, 1, 1, 1, 1), (WG32, 0, 1, 0, 0, 0, PLAIN, A_PLAIN)),
    (("densify_rows", A, 0, 1, 0, 1, 1, 1, 1), (WG32, 0, 1, 0, 0, 0, PLAIN, A_PLAIN)),
    # ---- S = 12, W = 10: the distinct form inside the kernel for short records, the late one for long ones ----
    (("rule", B, 150, 1, 1, 0, 1, 1, 1), (WAVE, 192, 1, 0, 0, 0, F_WAVE, B_W192)),
    (("rule", B, 1000, 1, 1, 0, 1, 1, 1), (WG256, 0, 1, 1, 0, 0, DISTINCT, B_DISTINCT)),
    (("rule", B, 20000, 1, 1, 0, 1, 1, 1), (WG2, 0, 1, 0, 1, 1, LATE, B_FILTER)),
    (("rule", B, 1000, 1, 1, 1, 1, 1, 1), (WG256, 0, 1, 0, 0, 0, PLAIN, B_PLAIN)),
    (("workgroup", B, 0, 1, 1, 0, 1, 1, 1), (WG256, 0, 1, 1, 0, 0, DISTINCT, B_DISTINCT)),
    (("densify_rows", B, 0, 1, 0, 1, 1, 1, 1), (WAVE, 384, 1, 0, 0, 0, F_WAVE, B_W384)),
    (("densify_rows", B, 0, 1, 0, 1, 1, 0, 1), (WG256, 0, 1, 0, 0, 0, PLAIN, B_PLAIN)),
    # ---- S = 14, W = 12: too many cells for the tables inside the kernel ----
    (("rule", C, 600, 1, 1, 0, 1, 1, 1), (WG256, 0, 1, 0, 0, 1, LATE, C_PLAIN)),
    (("rule", C, 300, 1, 1, 0, 1, 1, 1), (WAVE, 384, 1, 0, 0, 0, F_WAVE, C_W384)),
    # ---- S = 16: halves = 2; densify refused with record bytes; global densify; requests fall through or are refused.
    # (A 384-entry list that does not fit 160 KB beside the cells is this case too: such cells do not fit beside 16 stacks.) ----
    (("rule", D, 150, 1, 1, 0, 1, 1, 1), (REFUSED, 0, 2, 0, 0, 0, NONE, 0)),
    (("rule", D, 150, 1, 1, 0, 0, 1, 1), (WG256, 0, 2, 0, 0, 0, NONE, A_PLAIN)),
    (("rule", D, 5000000, 1, 1, 0, 0, 1, 1), (WG32, 0, 2, 0, 1, 0, NONE, A_FILTER)),
    (("long_list", D, 0, 1, 1, 0, 0, 1, 1), (WG256, 0, 2, 0, 0, 0, NONE, A_PLAIN)),
    (("workgroup", D, 0, 1, 1, 0, 1, 1, 1), (REFUSED, 0, 2, 0, 0, 0, NONE, 0)),
    (("densify_only", D, 0, 1, 0, 1, 1, 1, 1), (GLOBAL, 0, 2, 0, 0, 0, F_GLOBAL, 0)),
    (("densify_rows", D, 0, 1, 0, 1, 1, 1, 1), (GLOBAL, 0, 2, 0, 0, 0, F_GLOBAL, 0)),
    # ---- F = 2: never 1024 x 32 ----
    (("rule", E, 5000000, 1, 1, 0, 1, 1, 1), (WG8, 0, 1, 0, 1, 0, PLAIN, 8 + 2320 + 16 * 1536 + 576)),
    (("densify_only", E, 0, 1, 0, 1, 1, 1, 1), (WG8, 0, 1, 0, 0, 0, PLAIN, 8 + 2320)),
    (("densify_rows", E, 0, 1, 0, 1, 1, 1, 1), (WAVE, 384, 1, 0, 0, 0, F_WAVE, 8 + 3072)),
    # ---- after niqki_select_best_H: no filter, no distinct form of either kind ----
    (("rule", G, 5000000, 1, 1, 0, 1, 1, 1), (WG32, 0, 1, 0, 0, 0, PLAIN, A_PLAIN)),
    (("rule", G, 1000, 1, 1, 0, 1, 1, 1), (WG256, 0, 1, 0, 0, 0, PLAIN, A_PLAIN)),
    (("rule", GB, 1000, 1, 1, 0, 1, 1, 1), (WG256, 0, 1, 0, 0, 0, PLAIN, B_PLAIN)),
    (("rule", G, 150, 1, 1, 0, 1, 1, 1), (WAVE, 192, 1, 0, 0, 0, F_WAVE, A_W192)),
]


def test_plan_of_every_row(tmp_path):
    """Every row's plan -- shape, list capacity, halves, distinct, filter, late_distinct, form, LDS bytes -- is the one
    typed in; sketch_needs_merge is true at S = 16 alone."""
    assert len(TABLE) >= 40
    src = tmp_path / "plan.cpp"
    src.write_text(SRC)
    exe = tmp_path / "plan"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "niqki_amd", "csrc"),
                           str(src), "-o", str(exe)])
    rows = "".join("%s %d %d %d %d %d %d %d %d %d %d %d\n" % ((req,) + tuple(params) + tuple(rest)) for (req, params, *rest), _ in TABLE)
    out = subprocess.run([str(exe)], input=rows, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.strip().split("\n")
    assert len(lines) == len(TABLE) + 1
    bad = [(row, want, tuple(int(x) for x in line.split()))
           for (row, want), line in zip(TABLE, lines) if tuple(int(x) for x in line.split()) != want]
    assert not bad, "\n".join("%r: expected %r, got %r" % b for b in bad)
    assert lines[-1] == "needs_merge 0 0 0 0 1"
