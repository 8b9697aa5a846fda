// nq_sketch_plan.h -- which kernel a sketch launch takes, as a value (launch_sketch, nq_sketch.hip).
//
// A launch is planned from the index parameters, the records' average length and what the caller wants done; the plan
// names the kernel, its LDS and the densification that follows.  sketch_dev and niqki_densify compute a plan, read what
// they need from it (the entry list of the one-wavefront kernel, the form for the stat "last_densify_form") and hand it
// to launch_sketch, which only carries it out.  A caller that wants one kernel whatever the length asks for it by name
// (the requests at the end).
//
// Host only, plain C++17: the kernels include this file for the LDS sizes they share with the rule,
// tests/test_sketch_plan_cpu.py compiles it with g++ and pins the rule row by row.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "nq_common.h"
#include "nq_sketch_lines.h"

namespace nq {

// ---- LDS sizes that the rule and the kernels share ----
constexpr uint32_t kStack = 192;  // candidate k-mers per wave-private stack: < 64 left by a drain + two steps of <= 64
constexpr uint32_t kLevelStateWords = 8;   // line form: a wave's own leveling state, behind its stack
constexpr uint32_t kLevelLdsBytes = 4 * kLevelWords + 16 * 4 * kLevelStateWords;   // ... and behind the 16 stacks the progress words
constexpr size_t kLdsLimit = 160 * 1024;
constexpr uint32_t kReadEntries = 6;                  // one-wavefront kernel: entries per lane (384: reads up to ~400 bases)
constexpr uint32_t kReadMaxEntries = 64 * kReadEntries;
constexpr uint32_t kReadShortEntries = 192;           // ... and its short list
constexpr uint32_t kReadTile = 512;                   // positions coded per tile
constexpr int kLateValues = 4;                        // densify_distinct_kernel: values per thread (2^W <= 4 * 1024)

// ---- the lengths (average input bytes per sketch) at which the rule changes ----
constexpr uint64_t kLenShortList = 200;        // up to here the 192-entry list: a 150-base read fills ~120 cells, and a sketch of
                                               // 2^12 cells leaves room for nine wavefronts per CU instead of eight
constexpr uint64_t kLenWave = 415;             // up to here the one-wavefront kernel (records of up to 384 + K bases: their occupied
                                               // cells fit the 384-entry list.  Longer ones would all take the plain pass over all
                                               // cells -- 21 ms instead of the workgroup kernel's 4.9 per 16 384 records of 500 bases)
constexpr uint64_t kLenLong = 16384;           // from here 1024 lanes and the candidate filter; below, 256 lanes
constexpr uint64_t kLenGroups8 = 1u << 18;     // from here chunks of 8 groups
constexpr uint64_t kLenNoLate = 1u << 19;      // from here no densify launch of its own: longer records leave no cell empty at these
                                               // sketch sizes, and a 5 Mbp genome's sketch must not pay a launch that finds nothing to do
constexpr uint64_t kLenLines = 1u << 21;       // from here chunks of 32 groups, whole lines per lane
static_assert(kLenShortList < kLenWave && kLenWave + 1 < kLenLong && kLenLong <= kLenGroups8 && kLenGroups8 <= kLenLines,
              "the named requests below stand on a length inside the band they name");

// the densification a launch chose (stat "last_densify_form")
enum DensifyForm : uint32_t {
  kDensifyNone = 0,          // the launch stores the cells as they are
  kDensifyWave = 1,          // sketch_reads_kernel: entry windows + closed-form tail, or its pass over all cells
  kDensifyPlain = 2,         // densify_lds inside sketch_kernel
  kDensifyDistinct = 3,      // densify_lds_distinct inside sketch_kernel
  kDensifyDistinctLate = 4,  // densify_distinct_kernel, a launch of its own behind sketch_kernel
  kDensifyGlobal = 5,        // densify_global_kernel (the cells do not fit LDS)
};

// the launch shapes there are: a kernel, its workgroup and the 16-base groups per chunk
enum SketchShape : uint32_t {
  kShapeRefused = 0,        // no launch: launch_sketch answers hipErrorInvalidValue
  kShapeWave = 1,           // sketch_reads_kernel, one wavefront per sketch
  kShape256x1 = 2,          // sketch_kernel<256, 1>
  kShape1024x2 = 3,         // sketch_kernel<1024, 2>
  kShape1024x8 = 4,         // sketch_kernel<1024, 8>
  kShape1024x32 = 5,        // sketch_kernel<1024, 32>: the line form where the filter is on
  kShapeDensifyGlobal = 6,  // densify_global_kernel alone
};

struct SketchPlan {
  SketchShape shape;
  uint32_t read_entries;   // kShapeWave: capacity of the entry list (192 or 384); else 0
  uint32_t halves;         // 2 when the F cells do not fit LDS (S = 16)
  uint32_t distinct;       // densify over distinct values inside sketch_kernel
  uint32_t filter;         // candidate filter: 0 off, 1 automatic, n >= 2 forced strength
  bool late_distinct;      // the kernel stores the cells as they are and densify_distinct_kernel follows
  DensifyForm form;
  size_t lds_bytes;        // dynamic LDS of the shape's kernel
};

// NIQKI_SKETCH_WAVE and NIQKI_SKETCH_FILTER as the launcher read them (sketch_switches(), nq_sketch.hip)
struct SketchSwitches {
  bool wave;         // false: NIQKI_SKETCH_WAVE=0, no one-wavefront kernel
  uint32_t filter;   // 0 = off, unset / 1 = automatic, n >= 2 = force n - 1 leading zeros (tests)
};

// (behind the 16 stacks of a 1024-lane workgroup: the leveling words of the line form)
inline size_t sketch_lds_bytes(const Derived &d, bool distinct, uint32_t ring_waves, uint32_t halves = 1) {
  return (size_t)(d.F / halves) * 4 + 16 + 256 + 2048 + (distinct ? (size_t)d.R * 12 : 0) + (size_t)ring_waves * kStack * 8 +
         (ring_waves == 16 ? kLevelLdsBytes : 0);
}
// true: no launch densifies inside the kernel for these parameters -- the caller fills the output with "empty" first,
// launches with densify = 0, then a densify-only launch (seqs = nullptr)
inline bool sketch_needs_merge(const Derived &d) { return sketch_lds_bytes(d, false, 16) > kLdsLimit; }

// entry list capacity by the records' average length (a record with more occupied cells than the list holds takes the
// plain pass over all cells, or is left to a later launch: SketchArgs::redo_mark)
inline uint32_t sketch_reads_entries(uint64_t avg_len) { return avg_len <= kLenShortList ? kReadShortEntries : kReadMaxEntries; }
inline size_t sketch_reads_lds_bytes(const Derived &d, uint32_t entries = kReadMaxEntries) {
  // sketch cells + one region that holds the position codes and the code table while the k-mers are hashed, the
  // entry list (cell, value) afterwards, the closed-form tail's two lists at the end
  const size_t list = (size_t)entries * 8, tile = kReadTile + 256 + 64;
  return (size_t)d.F * 4 + (list > tile ? list : tile);
}
// LDS of densify_distinct_kernel: the cells, mi[v] and the flags
inline size_t sketch_late_lds_bytes(const Derived &d) { return (size_t)d.F * 4 + (size_t)d.R * 4 + 64; }

// The rule.  avg_len: average input bytes per sketch and workgroup (the caller divides by splits); has_seqs: there are
// record bytes (false: a densify-only launch over the caller's cells); accumulate, densify: as in SketchArgs.
inline SketchPlan sketch_plan(const Derived &d, uint64_t avg_len, uint32_t splits, bool has_seqs, bool accumulate, bool densify,
                              SketchSwitches sw) {
  SketchPlan p{kShapeRefused, 0, sketch_needs_merge(d) ? 2u : 1u, 0, 0, false, kDensifyNone, 0};
  if (p.halves > 1) {
    if (!has_seqs) {  // densify-only launch
      p.shape = kShapeDensifyGlobal;
      p.form = kDensifyGlobal;
      return p;
    }
    if (densify) return p;  // see sketch_needs_merge
  }
  // Launch shape by the average input length of a sketch: one wavefront or a 256-thread workgroup for reads, else
  // 1024 threads with chunks of 32 / 128 / 512 k-mers per lane (long chunks amortise the K-1 warm-up steps, short ones
  // keep all lanes busy on short records).
  // reads: one wavefront per sketch when the sketch and its entry list leave room for several waves per CU
  const uint32_t entries = sketch_reads_entries(avg_len);
  if (avg_len <= kLenWave && splits == 1 && p.halves == 1 && sketch_reads_lds_bytes(d, entries) <= kLdsLimit && sw.wave) {
    p.shape = kShapeWave;
    p.read_entries = entries;
    p.form = densify ? kDensifyWave : kDensifyNone;
    p.lds_bytes = sketch_reads_lds_bytes(d, entries);
    return p;
  }
  const bool short_records = avg_len < kLenLong;
  // distinct-value densification
  // after niqki_select_best_H the fingerprint parts may overlap and leave [0, 2^W): the
  // value-indexed tables and the filter's ordering argument need the regular form
  const bool regular = d.mask_m == (1u << d.M) - 1u && d.max_rem == (1u << d.H) - 1u;
  // ... and cells this launch produced itself: a caller's sketch (niqki_densify, accumulate) may hold
  // any value, the value-indexed tables only values below 2^W
  const bool own_cells = has_seqs && !accumulate;
  // ... and where the values are few against the cells (a pass walks 2^W values instead of 2^S cells, but pays three table
  // words per value: at 2^W = 2^S the plain passes are 1.6 x faster, at 2^S = 4 x 2^W the distinct ones 1.5 x, at 32 x
  // seventeen times -- profiles/r06_densify_lean_and_tail.txt 7) and the tables fit the CU's LDS beside the cells
  // -- inside the kernel for sketches of up to 2^13 cells; larger ones take the launch of its own below, which is faster
  // there even where the tables would fit (S=14 W=12: 28 -> 9 ms per 4096 records of 600 bases)
  p.distinct = (regular && own_cells && short_records && p.halves == 1 && 4u * d.R <= d.F && d.S <= 13 &&
                sketch_lds_bytes(d, true, 0) <= 150 * 1024) ? 1u : 0u;
  // candidate filter: long records only (the kernel picks its strength per sketch)
  p.filter = (regular && !short_records && has_seqs) ? sw.filter : 0u;
  // ... or afterwards, as a launch of its own with a thread's hash words in registers, where the three tables do not fit
  // beside the cells (densify_distinct_kernel)
  p.late_distinct = densify && !p.distinct && regular && own_cells && avg_len < kLenNoLate && p.halves == 1 && splits == 1 &&
                    4u * d.R <= d.F && d.R <= (uint32_t)kLateValues * 1024u && sketch_late_lds_bytes(d) <= kLdsLimit;
  // (a part of a split record and a half of the slots are merged in global memory, not densified)
  p.form = p.late_distinct ? kDensifyDistinctLate
           : !(densify && splits == 1 && p.halves == 1) ? kDensifyNone : p.distinct ? kDensifyDistinct : kDensifyPlain;
  p.lds_bytes = sketch_lds_bytes(d, p.distinct != 0, p.filter ? (short_records ? 4 : 16) : 0, p.halves);
  if (p.lds_bytes > kLdsLimit) return p;   // (cells, stacks and leveling words: S <= 15 per half fits)
  p.shape = short_records ? kShape256x1
            : avg_len < kLenGroups8 ? kShape1024x2
            : avg_len < kLenLines || d.F < 4 ? kShape1024x8   // (F = 2: the line form's LDS state would not sit at multiples of 16 bytes)
            : kShape1024x32;
  return p;
}

// ---- requests by name: the kernel a caller wants whatever its records' lengths.  Each is the rule at a length inside
// the band it names, so a request that the rule refuses there falls through as any launch of that length does. ----

// The one-wavefront kernel with its 384-entry list (the second launch of the read chain; cells the caller brings).
// Where the rule refuses that shape -- the wave switch is off, the list does not fit LDS beside the cells, halves > 1
// -- the 256-lane workgroup kernel.
inline SketchPlan sketch_plan_long_list(const Derived &d, bool has_seqs, bool accumulate, bool densify, SketchSwitches sw) {
  return sketch_plan(d, kLenWave, 1, has_seqs, accumulate, densify, sw);
}
// The 256-lane workgroup kernel on record bytes (the last launch of the read chain)
inline SketchPlan sketch_plan_workgroup(const Derived &d, bool densify, SketchSwitches sw) {
  return sketch_plan(d, kLenWave + 1, 1, true, false, densify, sw);
}
// The densify-only launch behind merged partial sketches: densify_global_kernel where the cells do not fit LDS, else
// sketch_kernel without record bytes -- at the length of the longest records, so the 1024 x 32 instantiation (F >= 4).
inline SketchPlan sketch_plan_densify_only(const Derived &d, SketchSwitches sw) {
  return sketch_plan(d, kLenLines, 1, false, true, true, sw);
}
// niqki_densify: the one-wavefront kernel with the long list for sketches of up to 2^12 cells, else the densify-only launch
inline SketchPlan sketch_plan_densify_rows(const Derived &d, SketchSwitches sw) {
  return d.F <= 4096 ? sketch_plan_long_list(d, false, true, true, sw) : sketch_plan_densify_only(d, sw);
}

}  // namespace nq
