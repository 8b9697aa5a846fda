// nq_unite_blocks.h -- launch shape of the per-label minimum over the sketch store (nq_unite.hip, store_unite_kernel;
// niqki_unite).
//
// The sketch store is u16 [slot][cap], one column per genome, 0xFFFF = empty.  Uniting genomes by label writes a NEW
// store with one column per label: cell (s, l) is the unsigned minimum of row s over the columns of label l's members.
// A wavefront owns kUniteCols consecutive DESTINATION columns of kUniteRows consecutive rows, lane i column c0 + i.
//   lane route   a label of at most kUniteLaneMax members is folded by its own lane, member after member
//   wave route   a larger label is folded by the whole wavefront, lanes striding over its members, one label after
//                the other; lane r of the wavefront then holds row r's minimum
// Either way the cell is stored by one lane, once, 2 bytes; a column in [L, cap) is stored as empty by its lane.
//
// Host and device share these numbers: the kernel and the launch use them, the designed labellings of
// tests/unite_ref.py read them from this file.
#pragma once
#include <stdint.h>

namespace nq {

constexpr uint32_t kUniteCols = 64;      // destination columns of a wavefront: one per lane
constexpr uint32_t kUniteWaves = 4;      // wavefronts of a workgroup (kUniteCols * kUniteWaves columns)
constexpr uint32_t kUniteRows = 16;      // slot rows a wavefront serves with one reading of its labels' member lists
constexpr uint32_t kUniteLaneMax = 32;   // members of the largest label a single lane folds

}  // namespace nq
