// nq_gather_ops.h -- device helpers that the kernels of a query launch share (nq_gather.hip, nq_lookup.hip).
#pragma once
#include "nq_kernels.h"

namespace nq {

typedef __attribute__((address_space(3))) uint32_t lds_u32;
typedef __attribute__((address_space(3))) void lds_void;
typedef __attribute__((address_space(1))) const void glb_cvoid;

// The packed table (IndexView::ptab, one word per entry) keeps the tiles in GROUPS of two: the words of tiles
// t0, t0 + 1 (t0 even) of all slots lie together as [f_local][R][2] from this word on ([f_local][R][1] for a last
// odd tile) -- a launch over one group streams exactly its own rows.  With <= 2 tiles this is the whole table.
__host__ __device__ inline uint64_t packed_table_offset(const IndexView &v, uint32_t t0) { return (uint64_t)v.f_local * v.d.R * t0; }
__device__ __forceinline__ void wave_lds_fence() {   // this wave's LDS traffic so far has completed
  __builtin_amdgcn_wave_barrier();
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ void lds_barrier() {   // a workgroup barrier that waits for LDS traffic only:
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // the row loads in flight stay in flight
}

}  // namespace nq
