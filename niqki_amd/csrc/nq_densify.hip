// nq_densify.hip -- densification as launches of their own, behind sketch_kernel (nq_sketch.hip) or on cells the caller
// brings: over distinct values with the cells in LDS (densify_distinct_kernel), or on cells in global memory where
// they do not fit LDS (densify_global_kernel).  The pass-parallel restatement of src/niqki_index.cpp:313-331 is that
// of densify_lds / densify_lds_distinct (nq_sketch.hip; DESIGN.md "densification").
#include "nq_kernels.h"

namespace nq {

// Distinct-value densification as a launch of its own, for sketches whose cells leave no room for the three tables
// of densify_lds_distinct beside them (the reference's defaults, S = 15 W = 12: 128 KB of cells, 48 KB of tables): a
// thread's values are always the same ones (v = tid + k 1024, k < 4: 2^W <= 4096), so their two hash words live in its
// registers and the LDS holds the cells and mi[v] alone.  The sketch kernel stores the cells as they are (densify = 0),
// this kernel takes them from there.  Records of 0.6 .. 15 kbp at S = 15 W = 12: see profiles/r06_densify_lean_and_tail.txt.
__global__ __launch_bounds__(1024) void densify_distinct_kernel(SketchArgs a) {
  extern __shared__ __align__(16) uint32_t smem[];
  const Derived &d = a.d;
  const uint32_t F = d.F, R = d.R, W = d.W, tid = threadIdx.x;
  const uint32_t entry = blockIdx.x;
  if (a.redo_only && a.redo[entry] != a.redo_only) return;   // (uniform) not this launch's sketch
  uint32_t *sk = smem, *mi = smem + F, *s_flag = mi + R;
  uint32_t *row = (uint32_t *)a.sketches + (uint64_t)entry * F;
  uint32_t local = 0;
  for (uint32_t i = tid; i < F; i += 1024) {
    const uint32_t v = row[i];
    sk[i] = v;
    local += (v == kEmpty32);
  }
  for (uint32_t v = tid; v < R; v += 1024) mi[v] = kEmpty32;
  if (tid == 0) { s_flag[0] = 0; s_flag[1] = 0; }
  __syncthreads();
  if (local) atomicAdd(&s_flag[0], local);
  for (uint32_t i = tid; i < F; i += 1024) {
    const uint32_t v = sk[i];
    if (v != kEmpty32) atomicMin(&mi[v], i);
  }
  __syncthreads();
  uint32_t empty = s_flag[0];
  if (empty == 0 || empty == F) return;   // (nothing to fill, or nothing to fill from: the row stays as it is)
  uint32_t ra[kLateValues], rb[kLateValues];
#pragma unroll
  for (int k = 0; k < kLateValues; ++k) {
    const uint32_t v = tid + (uint32_t)k * 1024u;
    ra[k] = (uint32_t)unrev64(v);
    rb[k] = (uint32_t)rev64(v);
  }
  uint32_t step = 0, idle = 0;
  while (true) {
    uint32_t mk[kLateValues], filled = 0;   // this pass's proposals (all ones: none)
#pragma unroll
    for (int k = 0; k < kLateValues; ++k) {
      const uint32_t v = tid + (uint32_t)k * 1024u;
      const uint32_t m = v < R ? mi[v] : kEmpty32;
      const uint32_t t = (ra[k] + step * rb[k]) & (F - 1u);  // hash_family(v, step) % F, src/niqki_index.cpp:308-310,:319
      const bool prop = m != kEmpty32 && sk[t] >= 0x80000000u;
      mk[k] = prop ? (0x80000000u | (m << W) | v) : kEmpty32;
      if (prop) atomicMin(&sk[t], mk[k]);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kLateValues; ++k) {
      const uint32_t v = tid + (uint32_t)k * 1024u;
      const uint32_t t = (ra[k] + step * rb[k]) & (F - 1u);
      const bool won = mk[k] != kEmpty32 && sk[t] == mk[k];
      if (won) {
        sk[t] = v;
        if (t < ((mk[k] & 0x7FFFFFFFu) >> W)) mi[v] = t;
      }
      filled += won ? 1u : 0u;
    }
    if (filled) atomicAdd(&s_flag[1], filled);
    __syncthreads();
    const uint32_t tot = s_flag[1];  // every proposed-to cell now holds its winner's value
    __syncthreads();
    if (tid == 0) s_flag[1] = 0;
    empty -= tot;
    ++step;
    idle = tot ? 0u : idle + 1u;
    if (empty == 0 || idle >= F) break;
    __syncthreads();
  }
  __syncthreads();
  for (uint32_t i = tid; i < F; i += 1024) row[i] = sk[i];
}

// densify_lds on the cells in global memory.  One workgroup per sketch; the cells are read and
// written with agent-scope atomics only (a plain load could see a stale L1 line behind another
// wave's atomicMin).  Rare path: a 5 Mbp genome has no empty cell at S = 16 and leaves after the count.
__global__ __launch_bounds__(1024) void densify_global_kernel(SketchArgs a) {
  __shared__ uint32_t s_flag[2];
  const Derived &d = a.d;
  const uint32_t F = d.F, tid = threadIdx.x;
  uint32_t *sk = (uint32_t *)a.sketches + (uint64_t)blockIdx.x * F;
  auto ld = [&](uint32_t i) { return __hip_atomic_load(&sk[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
  auto st = [&](uint32_t i, uint32_t v) { __hip_atomic_store(&sk[i], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
  uint32_t local = 0;
  for (uint32_t i = tid; i < F; i += 1024) local += (ld(i) == kEmpty32);
  if (tid == 0) { s_flag[0] = 0; s_flag[1] = 0; }
  __syncthreads();
  if (local) atomicAdd(&s_flag[0], local);
  __syncthreads();
  uint32_t empty = s_flag[0];
  if (empty == 0 || empty == F) return;
  uint32_t step = 0, idle = 0;
  while (true) {
    for (uint32_t i = tid; i < F; i += 1024) {
      const uint32_t v = ld(i);
      if (v < 0x80000000u) {
        const uint32_t t = ((uint32_t)unrev64(v) + step * (uint32_t)rev64(v)) & (F - 1u);  // :308-310, :319
        atomicMin(&sk[t], 0x80000000u | i);
      }
    }
    __threadfence();
    __syncthreads();
    uint32_t filled = 0;
    for (uint32_t i = tid; i < F; i += 1024) {
      const uint32_t v = ld(i);
      if (v >= 0x80000000u && v != kEmpty32) { st(i, ld(v & 0x7FFFFFFFu)); ++filled; }
    }
    if (filled) atomicAdd(&s_flag[1], filled);
    __threadfence();
    __syncthreads();
    const uint32_t tot = s_flag[1];
    __syncthreads();
    if (tid == 0) s_flag[1] = 0;
    empty -= tot;
    ++step;
    idle = tot ? 0u : idle + 1u;
    if (empty == 0 || idle >= F) break;
    __syncthreads();
  }
}

hipError_t launch_densify_distinct(const SketchArgs &a, uint32_t n_entry, size_t lds, hipStream_t stream) {
  hipError_t e = hipFuncSetAttribute((const void *)densify_distinct_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(densify_distinct_kernel, dim3(n_entry), dim3(1024), lds, stream, a);
  return hipGetLastError();
}

hipError_t launch_densify_global(const SketchArgs &a, uint32_t n_entry, hipStream_t stream) {
  hipLaunchKernelGGL(densify_global_kernel, dim3(n_entry), dim3(1024), 0, stream, a);
  return hipGetLastError();
}

}  // namespace nq
