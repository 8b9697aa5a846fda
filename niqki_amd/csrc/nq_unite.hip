// nq_unite.hip -- niqki_unite's device pass: the per-label minimum over the columns of the sketch store.
//
// src is u16 [f_local][src_cap], dst u16 [f_local][dst_cap]; label l's members are members[off[l] .. off[l + 1]),
// ascending genome ids below src_cap.  dst(s, l) = the unsigned minimum of src(s, m) over l's members; 0xFFFF (empty)
// compares above every valid cell, so a label without a valid cell in row s comes out empty; so do the columns
// [n_labels, dst_cap).  Launch shape and the two routes: nq_unite_blocks.h.  A wavefront reads the member list of each of
// its labels once and keeps kUniteRows running minima per lane, so a member costs kUniteRows independent 2-byte loads;
// there is no LDS, no barrier and no atomic, and every destination cell is written by one plain 2-byte store.
// DESIGN.md 4.6h.
#include "nq_kernels.h"

namespace nq {

namespace {

// the rows' running minima of one member column (rows past n_rows repeat row 0: loaded, never stored)
__device__ __forceinline__ void unite_fold(uint32_t (&acc)[kUniteRows], const uint16_t *col, uint64_t src_cap, uint32_t n_rows) {
  uint32_t v[kUniteRows];
#pragma unroll
  for (uint32_t r = 0; r < kUniteRows; ++r) v[r] = col[(uint64_t)(r < n_rows ? r : 0u) * src_cap];
#pragma unroll
  for (uint32_t r = 0; r < kUniteRows; ++r) acc[r] = v[r] < acc[r] ? v[r] : acc[r];
}

__device__ __forceinline__ uint32_t wave_min(uint32_t x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t y = __shfl_xor(x, o, 64);
    x = y < x ? y : x;
  }
  return x;
}

}  // namespace

__global__ __launch_bounds__(kUniteCols * kUniteWaves) void store_unite_kernel(const uint16_t *src, uint64_t src_cap, uint16_t *dst,
                                                                               uint64_t dst_cap, uint32_t f_local, uint32_t n_labels,
                                                                               const uint32_t *off, const uint32_t *members) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint64_t c = ((uint64_t)blockIdx.x * kUniteWaves + wave) * kUniteCols + lane;   // this lane's destination column
  const uint32_t r0 = blockIdx.y * kUniteRows;
  const uint32_t n_rows = f_local - r0 < kUniteRows ? f_local - r0 : kUniteRows;
  const uint16_t *s = src + (uint64_t)r0 * src_cap;
  uint32_t o = 0, sz = 0;
  if (c < n_labels) {
    o = off[c];
    sz = off[c + 1] - o;
  }
  uint32_t acc[kUniteRows];
#pragma unroll
  for (uint32_t r = 0; r < kUniteRows; ++r) acc[r] = kEmpty16;

  // lane route: this lane's own label, member after member
  const bool own = sz <= kUniteLaneMax;
  for (uint32_t j = 0; j < (own ? sz : 0u); ++j) unite_fold(acc, s + members[o + j], src_cap, n_rows);

  // wave route: the wavefront's larger labels in turn, lanes striding over the members; the label's own lane (which
  // folded nothing above) keeps the rows' minima
  unsigned long long todo = __ballot(!own);
  while (todo) {
    const uint32_t l = (uint32_t)__ffsll((long long)todo) - 1u;
    todo &= todo - 1ull;
    const uint32_t lo = __shfl(o, l, 64), lsz = __shfl(sz, l, 64);
    uint32_t part[kUniteRows];
#pragma unroll
    for (uint32_t r = 0; r < kUniteRows; ++r) part[r] = kEmpty16;
    for (uint32_t j = lane; j < lsz; j += 64) unite_fold(part, s + members[lo + j], src_cap, n_rows);
#pragma unroll
    for (uint32_t r = 0; r < kUniteRows; ++r) {
      const uint32_t m = wave_min(part[r]);
      if (lane == l) acc[r] = m;
    }
  }
  if (c < dst_cap) {
    uint16_t *d = dst + (uint64_t)r0 * dst_cap + c;
#pragma unroll
    for (uint32_t r = 0; r < kUniteRows; ++r)
      if (r < n_rows) d[(uint64_t)r * dst_cap] = (uint16_t)acc[r];
  }
}

hipError_t launch_store_unite(const uint16_t *src, uint64_t src_cap, uint16_t *dst, uint64_t dst_cap, uint32_t f_local, uint32_t n_labels,
                              const uint32_t *off, const uint32_t *members, hipStream_t stream) {
  if (f_local == 0 || dst_cap == 0) return hipSuccess;
  const uint32_t cols = kUniteCols * kUniteWaves;
  hipLaunchKernelGGL(store_unite_kernel, dim3((uint32_t)((dst_cap + cols - 1) / cols), (f_local + kUniteRows - 1) / kUniteRows),
                     dim3(cols), 0, stream, src, src_cap, dst, dst_cap, f_local, n_labels, off, members);
  return hipGetLastError();
}

}  // namespace nq
