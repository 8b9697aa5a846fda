// nq_probe.hip -- the ceilings the bench measures the sketch kernels against (niqki_measure_alu, niqki_hip_bench.h):
// integer-ALU and streaming-copy probes, and the LDS round trips of a densification pass.
#include "nq_kernels.h"
#include "nq_sketch_ops.h"

namespace nq {

// ---- integer-ALU ceiling probes ---------------------------------------------------------------
template <int WHAT>
__global__ __launch_bounds__(1024) void alu_probe_kernel(uint32_t iters, uint32_t *sink) {
  const uint32_t t = blockIdx.x * 1024u + threadIdx.x;
  if (WHAT == 2) {
    // the long-record path's arithmetic per k-mer as the kernel does it (K = 31): rolling update of both
    // words from pre-placed codes, canonical choice, high word of revhash64 as v_mad_u64_u32 chains and
    // the filter compare; 16 k-mers per round
    uint64_t fw = t * 0x9E3779B97F4A7C15ULL, rc = ~fw;
    fw &= (1ULL << 62) - 1; rc &= (1ULL << 62) - 1;
    uint32_t e = t * 2654435761u, pass = 0;
    for (uint32_t i = 0; i < iters; ++i) {
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const uint32_t c = (e >> (2 * j)) & 3u;
        const uint64_t ent = ((uint64_t)((3u - c) << 30) << 32) | c;   // a code table entry
        rc = shr2_64(rc | (ent & 0xFFFFFFFF00000000ULL));
        fw = shl2_add64(fw, ent) & ((1ULL << 62) - 1ULL);
        const uint64_t canon = min62(fw, rc);
        pass += rev64_hi_mad(canon) < (1u << 29);
      }
      e = e * 1664525u + 1013904223u;
    }
    if (pass == 0xFFFFFFFFu) sink[0] = pass;
  } else if (WHAT == 3) {
    // a three-operand integer instruction (v_lshl_add_u32): the issue rate of every vector opcode outside the
    // add / sub / and / or / xor / mov / shift-right class on gfx950 (profiles/r03_opcode_costs.txt)
    uint32_t a0 = t, a1 = t * 3 + 1, a2 = t ^ 0x1234567, a3 = t + 77, a4 = t * 5, a5 = ~t, a6 = t + 9, a7 = t * 7;
    for (uint32_t i = 0; i < iters; ++i) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
#define NQ_LA(x, y) asm volatile("v_lshl_add_u32 %0, %0, 3, %1" : "+v"(x) : "v"(y))
        NQ_LA(a0, a1); NQ_LA(a1, a2); NQ_LA(a2, a3); NQ_LA(a3, a4); NQ_LA(a4, a5); NQ_LA(a5, a6); NQ_LA(a6, a7); NQ_LA(a7, a0);
#undef NQ_LA
      }
    }
    const uint32_t x = a0 ^ a1 ^ a2 ^ a3 ^ a4 ^ a5 ^ a6 ^ a7;
    if (x == 0x12345u) sink[0] = x;
  } else {
    uint32_t a0 = t, a1 = t * 3 + 1, a2 = t ^ 0x1234567, a3 = t + 77, a4 = t * 5, a5 = ~t, a6 = t + 9, a7 = t * 7;
    for (uint32_t i = 0; i < iters; ++i) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (WHAT == 0) { a0 += a1; a1 += a2; a2 += a3; a3 += a4; a4 += a5; a5 += a6; a6 += a7; a7 += a0; }
        else { a0 *= a1; a1 *= a2; a2 *= a3; a3 *= a4; a4 *= a5; a5 *= a6; a6 *= a7; a7 *= (a0 | 1u); }  // data dependent: nothing folds
      }
    }
    const uint32_t x = a0 ^ a1 ^ a2 ^ a3 ^ a4 ^ a5 ^ a6 ^ a7;
    if (x == 0x12345u) sink[0] = x;
  }
}

// streaming copy: the HBM rate a kernel reaches on this device (the practical ceiling beside the spec peak).
// Four 16-byte nontemporal loads in flight per thread, one workgroup per 16 KB: the fastest of the forms in
// tools/ubench_copy.hip (6.2 TB/s; a plain one-load loop 4.8, hipMemcpyAsync 4.7).
typedef unsigned int copy_u4 __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void copy_probe_kernel(const copy_u4 *src, copy_u4 *dst, uint64_t n) {
  const uint64_t step = (uint64_t)gridDim.x * 1024;
  for (uint64_t i = (uint64_t)blockIdx.x * 1024 + threadIdx.x; i < n; i += step) {
    copy_u4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (i + u * 256 < n) v[u] = __builtin_nontemporal_load(src + i + u * 256);
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (i + u * 256 < n) __builtin_nontemporal_store(v[u], dst + i + u * 256);
  }
}
hipError_t launch_copy_probe(const void *src, void *dst, uint64_t bytes, hipStream_t stream) {
  hipLaunchKernelGGL(copy_probe_kernel, dim3(32768), dim3(256), 0, stream, (const copy_u4 *)src, (copy_u4 *)dst, bytes / 16);
  return hipGetLastError();
}

// The short-read kernel's densification passes with nothing but their LDS traffic and exit test: one wavefront per
// workgroup with the 150-base kernel's LDS footprint (the F = 4096 cells + entry list + code tile: 8 workgroups per
// CU), two register entries per lane (a 150-base read has ~120 occupied cells), per pass two ds_min_u32 proposals
// to pseudo-random cells, their read-backs behind them in issue order, a ballot + popcount and the advance of the
// targets -- the plain pass (every entry proposing) without winner writes.  The rate of these passes is the ceiling the passes of
// sketch_reads_kernel are measured against (LDS round-trip latency at 8 waves per CU).
__global__ __launch_bounds__(64) void lds_pass_probe_kernel(uint32_t iters, uint32_t *sink) {
  extern __shared__ __align__(16) uint32_t smem[];
  const uint32_t F = 4096, Fm = F - 1u, lane = threadIdx.x;
  for (uint32_t i = lane; i < F; i += 64) smem[i] = kEmpty32;
  __syncthreads();
  uint32_t T[2], B[2], mk[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const uint32_t v = (blockIdx.x * 131u + lane * 2u + (uint32_t)k) * 2654435761u;
    T[k] = (uint32_t)unrev64(v);
    B[k] = (uint32_t)rev64(v) | 1u;
    mk[k] = 0x80000000u | ((lane * 2u + (uint32_t)k) & Fm);
  }
  uint32_t tot = 0;
  for (uint32_t it = 0; it < iters; ++it) {
#pragma unroll
    for (int k = 0; k < 2; ++k) atomicMin(&smem[T[k] & Fm], mk[k]);
    wave_lds_order();
    uint32_t back[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) back[k] = smem[T[k] & Fm];
    wave_lds_order();
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      tot += (uint32_t)__popcll(__ballot(back[k] == mk[k]));
      T[k] += B[k];
    }
    if (tot == 0xFFFFFFFFu) break;   // (the exit test of a pass; never taken)
  }
  if (tot == 0x12345u) sink[0] = tot;
}

hipError_t launch_alu_probe(int what, uint32_t iters, uint32_t *sink, uint64_t *units, hipStream_t stream) {
  if (what == 5) {
    const uint32_t blocks = 256 * 9 * 4;   // four rounds of 9 one-wave workgroups per CU
    const size_t lds = 4096 * 4 + 192 * 8;   // sketch_reads_lds_bytes at S = 12 for 150-base reads
    hipLaunchKernelGGL(lds_pass_probe_kernel, dim3(blocks), dim3(64), lds, stream, iters * 16, sink);
    *units = (uint64_t)blocks * iters * 16;
    return hipGetLastError();
  }
  const uint32_t blocks = 256 * 4;  // four 1024-thread workgroups per CU: 16 waves per SIMD-quartet, as the sketch kernel
  const uint64_t threads = (uint64_t)blocks * 1024;
  if (what == 0) { hipLaunchKernelGGL(alu_probe_kernel<0>, dim3(blocks), dim3(1024), 0, stream, iters, sink); *units = threads * iters * 64; }
  else if (what == 1) { hipLaunchKernelGGL(alu_probe_kernel<1>, dim3(blocks), dim3(1024), 0, stream, iters, sink); *units = threads * iters * 64; }
  else if (what == 2) { hipLaunchKernelGGL(alu_probe_kernel<2>, dim3(blocks), dim3(1024), 0, stream, iters, sink); *units = threads * iters * 16; }
  else if (what == 3) { hipLaunchKernelGGL(alu_probe_kernel<3>, dim3(blocks), dim3(1024), 0, stream, iters, sink); *units = threads * iters * 64; }
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

}  // namespace nq
