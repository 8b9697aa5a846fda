// nq_order.hip -- the locality order of a query batch, for gfx950: probe_kernel, order_kernel and launch_order.
#include "nq_kernels.h"

namespace nq {

// ---- locality order of a query batch -----------------------------------------------------
// Queries that hit the same genomes read the same table and bucket lines.  When they run on
// the same XCD at the same time those lines are fetched from HBM once (measured: 13 % off the
// launch when the 4 queries of a family sit 8 blocks apart).  So a batch is ordered by its
// best probable hit: probe_kernel counts the first kProbeSlots slots only and takes the genome
// with the most hits as the query's key, order_kernel sorts (key, query), and gather_kernel
// maps sorted neighbours to one XCD.  Only the order of the work changes, never a result.
// (kOrderGroup, kOrderMax: nq_gather_plan.h)
constexpr uint32_t kProbeSlots = 16;

// Counters per block of kProbeBlock consecutive genomes (a key only has to bring the queries of one
// family together): a few KB of LDS instead of the gather kernel's whole tile, so many probes share
// a CU and hide each other's three dependent memory round trips (sketch -> entry -> ids).
constexpr uint32_t kProbeBlock = 64;
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void probe_kernel(IndexView v, const int32_t *sketches, uint32_t *keys) {
  extern __shared__ __align__(16) uint32_t cnt[];
  __shared__ uint32_t s_best;
  const uint32_t q = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const int32_t *sk = sketches + (uint64_t)q * v.q_stride + v.q_off;
  const uint32_t n_probe = v.f_local < kProbeSlots ? v.f_local : kProbeSlots;
  const uint32_t n_blocks = (v.n_genomes + kProbeBlock - 1) / kProbeBlock;
  if (tid == 0) s_best = 0;
  for (uint32_t i = tid; i < n_blocks; i += BLOCK) cnt[i] = 0;
  __syncthreads();
  for (uint32_t w = wave; w < n_probe * v.n_tiles; w += BLOCK / 64) {
    const uint32_t s = w / v.n_tiles, t = w % v.n_tiles;
    const int32_t fp = sk[s];
    if (fp < 0 || (uint32_t)fp >= v.d.R) continue;  // wave uniform
    const Entry e = v.entries[((uint64_t)s * v.d.R + (uint32_t)fp) * v.n_tiles + t];
    const uint16_t *b = v.gids + v.tile_base[t] + ((uint64_t)e.start << v.align_log2);
    for (uint32_t o = lane; o < e.len; o += 64) atomicAdd(&cnt[tile_gid(v, t, b[o]) / kProbeBlock], 1u);
  }
  __syncthreads();
  uint32_t best = 0;  // count << 20 | block
  for (uint32_t i = tid; i < n_blocks; i += BLOCK) {
    const uint32_t c = cnt[i] < 4095u ? cnt[i] : 4095u;
    const uint32_t a = (c << 20) | i;
    best = best > a ? best : a;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t y = __shfl_xor(best, o, 64);
    best = best > y ? best : y;
  }
  if (lane == 0) atomicMax(&s_best, best);
  __syncthreads();
  if (tid == 0) {
    const uint32_t c = s_best >> 20;
    const uint32_t key = c >= 2 ? (s_best & 0xFFFFFu) : 0xFFFFFu;  // unrelated queries: one group at the end
    keys[q] = (key << 12) | q;
  }
}

// keys[0..nq) -> order[0..nq): ascending (key, query index); one workgroup, bitonic in LDS
__global__ __launch_bounds__(1024) void order_kernel(const uint32_t *keys, uint32_t nq, uint32_t *order) {
  __shared__ uint32_t a[kOrderMax];
  const uint32_t tid = threadIdx.x;
  for (uint32_t i = tid; i < kOrderMax; i += 1024) a[i] = i < nq ? keys[i] : 0xFFFFFFFFu;
  __syncthreads();
  for (uint32_t k = 2; k <= kOrderMax; k <<= 1) {
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      for (uint32_t i = tid; i < kOrderMax; i += 1024) {
        const uint32_t l = i ^ j;
        if (l > i) {
          const uint32_t x = a[i], y = a[l];
          const bool up = (i & k) == 0;
          if ((x > y) == up) { a[i] = y; a[l] = x; }
        }
      }
      __syncthreads();
    }
  }
  for (uint32_t i = tid; i < nq; i += 1024) order[i] = a[i] & 0xFFFu;
}

hipError_t launch_order(const IndexView &v, const int32_t *sketches, uint32_t nq, uint32_t *keys,
                        uint32_t *order, hipStream_t stream) {
  if (nq == 0 || nq > kOrderMax || v.n_genomes >= kOrderMaxGenomes) return hipErrorInvalidValue;
  const size_t lds = (size_t)((v.n_genomes + kProbeBlock - 1) / kProbeBlock) * 4;   // <= 64 KB (n_genomes < 2^20)
  hipError_t e = hipFuncSetAttribute((const void *)probe_kernel<256>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(probe_kernel<256>, dim3(nq), dim3(256), lds, stream, v, sketches, keys);
  hipLaunchKernelGGL(order_kernel, dim3(1), dim3(1024), 0, stream, keys, nq, order);
  return hipGetLastError();
}

}  // namespace nq
