// nq_cover.hip -- the kernels of niqki_cover (nq_api_cover.hip): a round's picks, the compaction of the still-active
// queries, and the pick log turned into per-query lists.  Counts and winners come from the query path; nothing here
// counts or orders hits.  Every kernel is a bounded loop over its own rows: none waits for another.  DESIGN.md 4.5c.
#include "nq_common.h"
#include "nq_kernels.h"

#include <hip/hip_runtime.h>

namespace nq {

namespace {

constexpr uint32_t kCoverBlock = 256;
constexpr uint32_t kScanBlock = 1024;

// valid cell of a query sketch: Index::query_sketch, src/niqki_index.cpp:639
__device__ __forceinline__ bool cover_valid(int32_t v, uint32_t R) { return v >= 0 && (uint32_t)v < R; }

// One workgroup per active query i (row i of `masked`, query qidx[i] of the batch).  A query with a hit: its winner's
// store column against the original row (total) and against the masked row (those cells become -1), one log entry,
// flag[i] = it goes on.  A query without a hit: an entry without a pick, flag[i] = 0.
__global__ __launch_bounds__(kCoverBlock) void cover_pick_kernel(CoverPickArgs a) {
  __shared__ uint32_t sh_total, sh_masked;
  const uint32_t i = blockIdx.x;
  const uint32_t q = a.qidx[i];
  const unsigned long long h0 = a.hit_off[i], h1 = a.hit_off[i + 1];
  CoverPick *e = a.log + i;
  if (h1 <= h0) {   // (uniform over the workgroup)
    if (threadIdx.x == 0) {
      *e = CoverPick{q, kCoverNoPick, 0u, 0u, 0u};
      a.flag[i] = 0;
    }
    return;
  }
  const uint32_t count = a.hit_counts[h0], g = a.hit_gids[h0];
  if (g >= a.n_genomes) {   // never a column outside the store; the host ends the call
    if (threadIdx.x == 0) {
      *e = CoverPick{q, kCoverNoPick, 0u, 0u, 0u};
      a.flag[i] = 0;
      atomicAdd(a.info + kCoverInfoStuck, 1u);
    }
    return;
  }
  if (threadIdx.x == 0) {
    sh_total = 0;
    sh_masked = 0;
  }
  __syncthreads();
  const int32_t *orig = a.orig + (uint64_t)q * a.F;
  int32_t *masked = a.masked + (uint64_t)i * a.F;
  const uint16_t *col = a.store + g;
  uint32_t total = 0, n_masked = 0;
  for (uint32_t s = threadIdx.x; s < a.F; s += kCoverBlock) {
    const int32_t o = orig[s], m = masked[s];
    if (!cover_valid(o, a.R)) continue;   // (a masked cell is its original or -1)
    if (col[(uint64_t)s * a.cap] != (uint16_t)o) continue;
    total += 1;
    if (m == o) {
      masked[s] = -1;
      n_masked += 1;
    }
  }
  if (total) atomicAdd(&sh_total, total);
  if (n_masked) atomicAdd(&sh_masked, n_masked);
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t pos = a.n_picks[q];
    a.n_picks[q] = pos + 1;
    *e = CoverPick{q, pos, count, g, sh_total};
    const uint32_t nm = sh_masked, diff = nm > count ? nm - count : count - nm;
    if (diff) atomicAdd(a.info + kCoverInfoMismatch, diff);
    if (nm == 0) atomicAdd(a.info + kCoverInfoStuck, 1u);
    a.flag[i] = (a.max_picks == 0 || pos + 1 < a.max_picks) ? 1u : 0u;
    atomicAdd(a.info + kCoverInfoPicks, 1u);
  }
}

// exclusive scan of v[0 .. n) into out[0 .. n], out[n] = the sum; one workgroup
template <typename T>
__device__ void block_scan(const uint32_t *v, uint32_t n, T *out) {
  __shared__ unsigned long long part[kScanBlock];
  __shared__ unsigned long long carry;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (uint32_t base = 0; base < n; base += kScanBlock) {
    const uint32_t j = base + threadIdx.x;
    const unsigned long long x = j < n ? v[j] : 0ull;
    part[threadIdx.x] = x;
    __syncthreads();
    for (uint32_t d = 1; d < kScanBlock; d <<= 1) {
      const unsigned long long y = threadIdx.x >= d ? part[threadIdx.x - d] : 0ull;
      __syncthreads();
      part[threadIdx.x] += y;
      __syncthreads();
    }
    if (j < n) out[j] = (T)(carry + part[threadIdx.x] - x);
    __syncthreads();
    if (threadIdx.x == 0) carry += part[kScanBlock - 1];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[n] = (T)carry;
}

// the rows that go on: pos[i] = the row's place among them (query order is kept), info[kCoverInfoActive] = how many
__global__ __launch_bounds__(kScanBlock) void cover_compact_scan_kernel(const uint32_t *flag, uint32_t n, uint32_t *pos, uint32_t *info) {
  block_scan<uint32_t>(flag, n, pos);
  __syncthreads();
  if (threadIdx.x == 0) info[kCoverInfoActive] = pos[n];
}

// row i of the masked sketches and its query number to place pos[i] of the other buffer
__global__ __launch_bounds__(kCoverBlock) void cover_compact_kernel(const uint32_t *flag, const uint32_t *pos, const int32_t *src,
                                                                  const uint32_t *qidx_src, int32_t *dst, uint32_t *qidx_dst, uint32_t F) {
  const uint32_t i = blockIdx.x;
  if (!flag[i]) return;
  const uint32_t p = pos[i];
  const int32_t *s = src + (uint64_t)i * F;
  int32_t *d = dst + (uint64_t)p * F;
  for (uint32_t c = threadIdx.x; c < F; c += kCoverBlock) d[c] = s[c];
  if (threadIdx.x == 0) qidx_dst[p] = qidx_src[i];
}

__global__ __launch_bounds__(kCoverBlock) void cover_init_kernel(uint32_t *qidx, uint32_t *n_picks, uint32_t n) {
  const uint32_t i = blockIdx.x * kCoverBlock + threadIdx.x;
  if (i < n) {
    qidx[i] = i;
    n_picks[i] = 0;
  }
}

// per-query pick counts -> offsets
__global__ __launch_bounds__(kScanBlock) void cover_finish_kernel(const uint32_t *n_picks, uint32_t n, unsigned long long *hit_off) {
  block_scan<unsigned long long>(n_picks, n, hit_off);
}

// the log into the per-query lists: a query picks once a round, so its entries' `pos` are its list in round order
__global__ __launch_bounds__(kCoverBlock) void cover_scatter_kernel(const CoverPick *log, uint64_t n_log, const unsigned long long *hit_off,
                                                                  uint32_t *hit_counts, uint32_t *hit_gids, uint32_t *hit_totals,
                                                                  uint64_t capacity) {
  const uint64_t j = (uint64_t)blockIdx.x * kCoverBlock + threadIdx.x;
  if (j >= n_log) return;
  const CoverPick e = log[j];
  if (e.pos == kCoverNoPick) return;
  const unsigned long long p = hit_off[e.q] + e.pos;
  if (p >= capacity) return;
  hit_counts[p] = e.count;
  hit_gids[p] = e.gid;
  if (hit_totals) hit_totals[p] = e.total;
}

}  // namespace

hipError_t launch_cover_init(uint32_t *qidx, uint32_t *n_picks, uint32_t n, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(cover_init_kernel, dim3((n + kCoverBlock - 1) / kCoverBlock), dim3(kCoverBlock), 0, stream, qidx, n_picks, n);
  return hipGetLastError();
}

hipError_t launch_cover_pick(const CoverPickArgs &a, uint32_t n_active, hipStream_t stream) {
  if (n_active == 0) return hipSuccess;
  hipLaunchKernelGGL(cover_pick_kernel, dim3(n_active), dim3(kCoverBlock), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_cover_compact_scan(const uint32_t *flag, uint32_t n_active, uint32_t *pos, uint32_t *info, hipStream_t stream) {
  hipLaunchKernelGGL(cover_compact_scan_kernel, dim3(1), dim3(kScanBlock), 0, stream, flag, n_active, pos, info);
  return hipGetLastError();
}

hipError_t launch_cover_compact(const uint32_t *flag, const uint32_t *pos, const int32_t *src, const uint32_t *qidx_src, int32_t *dst,
                                uint32_t *qidx_dst, uint32_t F, uint32_t n_active, hipStream_t stream) {
  if (n_active == 0) return hipSuccess;
  hipLaunchKernelGGL(cover_compact_kernel, dim3(n_active), dim3(kCoverBlock), 0, stream, flag, pos, src, qidx_src, dst, qidx_dst, F);
  return hipGetLastError();
}

hipError_t launch_cover_finish(const uint32_t *n_picks, uint32_t n, unsigned long long *hit_off, hipStream_t stream) {
  hipLaunchKernelGGL(cover_finish_kernel, dim3(1), dim3(kScanBlock), 0, stream, n_picks, n, hit_off);
  return hipGetLastError();
}

hipError_t launch_cover_scatter(const CoverPick *log, uint64_t n_log, const unsigned long long *hit_off, uint32_t *hit_counts,
                                uint32_t *hit_gids, uint32_t *hit_totals, uint64_t capacity, hipStream_t stream) {
  if (n_log == 0) return hipSuccess;
  hipLaunchKernelGGL(cover_scatter_kernel, dim3((uint32_t)((n_log + kCoverBlock - 1) / kCoverBlock)), dim3(kCoverBlock), 0, stream, log,
                     n_log, hit_off, hit_counts, hit_gids, hit_totals, capacity);
  return hipGetLastError();
}

}  // namespace nq
