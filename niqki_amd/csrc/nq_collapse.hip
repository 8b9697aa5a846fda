// nq_collapse.hip -- the kernels of niqki_query_collapsed (nq_api_collapse.hip): which entries of a query's ordered
// hit list are the first of their label, how many members each label has in the list, and those entries written out in
// list order.  Counts, threshold, order and ties come from the query path; nothing here counts or orders hits, and
// nothing sorts.  Every loop is bounded by its list or its table: none waits for another thread.  DESIGN.md 4.5d.
#include "nq_common.h"
#include "nq_kernels.h"

#include <hip/hip_runtime.h>

#include <algorithm>

namespace nq {

namespace {

constexpr uint32_t kCollapseBlock = 256;
constexpr uint32_t kCollapseScanBlock = 1024;
constexpr uint32_t kEmptyKey = 0xFFFFFFFFu;   // (a dense label id is below the genome count)
constexpr uint32_t kNoSlot = 0xFFFFFFFFu;
constexpr unsigned long long kClearedEntry = 0x00000000FFFFFFFFull;   // {first = 0xFFFFFFFF, members = 0}

// the table a list of len entries takes: at least two slots an entry, a power of two, 64 or more
__device__ __forceinline__ uint32_t table_log2(uint32_t len) {
  const uint32_t lg = 32u - (uint32_t)__clz((int)(2u * len - 1u));
  return lg < 6u ? 6u : lg;
}

__device__ __forceinline__ uint32_t table_home(uint32_t d, uint32_t lg) { return (d * 2654435761u) >> (32u - lg); }

// the slot of label d, claimed if no entry had it yet; at most `slots` probes (the table is never more than half full)
__device__ __forceinline__ uint32_t table_claim(uint32_t *keys, uint32_t d, uint32_t lg) {
  const uint32_t slots = 1u << lg, mask = slots - 1u;
  uint32_t s = table_home(d, lg);
  for (uint32_t n = 0; n < slots; ++n) {
    const uint32_t prev = atomicCAS(&keys[s], kEmptyKey, d);
    if (prev == kEmptyKey || prev == d) return s;
    s = (s + 1u) & mask;
  }
  return kNoSlot;
}

__device__ __forceinline__ uint32_t table_find(const uint32_t *keys, uint32_t d, uint32_t lg) {
  const uint32_t slots = 1u << lg, mask = slots - 1u;
  uint32_t s = table_home(d, lg);
  for (uint32_t n = 0; n < slots; ++n) {
    const uint32_t k = keys[s];
    if (k == d) return s;
    if (k == kEmptyKey) return kNoSlot;
    s = (s + 1u) & mask;
  }
  return kNoSlot;
}

// Workgroup b takes queries b, b + gridDim.x, ... and owns global table b.  Per query: kept[e] = the members of the
// entry's label in the list where entry e is the first of its label, 0 elsewhere; n_kept[q] = the kept entries, cut to
// top_k.  A list of at most lds_cap entries goes through an open-addressing table in LDS keyed by the dense label id;
// a longer one through the workgroup's direct-indexed table in global memory, which it leaves cleared by walking the
// list again.
__global__ __launch_bounds__(kCollapseBlock) void collapse_first_kernel(CollapseArgs a) {
  extern __shared__ uint32_t lds[];
  __shared__ uint32_t sh_kept;
  uint32_t *keys = lds, *first = lds + a.lds_slots, *memb = first + a.lds_slots;
  unsigned long long *tab = a.tables ? a.tables + (uint64_t)blockIdx.x * a.n_labels : nullptr;
  if (threadIdx.x == 0) sh_kept = 0;
  for (uint32_t q = blockIdx.x; q < a.nq; q += gridDim.x) {
    const unsigned long long h0 = a.hit_off[q], h1 = a.hit_off[q + 1];
    // (uniform over the workgroup from here on: every barrier is reached by all its threads)
    if (h1 <= h0) {
      if (threadIdx.x == 0) a.n_kept[q] = 0;
      continue;
    }
    if (h1 - h0 > a.n_genomes) {   // never a position a table cannot hold; the host ends the call
      if (threadIdx.x == 0) {
        a.n_kept[q] = 0;
        atomicAdd(a.info + kCollapseInfoBad, 1u);
      }
      continue;
    }
    const uint32_t len = (uint32_t)(h1 - h0);
    const uint32_t *gids = a.hit_gids + h0;
    uint32_t *kept = a.kept + h0;
    uint32_t mine = 0, bad = 0;
    if (len <= a.lds_cap) {
      const uint32_t lg = table_log2(len), slots = 1u << lg;   // (slots <= lds_slots: len <= lds_cap)
      for (uint32_t s = threadIdx.x; s < slots; s += kCollapseBlock) {
        keys[s] = kEmptyKey;
        first[s] = 0xFFFFFFFFu;
        memb[s] = 0;
      }
      __syncthreads();
      for (uint32_t pos = threadIdx.x; pos < len; pos += kCollapseBlock) {
        const uint32_t g = gids[pos];
        const uint32_t s = g < a.n_genomes ? table_claim(keys, a.dense[g], lg) : kNoSlot;
        if (s == kNoSlot) {
          bad += 1;
          continue;
        }
        atomicMin(&first[s], pos);
        atomicAdd(&memb[s], 1u);
      }
      __syncthreads();
      for (uint32_t pos = threadIdx.x; pos < len; pos += kCollapseBlock) {
        const uint32_t g = gids[pos];
        const uint32_t s = g < a.n_genomes ? table_find(keys, a.dense[g], lg) : kNoSlot;
        const bool k = s != kNoSlot && first[s] == pos;
        kept[pos] = k ? memb[s] : 0u;
        mine += k ? 1u : 0u;
      }
    } else if (tab) {
      if (threadIdx.x == 0) atomicAdd(a.info + kCollapseInfoLong, 1u);
      uint32_t *tab32 = (uint32_t *)tab;   // entry d: word 2d = first position, word 2d + 1 = members
      for (uint32_t pos = threadIdx.x; pos < len; pos += kCollapseBlock) {
        const uint32_t g = gids[pos];
        const uint32_t d = g < a.n_genomes ? a.dense[g] : a.n_labels;
        if (d >= a.n_labels) {
          bad += 1;
          continue;
        }
        atomicMin(&tab32[2 * (uint64_t)d], pos);
        atomicAdd(&tab32[2 * (uint64_t)d + 1], 1u);
      }
      __threadfence();
      __syncthreads();
      // (the table is read where the atomics wrote it: loads that a line cached for an earlier query cannot answer)
      for (uint32_t pos = threadIdx.x; pos < len; pos += kCollapseBlock) {
        const uint32_t g = gids[pos];
        const uint32_t d = g < a.n_genomes ? a.dense[g] : a.n_labels;
        bool k = false;
        if (d < a.n_labels)
          k = __hip_atomic_load(&tab32[2 * (uint64_t)d], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == pos;
        kept[pos] = k ? __hip_atomic_load(&tab32[2 * (uint64_t)d + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
        mine += k ? 1u : 0u;
      }
      __syncthreads();
      for (uint32_t pos = threadIdx.x; pos < len; pos += kCollapseBlock) {
        const uint32_t g = gids[pos];
        const uint32_t d = g < a.n_genomes ? a.dense[g] : a.n_labels;
        if (d < a.n_labels) __hip_atomic_store(&tab[d], kClearedEntry, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      __threadfence();
    } else {   // a long list and no table: the host sized the workspace wrongly
      bad = threadIdx.x == 0 ? 1u : 0u;
    }
    if (mine) atomicAdd(&sh_kept, mine);
    if (bad) atomicAdd(a.info + kCollapseInfoBad, bad);
    __syncthreads();
    if (threadIdx.x == 0) {
      const uint32_t n = sh_kept;
      a.n_kept[q] = a.top_k && n > a.top_k ? a.top_k : n;
      sh_kept = 0;   // (the next query adds to it only behind a barrier)
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kCollapseBlock) void collapse_table_init_kernel(unsigned long long *tab, uint64_t n) {
  for (uint64_t i = (uint64_t)blockIdx.x * kCollapseBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kCollapseBlock)
    tab[i] = kClearedEntry;
}

// off[0 .. n] = exclusive scan of v[0 .. n), off[n] = the sum; one workgroup
__global__ __launch_bounds__(kCollapseScanBlock) void collapse_scan_kernel(const uint32_t *v, uint32_t n, unsigned long long *off) {
  __shared__ unsigned long long part[kCollapseScanBlock];
  __shared__ unsigned long long carry;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (uint32_t base = 0; base < n; base += kCollapseScanBlock) {
    const uint32_t j = base + threadIdx.x;
    const unsigned long long x = j < n ? v[j] : 0ull;
    part[threadIdx.x] = x;
    __syncthreads();
    for (uint32_t d = 1; d < kCollapseScanBlock; d <<= 1) {
      const unsigned long long y = threadIdx.x >= d ? part[threadIdx.x - d] : 0ull;
      __syncthreads();
      part[threadIdx.x] += y;
      __syncthreads();
    }
    if (j < n) off[j] = carry + part[threadIdx.x] - x;
    __syncthreads();
    if (threadIdx.x == 0) carry += part[kCollapseScanBlock - 1];
    __syncthreads();
  }
  if (threadIdx.x == 0) off[n] = carry;
}

// One workgroup per query: its kept entries, in list order, to out[off[q] ...), the first n_kept[q] of them.  A chunk of
// 256 entries gets its ranks from the waves' ballots; the walk ends where the cut is reached.
__global__ __launch_bounds__(kCollapseBlock) void collapse_emit_kernel(const unsigned long long *hit_off, const uint32_t *hit_counts,
                                                                     const uint32_t *hit_gids, const uint32_t *kept,
                                                                     const uint32_t *n_kept, const unsigned long long *off,
                                                                     CollapsedHit *out) {
  __shared__ uint32_t wave_n[kCollapseBlock / 64];
  const uint32_t q = blockIdx.x;
  const uint32_t limit = n_kept[q];
  if (limit == 0) return;   // (uniform)
  const unsigned long long h0 = hit_off[q];
  const uint32_t len = (uint32_t)(hit_off[q + 1] - h0);
  CollapsedHit *dst = out + off[q];
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  uint32_t done = 0;
  for (uint32_t c0 = 0; c0 < len && done < limit; c0 += kCollapseBlock) {
    const uint32_t pos = c0 + threadIdx.x;
    const uint32_t km = pos < len ? kept[h0 + pos] : 0u;
    const unsigned long long ballot = __ballot(km != 0);
    if (lane == 0) wave_n[w] = (uint32_t)__popcll(ballot);
    __syncthreads();
    uint32_t before = 0, total = 0;
    for (uint32_t i = 0; i < kCollapseBlock / 64; ++i) {
      before += i < w ? wave_n[i] : 0u;
      total += wave_n[i];
    }
    const uint32_t r = done + before + (uint32_t)__popcll(ballot & ((1ull << lane) - 1ull));
    if (km && r < limit) dst[r] = CollapsedHit{hit_counts[h0 + pos], hit_gids[h0 + pos], km};
    done += total;
    __syncthreads();
  }
}

__global__ __launch_bounds__(kCollapseBlock) void collapse_unpack_kernel(const CollapsedHit *in, uint64_t n, uint32_t *hit_counts,
                                                                       uint32_t *hit_gids, uint32_t *hit_members) {
  const uint64_t j = (uint64_t)blockIdx.x * kCollapseBlock + threadIdx.x;
  if (j >= n) return;
  const CollapsedHit e = in[j];
  hit_counts[j] = e.count;
  hit_gids[j] = e.gid;
  if (hit_members) hit_members[j] = e.members;
}

}  // namespace

uint32_t collapse_lds_slots(uint32_t lds_cap) {
  uint32_t s = 64;
  while (s < 2 * lds_cap) s *= 2;
  return s;
}

hipError_t launch_collapse_first(const CollapseArgs &a, uint32_t n_blocks, hipStream_t stream) {
  if (a.nq == 0 || n_blocks == 0) return hipSuccess;
  const size_t lds = (size_t)a.lds_slots * 12;
  if (lds > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void *)collapse_first_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(collapse_first_kernel, dim3(n_blocks), dim3(kCollapseBlock), lds, stream, a);
  return hipGetLastError();
}

hipError_t launch_collapse_table_init(unsigned long long *tables, uint64_t n_entries, hipStream_t stream) {
  if (n_entries == 0) return hipSuccess;
  const uint32_t blocks = (uint32_t)std::min<uint64_t>((n_entries + kCollapseBlock - 1) / kCollapseBlock, 4096);
  hipLaunchKernelGGL(collapse_table_init_kernel, dim3(blocks), dim3(kCollapseBlock), 0, stream, tables, n_entries);
  return hipGetLastError();
}

hipError_t launch_collapse_scan(const uint32_t *n_kept, uint32_t n, unsigned long long *off, hipStream_t stream) {
  hipLaunchKernelGGL(collapse_scan_kernel, dim3(1), dim3(kCollapseScanBlock), 0, stream, n_kept, n, off);
  return hipGetLastError();
}

hipError_t launch_collapse_emit(const unsigned long long *hit_off, const uint32_t *hit_counts, const uint32_t *hit_gids, const uint32_t *kept,
                                const uint32_t *n_kept, const unsigned long long *off, uint32_t n, CollapsedHit *out, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(collapse_emit_kernel, dim3(n), dim3(kCollapseBlock), 0, stream, hit_off, hit_counts, hit_gids, kept, n_kept, off, out);
  return hipGetLastError();
}

hipError_t launch_collapse_unpack(const CollapsedHit *in, uint64_t n, uint32_t *hit_counts, uint32_t *hit_gids, uint32_t *hit_members,
                                  hipStream_t stream) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(collapse_unpack_kernel, dim3((uint32_t)((n + kCollapseBlock - 1) / kCollapseBlock)), dim3(kCollapseBlock), 0, stream, in,
                     n, hit_counts, hit_gids, hit_members);
  return hipGetLastError();
}

}  // namespace nq
