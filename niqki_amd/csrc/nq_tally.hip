// nq_tally.hip -- the kernels of the taxon tally (nq_api_tally.hip): result rows (taxon, best_count, considered) of the
// LCA calls counted per taxon, and at read time every taxon's counts added to its ancestors'.  The rows are the LCA
// calls' own; nothing here looks at a hit or at the index.  Every loop is bounded by a count the host passes or by a
// table size: none waits for another thread, every barrier is reached by the whole workgroup, and a taxon is used as an
// index only after it was compared with n_taxa.  DESIGN.md 4.5g.
#include "nq_common.h"
#include "nq_kernels.h"

#include <hip/hip_runtime.h>

#include <algorithm>

namespace nq {

namespace {

constexpr uint32_t kTallyBlock = 256;
constexpr uint32_t kTallyRowsPerThread = kTallyPassRows / kTallyBlock;
constexpr uint32_t kTallySlotsLog2 = 11;
constexpr uint32_t kTallyEmpty = 0xFFFFFFFFu;   // (a classified row's taxon is below n_taxa < 0xFFFFFFFE)
constexpr uint32_t kTallyNoSlot = 0xFFFFFFFFu;
static_assert(kTallySlots == 1u << kTallySlotsLog2, "the table is a power of two");
static_assert(kTallyPassRows < kTallySlots, "a pass never fills the table");
static_assert(kTallyPassRows % kTallyBlock == 0, "every thread takes the same number of rows of a pass");

// the slot of taxon t, claimed if no row of the pass had it yet; at most kTallySlots probes (a pass has fewer rows)
__device__ __forceinline__ uint32_t tally_claim(uint32_t *keys, uint32_t t) {
  uint32_t s = (t * 2654435761u) >> (32u - kTallySlotsLog2);
  for (uint32_t n = 0; n < kTallySlots; ++n) {
    const uint32_t prev = atomicCAS(&keys[s], kTallyEmpty, t);
    if (prev == kTallyEmpty || prev == t) return s;
    s = (s + 1u) & (kTallySlots - 1u);
  }
  return kTallyNoSlot;
}

// A workgroup takes passes b, b + gridDim.x, ... of kTallyPassRows rows.  The classified rows of a pass are combined in
// an open-addressing table in LDS keyed by taxon -- LDS atomics on the slot's row count and 64-bit best sum -- and
// after a barrier every occupied slot goes out with ONE 64-bit global atomic per array and is cleared: however many
// rows of a pass share a taxon, the accumulator's L2 line sees one add.  Rows without a taxon and bad rows are counted
// in registers over all passes and leave the workgroup once.
__global__ __launch_bounds__(kTallyBlock) void tally_rows_kernel(TallyArgs a) {
  __shared__ uint32_t keys[kTallySlots], cnt[kTallySlots];
  __shared__ unsigned long long best[kTallySlots];
  __shared__ unsigned long long sh_words[kTallyWords];
  for (uint32_t s = threadIdx.x; s < kTallySlots; s += kTallyBlock) {
    keys[s] = kTallyEmpty;
    cnt[s] = 0;
    best[s] = 0;
  }
  if (threadIdx.x < kTallyWords) sh_words[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t n_pass = (uint32_t)(((uint64_t)a.n + kTallyPassRows - 1) / kTallyPassRows);
  uint32_t classified = 0, no_hit = 0, no_common = 0, bad = 0;
  for (uint32_t pass = blockIdx.x; pass < n_pass; pass += gridDim.x) {   // (uniform over the workgroup)
    const uint64_t base = (uint64_t)pass * kTallyPassRows;
    for (uint32_t k = 0; k < kTallyRowsPerThread; ++k) {
      const uint64_t i = base + (uint64_t)k * kTallyBlock + threadIdx.x;
      if (i >= a.n) continue;
      const uint32_t t = a.taxon[i];
      if (t < a.n_taxa) {
        const uint32_t s = tally_claim(keys, t);
        if (s == kTallyNoSlot) {   // (never: the table has more slots than the pass has rows)
          bad += 1;
          continue;
        }
        atomicAdd(&cnt[s], 1u);
        const uint32_t bc = a.best_count ? a.best_count[i] : 0u;
        if (bc) atomicAdd(&best[s], (unsigned long long)bc);
        classified += 1;
      } else if (t == kTaxonNone) {
        if (a.considered && a.considered[i] >= 1u) no_common += 1;
        else no_hit += 1;
      } else {
        bad += 1;
      }
    }
    __syncthreads();
    for (uint32_t s = threadIdx.x; s < kTallySlots; s += kTallyBlock) {
      const uint32_t t = keys[s];
      if (t == kTallyEmpty) continue;   // (t came out of tally_claim: below n_taxa)
      atomicAdd(a.direct + t, (unsigned long long)cnt[s]);
      if (best[s]) atomicAdd(a.direct_best + t, best[s]);
      keys[s] = kTallyEmpty;
      cnt[s] = 0;
      best[s] = 0;
    }
    __syncthreads();   // (the next pass claims slots only in a cleared table)
  }
  if (classified) atomicAdd(&sh_words[kTallyClassified], (unsigned long long)classified);
  if (no_hit) atomicAdd(&sh_words[kTallyNoHit], (unsigned long long)no_hit);
  if (no_common) atomicAdd(&sh_words[kTallyNoCommon], (unsigned long long)no_common);
  if (bad) atomicAdd(&sh_words[kTallyBad], (unsigned long long)bad);
  __syncthreads();
  if (threadIdx.x < kTallyWords && sh_words[threadIdx.x]) atomicAdd(a.words + threadIdx.x, sh_words[threadIdx.x]);
}

// A thread per taxon with rows of its own walks to its root and adds its two sums at every node on the way, itself
// included: clade[t] ends as the sum over t's subtree.  The walk ends at a self-parent and after max_depth + 1 nodes
// at the latest, whatever the nodes hold.
__global__ __launch_bounds__(kTallyBlock) void tally_clade_kernel(TallyCladeArgs a) {
  for (uint64_t t0 = (uint64_t)blockIdx.x * kTallyBlock + threadIdx.x; t0 < a.n_taxa; t0 += (uint64_t)gridDim.x * kTallyBlock) {
    const unsigned long long d = a.direct[t0];
    if (d == 0) continue;
    const unsigned long long b = a.direct_best[t0];
    uint32_t u = (uint32_t)t0;
    for (uint32_t step = 0; step <= a.max_depth; ++step) {
      atomicAdd(a.clade + u, d);
      if (b) atomicAdd(a.clade_best + u, b);
      const uint32_t p = a.nodes[u].parent;
      if (p == u || p >= a.n_taxa) break;
      u = p;
    }
  }
}

}  // namespace

hipError_t launch_tally_rows(const TallyArgs &a, hipStream_t stream) {
  if (a.n == 0) return hipSuccess;
  // a pass a workgroup and turn; no more workgroups than the device keeps resident (32 KiB of LDS each)
  const uint32_t n_pass = (uint32_t)(((uint64_t)a.n + kTallyPassRows - 1) / kTallyPassRows);
  const uint32_t blocks = std::min<uint32_t>(n_pass, 256u * 4u);
  hipLaunchKernelGGL(tally_rows_kernel, dim3(blocks), dim3(kTallyBlock), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_tally_clade(const TallyCladeArgs &a, hipStream_t stream) {
  if (a.n_taxa == 0) return hipSuccess;
  const uint32_t blocks = std::min<uint32_t>((a.n_taxa + kTallyBlock - 1) / kTallyBlock, 256u * 8u);
  hipLaunchKernelGGL(tally_clade_kernel, dim3(blocks), dim3(kTallyBlock), 0, stream, a);
  return hipGetLastError();
}

}  // namespace nq
