// nq_lca.hip -- the kernel of niqki_query_lca (nq_api_lca.hip): per query the considered prefix of its ordered hit list
// (the entries within top_permille of the best count) and the lowest common ancestor of those genomes' taxa.  Counts,
// threshold, order and ties come from the query path; nothing here counts or orders hits.  Every loop is bounded: the
// search by 6 steps, a walk up the tree by the taxonomy's depth, a fold by its list.  None waits for another thread.
// DESIGN.md 4.5e.
#include "nq_common.h"
#include "nq_kernels.h"

#include <hip/hip_runtime.h>

#include <algorithm>

namespace nq {

namespace {

constexpr uint32_t kLcaBlock = 256;
constexpr uint32_t kLcaWaves = kLcaBlock / 64;
constexpr uint32_t kLcaNothing = 0xFFFFFFFEu;   // the fold's identity: no taxon seen yet (n_taxa is below it)
constexpr uint32_t kLcaNoQuery = 0xFFFFFFFFu;

// the node of taxon t; one beyond the taxonomy counts as bad and reads as a root
__device__ __forceinline__ TaxNode lca_node(const LcaArgs &a, uint32_t t, uint32_t &bad) {
  if (t >= a.n_taxa) {
    bad += 1;
    return TaxNode{t, 0};
  }
  return a.nodes[t];
}

// The deepest common ancestor-or-self of x and y, kTaxonNone where they lie in two trees.  The deeper one is lifted to
// the other's depth, then both a level at a time until they meet or depth 0 is reached.  Lanes of a wavefront walk
// different distances: the loops run as long as the longest of them, at most max_depth steps each.
__device__ __forceinline__ uint32_t lca_pair(const LcaArgs &a, uint32_t x, uint32_t y, uint32_t &bad) {
  if (x == kLcaNothing) return y;
  if (y == kLcaNothing) return x;
  if (x == kTaxonNone || y == kTaxonNone) return kTaxonNone;
  if (x == y) return x;
  uint32_t dx = min(lca_node(a, x, bad).depth, a.max_depth), dy = min(lca_node(a, y, bad).depth, a.max_depth);
  for (uint32_t i = 0; i < a.max_depth && dx > dy; ++i) {
    x = lca_node(a, x, bad).parent;
    dx -= 1;
  }
  for (uint32_t i = 0; i < a.max_depth && dy > dx; ++i) {
    y = lca_node(a, y, bad).parent;
    dy -= 1;
  }
  for (uint32_t i = 0; i < a.max_depth && x != y && dx > 0; ++i) {
    x = lca_node(a, x, bad).parent;
    y = lca_node(a, y, bad).parent;
    dx -= 1;
  }
  return x == y ? x : kTaxonNone;
}

// the taxon of list entry gids[i]
__device__ __forceinline__ uint32_t lca_leaf_taxon(const LcaArgs &a, const uint32_t *gids, uint32_t i, uint32_t &bad) {
  const uint32_t g = gids[i];
  if (g >= a.n_genomes) {
    bad += 1;
    return kLcaNothing;
  }
  return a.genome_taxon[g];
}

// all 64 lanes' accumulators into every lane
__device__ __forceinline__ uint32_t lca_wave_reduce(const LcaArgs &a, uint32_t acc, uint32_t &bad) {
  for (uint32_t s = 32; s > 0; s >>= 1) {
    const uint32_t o = (uint32_t)__shfl_xor((int)acc, (int)s, 64);
    acc = lca_pair(a, acc, o, bad);
  }
  return acc;
}

// entries first, first + step, ... below m of the list folded by this lane; the wavefront stops once no lane of it can
// change any more (every accumulator is the absorbing kTaxonNone)
__device__ __forceinline__ uint32_t lca_fold(const LcaArgs &a, const uint32_t *gids, uint32_t first, uint32_t step, uint32_t m, uint32_t &bad) {
  uint32_t acc = kLcaNothing;
  const uint32_t lane = threadIdx.x & 63u;
  for (uint32_t base = first - lane; base < m; base += step) {   // (base is the wavefront's: the trip count is uniform)
    const uint32_t i = base + lane;
    if (i < m) acc = lca_pair(a, acc, lca_leaf_taxon(a, gids, i, bad), bad);
    if (__ballot(acc != kTaxonNone) == 0ull) break;
  }
  return acc;
}

// How many leading entries of the ordered counts[0 .. len) are considered.  Entry 0 is (it is the best); the 64 lanes
// probe evenly spaced positions of what is still unknown and a ballot keeps the one gap that holds the boundary, so
// the unknown range shrinks 64-fold a step: 6 steps settle any 32-bit length.
__device__ __forceinline__ uint32_t lca_considered(const uint32_t *counts, uint32_t len, unsigned long long floor1000) {
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t lo = 0, hi = len;   // entry lo is considered, entry hi is not (hi = len: the end)
  for (uint32_t s = 0; s < 6 && hi - lo > 1; ++s) {
    const uint32_t span = hi - lo - 1;           // positions lo + 1 .. hi - 1 are unknown
    const uint32_t step = (span + 63u) / 64u;    // >= 1
    const unsigned long long p = (unsigned long long)lo + 1ull + (unsigned long long)lane * step;
    const bool in = p < hi && (unsigned long long)counts[p] * 1000ull >= floor1000;
    const unsigned long long b = __ballot(in);
    const uint32_t n = b == ~0ull ? 64u : (uint32_t)__ffsll((long long)~b) - 1u;   // the leading considered probes
    const unsigned long long next = (unsigned long long)lo + 1ull + (unsigned long long)n * step;   // the first probe that is not
    if (next < hi) hi = (uint32_t)next;
    if (n) lo = lo + 1u + (n - 1u) * step;
  }
  return hi;
}

// A 256-thread workgroup takes four queries at a time, a wavefront each.  A query whose considered prefix is longer
// than wave_cap is left to the whole workgroup, which folds such queries after the four waves are through with theirs.
__global__ __launch_bounds__(kLcaBlock) void lca_kernel(LcaArgs a) {
  __shared__ uint32_t sh_q[kLcaWaves], sh_m[kLcaWaves], sh_part[kLcaWaves];
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  uint32_t bad = 0;
  for (uint32_t q0 = blockIdx.x * kLcaWaves; q0 < a.nq; q0 += gridDim.x * kLcaWaves) {   // (uniform over the workgroup)
    const uint32_t q = q0 + w;
    uint32_t long_q = kLcaNoQuery, m = 0;
    if (q < a.nq) {   // (uniform over the wavefront)
      const unsigned long long h0 = a.hit_off[q], h1 = a.hit_off[q + 1];
      uint32_t taxon = kTaxonNone, best = 0, best_g = 0xFFFFFFFFu;
      bool done = true;
      if (h1 > h0 && h1 - h0 <= a.n_genomes) {
        const uint32_t len = (uint32_t)(h1 - h0);
        const uint32_t *counts = a.hit_counts + h0, *gids = a.hit_gids + h0;
        best = counts[0];
        best_g = gids[0];
        m = lca_considered(counts, len, (unsigned long long)best * (1000u - a.top_permille));
        if (m <= a.wave_cap) {
          taxon = lca_wave_reduce(a, lca_fold(a, gids, lane, 64, m, bad), bad);
          if (taxon == kLcaNothing) taxon = kTaxonNone;   // (only after bad entries)
        } else {
          long_q = q;
          done = false;
        }
      } else if (h1 > h0) {   // never a list longer than the genome count; the host ends the call
        bad += lane == 0 ? 1u : 0u;
      }
      if (lane == 0) {
        if (done) {
          a.taxon[q] = taxon;
          if (taxon == kTaxonNone && m >= 2) atomicAdd(a.info + kLcaInfoNoCommon, 1u);
        }
        if (a.best_count) a.best_count[q] = best;
        if (a.best_gid) a.best_gid[q] = best_g;
        if (a.considered) a.considered[q] = m;
      }
    }
    if (lane == 0) {
      sh_q[w] = long_q;
      sh_m[w] = m;
    }
    __syncthreads();
    for (uint32_t j = 0; j < kLcaWaves; ++j) {
      const uint32_t lq = sh_q[j];
      if (lq == kLcaNoQuery) continue;   // (read from LDS behind a barrier: uniform over the workgroup)
      const uint32_t *gids = a.hit_gids + a.hit_off[lq];
      const uint32_t part = lca_wave_reduce(a, lca_fold(a, gids, threadIdx.x, kLcaBlock, sh_m[j], bad), bad);
      if (lane == 0) sh_part[w] = part;
      __syncthreads();
      if (w == 0) {
        uint32_t taxon = lca_wave_reduce(a, lane < kLcaWaves ? sh_part[lane] : kLcaNothing, bad);
        if (taxon == kLcaNothing) taxon = kTaxonNone;
        if (lane == 0) {
          a.taxon[lq] = taxon;
          atomicAdd(a.info + kLcaInfoLong, 1u);
          if (taxon == kTaxonNone) atomicAdd(a.info + kLcaInfoNoCommon, 1u);   // (a long prefix has two entries or more)
        }
      }
      __syncthreads();   // (sh_part is written again by the next long query)
    }
    __syncthreads();   // (sh_q and sh_m are written again by the next four queries)
  }
  if (bad) atomicAdd(a.info + kLcaInfoBad, bad);
}

}  // namespace

hipError_t launch_lca(const LcaArgs &a, hipStream_t stream) {
  if (a.nq == 0) return hipSuccess;
  // four queries a workgroup and turn; no more workgroups than keep every compute unit full
  const uint32_t blocks = std::min<uint32_t>((a.nq + kLcaWaves - 1) / kLcaWaves, 256u * 8u);
  hipLaunchKernelGGL(lca_kernel, dim3(blocks), dim3(kLcaBlock), 0, stream, a);
  return hipGetLastError();
}

}  // namespace nq
