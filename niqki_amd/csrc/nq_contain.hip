// nq_contain.hip -- the kernels of niqki_query_contained (nq_api_contain.hip): the share of every entry of a query's
// ordered hit list (nq_contain_share.h), the entries that have a size and reach the threshold, and those in the order of
// their shares with ties in the list's order.  Counts, the floor, H's order and its ties come from the query path;
// nothing here counts hits.  A workgroup of 256 takes a query; every loop is bounded by its list, none waits for
// another thread, and every barrier stands where the whole workgroup passes.  DESIGN.md 4.5h.
#include "nq_common.h"
#include "nq_contain_share.h"
#include "nq_kernels.h"
#include "nq_sort_blocks.h"

#include <hip/hip_runtime.h>

namespace nq {

namespace {

constexpr uint32_t kContainBlock = 256;

// Per query: n_unsized = its entries without a size (the query's own size 0: all of them); the others' shares; those
// with share >= min_share compacted in list order to a_share / a_npos[hit_off[q] ...), n_surv of them.  A chunk of 256
// entries gets its ranks from the waves' ballots.
__global__ __launch_bounds__(kContainBlock) void contain_share_kernel(ContainArgs a) {
  __shared__ uint32_t wave_n[kContainBlock / 64];
  __shared__ uint32_t sh_unsized;
  const uint32_t q = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
  const unsigned long long h0 = a.hit_off[q], h1 = a.hit_off[q + 1];
  const unsigned long long qs = a.qsizes[q];
  // (uniform over the workgroup from here on)
  const bool fits = contain_size_fits(qs), in_range = h1 >= h0 && h1 - h0 <= a.n_genomes;
  if (!fits || !in_range || h1 == h0 || qs == 0) {
    if (tid == 0) {
      a.n_surv[q] = 0;
      a.n_unsized[q] = fits && in_range ? (uint32_t)(h1 - h0) : 0u;
      if (!fits) atomicAdd(a.info + kContainInfoBadSize, 1u);
      else if (!in_range) atomicAdd(a.info + kContainInfoBad, 1u);
    }
    return;
  }
  const uint32_t len = (uint32_t)(h1 - h0);
  const uint32_t *counts = a.hit_counts + h0, *gids = a.hit_gids + h0;
  uint32_t *o_share = a.a_share + h0, *o_npos = a.a_npos + h0;
  if (tid == 0) sh_unsized = 0;
  __syncthreads();
  uint32_t done = 0, unsized = 0, bad = 0;
  for (uint32_t c0 = 0; c0 < len; c0 += kContainBlock) {
    const uint32_t pos = c0 + tid;
    bool keep = false;
    uint32_t share = 0;
    if (pos < len) {
      const uint32_t c = counts[pos], g = gids[pos];
      if (g >= a.n_genomes || c > a.F) {
        bad += 1;
      } else {
        const unsigned long long gs = a.sizes[g];
        if (gs == 0) {
          unsized += 1;
        } else {
          share = contain_share(c, a.F, qs, gs, a.mode);
          keep = share >= a.min_share;
        }
      }
    }
    const unsigned long long ballot = __ballot(keep);
    if (lane == 0) wave_n[w] = (uint32_t)__popcll(ballot);
    __syncthreads();
    uint32_t before = 0, total = 0;
    for (uint32_t i = 0; i < kContainBlock / 64; ++i) {
      before += i < w ? wave_n[i] : 0u;
      total += wave_n[i];
    }
    if (keep) {
      const uint32_t r = done + before + (uint32_t)__popcll(ballot & ((1ull << lane) - 1ull));   // (r <= pos)
      o_share[r] = share;
      o_npos[r] = 0xFFFFFFFFu - pos;
    }
    done += total;
    __syncthreads();
  }
  if (unsized) atomicAdd(&sh_unsized, unsized);
  if (bad) atomicAdd(a.info + kContainInfoBad, bad);
  __syncthreads();
  if (tid == 0) {
    a.n_surv[q] = done;
    a.n_unsized[q] = sh_unsized;
  }
}

// Per query: its n_surv survivors from list order into descending key order (share << 32 | 0xFFFFFFFF - position:
// share descending, ties in list order), in place in a_*; n_kept = min(n_surv, top_k).  Up to kContainNetworkMax
// survivors are keys in LDS under the bitonic network of the hit kernels, which writes the first n_kept back.  More go
// through four stable 8-bit radix passes of one wave on the share with the position as payload, a_* -> b_* -> a_* twice
// (the survivors are in list order on entry, so equal shares stay in it).
__global__ __launch_bounds__(kContainBlock) void contain_order_kernel(ContainArgs a) {
  __shared__ unsigned long long keys[kContainNetworkMax];
  __shared__ uint32_t cur[256];
  const uint32_t q = blockIdx.x, tid = threadIdx.x;
  const uint32_t m = a.n_surv[q];
  const unsigned long long h0 = a.hit_off[q];
  const uint32_t n_out = a.top_k && m > a.top_k ? a.top_k : m;
  if (tid == 0) a.n_kept[q] = n_out;
  if (m <= 1) return;   // (uniform: nothing to order)
  uint32_t *as = a.a_share + h0, *an = a.a_npos + h0;
  if (m <= kContainNetworkMax) {
    const uint32_t P = m <= 256 ? 256u : m <= 512 ? 512u : m <= 1024 ? 1024u : 2048u;
    for (uint32_t i = tid; i < P; i += kContainBlock) keys[i] = i < m ? (unsigned long long)as[i] << 32 | an[i] : 0ull;   // (no key is 0)
    __syncthreads();
    if (P == 256) bitonic_desc_256<unsigned long long, 1>(keys, tid, n_out, as, an);
    else if (P == 512) bitonic_desc_256<unsigned long long, 2>(keys, tid, n_out, as, an);
    else if (P == 1024) bitonic_desc_256<unsigned long long, 4>(keys, tid, n_out, as, an);
    else bitonic_desc_256<unsigned long long, 8>(keys, tid, n_out, as, an);
  } else {
    if (tid == 0) atomicAdd(a.info + kContainInfoLong, 1u);
    if (tid < 64) {   // (wave-private below: no barrier)
      uint32_t *bs = a.b_share + h0, *bn = a.b_npos + h0;
      radix_pass_desc(as, an, bs, bn, m, 0, cur, tid);
      __threadfence_block();
      radix_pass_desc(bs, bn, as, an, m, 8, cur, tid);
      __threadfence_block();
      radix_pass_desc(as, an, bs, bn, m, 16, cur, tid);
      __threadfence_block();
      radix_pass_desc(bs, bn, as, an, m, 24, cur, tid);
    }
  }
}

__global__ __launch_bounds__(kContainBlock) void contain_emit_kernel(ContainArgs a, const unsigned long long *off, ContainedHit *out) {
  const uint32_t q = blockIdx.x;
  const uint32_t n = a.n_kept[q];
  const unsigned long long h0 = a.hit_off[q];
  const uint32_t len = (uint32_t)(a.hit_off[q + 1] - h0);
  ContainedHit *dst = out + off[q];
  for (uint32_t r = threadIdx.x; r < n; r += kContainBlock) {
    const uint32_t pos = 0xFFFFFFFFu - a.a_npos[h0 + r];
    // (a position outside the list cannot be: it would be read as no hit at all)
    dst[r] = pos < len ? ContainedHit{a.a_share[h0 + r], a.hit_counts[h0 + pos], a.hit_gids[h0 + pos]} : ContainedHit{0u, 0u, 0xFFFFFFFFu};
  }
}

__global__ __launch_bounds__(kContainBlock) void contain_unpack_kernel(const ContainedHit *in, uint64_t n, uint32_t *hit_shares,
                                                                      uint32_t *hit_counts, uint32_t *hit_gids) {
  const uint64_t j = (uint64_t)blockIdx.x * kContainBlock + threadIdx.x;
  if (j >= n) return;
  const ContainedHit e = in[j];
  hit_shares[j] = e.share;
  hit_counts[j] = e.count;
  hit_gids[j] = e.gid;
}

}  // namespace

hipError_t launch_contain_share(const ContainArgs &a, hipStream_t stream) {
  if (a.nq == 0) return hipSuccess;
  hipLaunchKernelGGL(contain_share_kernel, dim3(a.nq), dim3(kContainBlock), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_contain_order(const ContainArgs &a, hipStream_t stream) {
  if (a.nq == 0) return hipSuccess;
  hipLaunchKernelGGL(contain_order_kernel, dim3(a.nq), dim3(kContainBlock), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_contain_emit(const ContainArgs &a, const unsigned long long *off, ContainedHit *out, hipStream_t stream) {
  if (a.nq == 0) return hipSuccess;
  hipLaunchKernelGGL(contain_emit_kernel, dim3(a.nq), dim3(kContainBlock), 0, stream, a, off, out);
  return hipGetLastError();
}

hipError_t launch_contain_unpack(const ContainedHit *in, uint64_t n, uint32_t *hit_shares, uint32_t *hit_counts, uint32_t *hit_gids,
                                 hipStream_t stream) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(contain_unpack_kernel, dim3((uint32_t)((n + kContainBlock - 1) / kContainBlock)), dim3(kContainBlock), 0, stream, in, n,
                     hit_shares, hit_counts, hit_gids);
  return hipGetLastError();
}

}  // namespace nq
