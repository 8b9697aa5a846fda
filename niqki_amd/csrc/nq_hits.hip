// nq_hits.hip -- the threshold / compaction / ordering of the hits of a query, for gfx950.
//
// Replaces the second half of Index::query_sketch (src/niqki_index.cpp:633-687), behind the counting loop that is
// gather_kernel (nq_gather.hip): the threshold (:662-666) and the descending (count, gid) order (:685) are the
// hits_* kernels on counter rows, the hitlist_* kernels on the lists that leave the gather kernel; top-k select,
// candidate lists and the plane adds of S = 16 handles live here too.
#include "nq_kernels.h"
#include "nq_sort_blocks.h"

#include <algorithm>
#include <cstdlib>

namespace nq {

// ---- hits: threshold, compaction in descending gid order, stable sort on count ----

// blk_counts[q][b] = number of genomes of block b with count >= min_score, and the query's total
// in hit_off[q] (scanned into offsets by hits_scan_kernel).  One workgroup per query: wave w takes
// blocks w, w+16, ...; a lane reads 8 counters (16 bytes) at a time.
// WIDE: the 16 waves of a workgroup share one query (large indexes).  !WIDE (fewer than 8 blocks,
// i.e. < 32 768 genomes: the short-read indexes): a wave per query, 16 queries per workgroup.
template <bool WIDE>
__global__ __launch_bounds__(1024) void hits_count_kernel(HitsArgs a) {
  __shared__ uint32_t s_sum;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t q = WIDE ? blockIdx.x : blockIdx.x * 16u + wave;
  if (WIDE) {
    if (threadIdx.x == 0) s_sum = 0;
    __syncthreads();
  } else if (q >= a.nq) {
    return;   // (no barrier on this path)
  }
  const uint16_t *row = a.counts + (uint64_t)q * a.stride + a.gid_begin;
  const uint16_t *row2 = a.counts2 ? a.counts2 + (uint64_t)q * a.stride + a.gid_begin : nullptr;
  const bool vec = (((uintptr_t)row) & 15) == 0 && !row2;   // uniform per wave
  uint32_t mine = 0;
  for (uint32_t b = WIDE ? wave : 0u; b < a.n_blk; b += WIDE ? 16u : 1u) {
    const uint32_t lo = b * kHitsBlk;
    const uint32_t hi = (lo + kHitsBlk < a.n_gids) ? lo + kHitsBlk : a.n_gids;
    uint32_t c = 0;
    if (vec) {
      for (uint32_t i = lo + lane * 8; i < hi; i += 512) {
        if (i + 8 <= hi) {
          const uint4 w = *(const uint4 *)(row + i);
          const uint32_t x[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
          for (int k = 0; k < 4; ++k) c += ((x[k] & 0xFFFFu) >= a.min_score) + ((x[k] >> 16) >= a.min_score);
        } else {
          for (uint32_t j = i; j < hi; ++j) c += (row[j] >= a.min_score);
        }
      }
    } else {
      for (uint32_t i = lo + lane; i < hi; i += 64) c += ((uint32_t)row[i] + (row2 ? (uint32_t)row2[i] : 0u) >= a.min_score);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o, 64);
    if (lane == 0) { a.blk_counts[(uint64_t)q * a.n_blk + b] = c; mine += c; }
  }
  if (!WIDE) {
    if (lane == 0) a.hit_off[q] = mine;
    return;
  }
  if (lane == 0 && mine) atomicAdd(&s_sum, mine);
  __syncthreads();
  if (threadIdx.x == 0) a.hit_off[q] = s_sum;
}

// hit_off[0..nq): per-query totals -> exclusive prefix, hit_off[nq] = grand total.  One workgroup walks
// the totals 4096 at a time (four consecutive queries per thread, coalesced 32-byte pieces): thread sums, wave
// scan, the 16 wave totals through LDS, a running base.
__global__ __launch_bounds__(1024) void hits_scan_kernel(HitsArgs a) {
  __shared__ unsigned long long wave_tot[2][16];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  unsigned long long base = 0;
  uint32_t flip = 0;
  for (uint32_t q0 = 0; q0 < a.nq; q0 += 4096, flip ^= 1u) {
    const uint32_t q = q0 + 4 * tid;
    unsigned long long x[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) x[j] = q + j < a.nq ? a.hit_off[q + j] : 0ull;
    const unsigned long long mine = x[0] + x[1] + x[2] + x[3];
    unsigned long long incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned long long y = __shfl_up(incl, o, 64);
      if (lane >= (uint32_t)o) incl += y;
    }
    if (lane == 63) wave_tot[flip][wave] = incl;
    __syncthreads();   // (the other half of wave_tot is what the previous round may still be reading)
    unsigned long long before = 0, total = 0;
#pragma unroll
    for (uint32_t w = 0; w < 16; ++w) {
      const unsigned long long t = wave_tot[flip][w];
      if (w < wave) before += t;
      total += t;
    }
    unsigned long long run = base + before + incl - mine;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (q + j < a.nq) a.hit_off[q + j] = run;
      run += x[j];
    }
    base += total;
  }
  if (tid == 0) a.hit_off[a.nq] = base;
}

// Each (query, block) writes its hits at the mirrored position so that a
// query's segment ends up in DESCENDING gid order; the global block prefix is
// recomputed from hit_off and the per-block counts.
__global__ __launch_bounds__(256) void hits_compact_kernel(HitsArgs a) {
  __shared__ uint32_t wsum[4];
  __shared__ uint32_t s_before;
  __shared__ uint32_t tsum[4];
  const uint32_t q = blockIdx.x / a.n_blk, b = blockIdx.x % a.n_blk;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  if (a.blk_counts[blockIdx.x] == 0) return;  // nothing above the threshold in this block (uniform)
  // top-k: kept are c > T and the ties c == T from the skip-th of the block on (ascending gid); without top-k, or with
  // every tie of the block kept, c >= T (T = min_score without top-k: the threshold of src/niqki_index.cpp:662-666)
  const uint32_t T = a.thr ? a.thr[q] : a.min_score;
  const uint32_t skip = a.blk_skip ? a.blk_skip[blockIdx.x] : 0u;
  uint32_t tie_run = 0;   // ties of this block with smaller gid, so far
  if (tid == 0) {
    uint32_t before = 0;
    for (uint32_t i = 0; i < b; ++i) before += a.blk_counts[(uint64_t)q * a.n_blk + i];
    s_before = before;
  }
  const unsigned long long seg0 = a.hit_off[q], seg1 = a.hit_off[q + 1];
  const uint16_t *row = a.counts + (uint64_t)q * a.stride + a.gid_begin;
  const uint16_t *row2 = a.counts2 ? a.counts2 + (uint64_t)q * a.stride + a.gid_begin : nullptr;
  const uint32_t lo = b * kHitsBlk;
  const uint32_t hi = (lo + kHitsBlk < a.n_gids) ? lo + kHitsBlk : a.n_gids;
  __syncthreads();
  uint32_t run = s_before;  // hits of this query with smaller gid, so far
  for (uint32_t base = lo; base < hi; base += 256) {
    uint32_t i = base + tid;
    uint32_t c = (i < hi) ? (uint32_t)row[i] + (row2 ? (uint32_t)row2[i] : 0u) : 0u;
    bool hit = (i < hi) && (skip == 0 ? c >= T : c > T);
    if (skip != 0 && skip != kSkipAllTies) {   // the block where the ties' quota runs out (one per query at most)
      const bool tie = (i < hi) && c == T;
      const uint64_t tb = __ballot(tie);
      if (lane == 0) tsum[wave] = __popcll(tb);
      __syncthreads();
      uint32_t tpre = 0, ttot = 0;
#pragma unroll
      for (uint32_t w = 0; w < 4; ++w) { uint32_t x = tsum[w]; if (w < wave) tpre += x; ttot += x; }
      if (tie && tie_run + tpre + __popcll(tb & ((1ULL << lane) - 1ULL)) >= skip) hit = true;
      tie_run += ttot;
    }
    uint64_t bal = __ballot(hit);
    uint32_t rank = __popcll(bal & ((1ULL << lane) - 1ULL));
    if (lane == 0) wsum[wave] = __popcll(bal);
    __syncthreads();
    uint32_t pre = 0, tot = 0;
#pragma unroll
    for (uint32_t w = 0; w < 4; ++w) { uint32_t x = wsum[w]; if (w < wave) pre += x; tot += x; }
    if (hit) {
      unsigned long long asc = run + pre + rank;            // rank in ascending gid order
      unsigned long long pos = seg1 - 1 - asc;              // mirrored: descending gid
      if (pos >= seg0 && pos < a.capacity) {
        a.hit_counts[pos] = c;
        a.hit_gids[pos] = a.gid_begin + i;
      }
    }
    run += tot;
    __syncthreads();
  }
}

// ---- top-k: each query's boundary (T, r) on its counter row ----
// T = the largest count with at least k hits at or above it, r = how many genomes of count T are kept (the largest
// gids: the order of src/niqki_index.cpp:685 puts them first).  Radix select by count: pass 1 builds a histogram of
// count >> 4 over the hits in LDS (the boundary bin bh and the hits above it), pass 2 a histogram of the 16 counts of
// bin bh.  With n <= k hits nothing is cut: T = min_score, every tie kept (r = kSkipAllTies).

struct SelShared {
  uint32_t wsum[4];
  uint32_t h16[16];
  uint32_t bh, above, T, r;
};

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  return x;
}

// f(c) for every genome of [lo, hi) that a wave reads; lo is a multiple of kHitsBlk (rows start on 16-byte boundaries
// for the 8-counter loads where the caller made them so: NIQKI_ROW_STRIDE)
template <class Fn>
__device__ __forceinline__ void sel_walk(const uint16_t *row, const uint16_t *row2, uint32_t lo, uint32_t hi, uint32_t lane, Fn f) {
  if ((((uintptr_t)row) & 15) == 0 && !row2) {
    for (uint32_t i = lo + lane * 8; i < hi; i += 512) {
      if (i + 8 <= hi) {
        const uint4 w = *(const uint4 *)(row + i);
        f(w.x & 0xFFFFu); f(w.x >> 16); f(w.y & 0xFFFFu); f(w.y >> 16);
        f(w.z & 0xFFFFu); f(w.z >> 16); f(w.w & 0xFFFFu); f(w.w >> 16);
      } else {
        for (uint32_t j = i; j < hi; ++j) f((uint32_t)row[j]);
      }
    }
  } else {
    for (uint32_t i = lo + lane; i < hi; i += 64) f((uint32_t)row[i] + (row2 ? (uint32_t)row2[i] : 0u));
  }
}

// The boundary of one query's row, by the 256 threads of a workgroup (wave w takes blocks w, w+4, ...); hist:
// kSelBins words of LDS.  Returns n, the query's hit count; T and r only when n > k.  BLK (hits_select_kernel): pass 1
// also writes the blocks' hit counts to blk_counts (the answer when n <= k) and pass 2 the blocks' genomes above bin
// bh and their counts in bin bh to blk_tmp (kSelBlkWords per block), from which the kept entries of every block follow
// once T is known -- the row is read twice here and once more by the compaction.
template <bool BLK>
__device__ uint32_t sel_boundary(const uint16_t *row, const uint16_t *row2, uint32_t n_gids, uint32_t min_score, uint32_t k,
                                 uint32_t *hist, SelShared &sh, uint32_t *blk_counts, uint32_t *blk_skip, uint32_t *blk_tmp,
                                 uint32_t &T, uint32_t &r) {
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t n_blk = (n_gids + kHitsBlk - 1) / kHitsBlk;
  for (uint32_t i = tid; i < kSelBins; i += 256) hist[i] = 0;
  __syncthreads();
  uint32_t low = 0;   // hits of bin 0 (counts 0 .. 15: nearly every genome against an unrelated query) in a register
  for (uint32_t b = wave; b < n_blk; b += 4) {
    const uint32_t lo = b * kHitsBlk, hi = lo + kHitsBlk < n_gids ? lo + kHitsBlk : n_gids;
    uint32_t m = 0;
    sel_walk(row, row2, lo, hi, lane, [&](uint32_t c) {
      if (c >= min_score) {
        ++m;
        if (c < 16) ++low;
        else atomicAdd(&hist[(c >> 4) < kSelBins ? (c >> 4) : kSelBins - 1], 1u);
      }
    });
    if (BLK) {
      m = wave_sum_u32(m);
      if (lane == 0) { blk_counts[b] = m; blk_skip[b] = 0; }
    }
  }
  low = wave_sum_u32(low);
  if (lane == 0 && low) atomicAdd(&hist[0], low);
  __syncthreads();
  // thread t holds bins [17 t, 17 t + 17); the hits above its bins: a suffix sum over the threads
  uint32_t s = 0;
#pragma unroll
  for (uint32_t j = 0; j < 17; ++j) s += hist[tid * 17 + j];
  uint32_t incl = s;   // s of this lane and the lanes above it
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t y = __shfl_down(incl, o, 64);
    if (lane + (uint32_t)o < 64) incl += y;
  }
  if (lane == 0) sh.wsum[wave] = incl;
  if (tid < 16) sh.h16[tid] = 0;
  __syncthreads();
  uint32_t above_w = 0, n = 0;
#pragma unroll
  for (uint32_t w = 0; w < 4; ++w) { const uint32_t x = sh.wsum[w]; if (w > wave) above_w += x; n += x; }
  if (n <= k) return n;   // (uniform)
  const uint32_t excl = above_w + incl - s;
  if (excl < k && excl + s >= k) {   // the one thread whose bins hold the boundary
    uint32_t cum = excl;
    int j = 16;
    for (; j > 0; --j) {
      const uint32_t h = hist[tid * 17 + j];
      if (cum + h >= k) break;
      cum += h;
    }
    sh.bh = tid * 17 + j;
    sh.above = cum;
  }
  __syncthreads();
  const uint32_t bh = sh.bh;
  for (uint32_t b = wave; b < n_blk; b += 4) {
    const uint32_t lo = b * kHitsBlk, hi = lo + kHitsBlk < n_gids ? lo + kHitsBlk : n_gids;
    uint32_t above = 0, cnt[16];
#pragma unroll
    for (int v = 0; v < 16; ++v) cnt[v] = 0;
    sel_walk(row, row2, lo, hi, lane, [&](uint32_t c) {
      if (c >= min_score) {
        above += (c >> 4) > bh;
        if ((c >> 4) == bh) {
#pragma unroll
          for (uint32_t v = 0; v < 16; ++v) cnt[v] += (c & 15u) == v;
        }
      }
    });
    above = wave_sum_u32(above);
    if (BLK && lane == 0) blk_tmp[(size_t)b * kSelBlkWords] = above;
#pragma unroll
    for (uint32_t v = 0; v < 16; ++v) {
      const uint32_t x = wave_sum_u32(cnt[v]);
      if (lane == 0) {
        if (BLK) blk_tmp[(size_t)b * kSelBlkWords + 1 + v] = x;
        if (x) atomicAdd(&sh.h16[v], x);
      }
    }
  }
  __syncthreads();
  if (tid == 0) {
    uint32_t cum = sh.above;
    int v = 15;
    for (; v > 0; --v) {
      if (cum + sh.h16[v] >= k) break;
      cum += sh.h16[v];
    }
    sh.T = bh * 16 + (uint32_t)v;
    sh.r = k - cum;
  }
  __syncthreads();
  T = sh.T;
  r = sh.r;
  return n;
}

// top-k in place of hits_count_kernel: one workgroup per query.  hit_off[q] = min(n, k); blk_counts / blk_skip / thr
// as hits_compact_kernel takes them.  The ties at T are kept from the top gid down: block b keeps
// min(eq_b, max(0, r - ties in the blocks above b)) of its eq_b ties, its largest ones.
__global__ __launch_bounds__(256) void hits_select_kernel(HitsArgs a) {
  __shared__ uint32_t hist[kSelBins];
  __shared__ SelShared sh;
  const uint32_t q = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint16_t *row = a.counts + (uint64_t)q * a.stride + a.gid_begin;
  const uint16_t *row2 = a.counts2 ? a.counts2 + (uint64_t)q * a.stride + a.gid_begin : nullptr;
  uint32_t *bc = a.blk_counts + (uint64_t)q * a.n_blk, *bs = a.blk_skip + (uint64_t)q * a.n_blk;
  uint32_t *bt = a.blk_tmp + (uint64_t)q * a.n_blk * kSelBlkWords;
  uint32_t T = 0, r = 0;
  const uint32_t n = sel_boundary<true>(row, row2, a.n_gids, a.min_score, a.top_k, hist, sh, bc, bs, bt, T, r);
  if (n <= a.top_k) {
    if (tid == 0) { a.thr[q] = a.min_score; a.hit_off[q] = n; }
    return;
  }
  if (tid == 0) { a.thr[q] = T; a.hit_off[q] = a.top_k; }
  const uint32_t vt = T & 15u;
  uint32_t run = 0;   // ties in the blocks above the current 256
  for (uint32_t c0 = 0; c0 < a.n_blk; c0 += 256) {
    const uint32_t i = c0 + tid;
    const bool valid = i < a.n_blk;
    const uint32_t b = valid ? a.n_blk - 1 - i : 0u;   // thread order = descending block
    uint32_t gt = 0, eq = 0;
    if (valid) {
      const uint32_t *t = bt + (size_t)b * kSelBlkWords;
      gt = t[0];
      for (uint32_t v = vt + 1; v < 16; ++v) gt += t[1 + v];
      eq = t[1 + vt];
    }
    uint32_t incl = eq;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t y = __shfl_up(incl, o, 64);
      if (lane >= (uint32_t)o) incl += y;
    }
    __syncthreads();   // (sh.wsum of the previous round is read)
    if (lane == 63) sh.wsum[wave] = incl;
    __syncthreads();
    uint32_t before = 0, tot = 0;
#pragma unroll
    for (uint32_t w = 0; w < 4; ++w) { const uint32_t x = sh.wsum[w]; if (w < wave) before += x; tot += x; }
    const uint32_t after = run + before + incl - eq;   // ties in the blocks above b
    const uint32_t kept = r > after ? (r - after < eq ? r - after : eq) : 0u;
    if (valid) {
      bc[b] = gt + kept;
      bs[b] = kept == eq ? 0u : (kept == 0 ? kSkipAllTies : eq - kept);
    }
    run += tot;
  }
}

// One wave per query: stable LSD radix sort (2 x 8 bits) of the segment on the
// count, descending, in place in hit_* (descending gid on entry) through tmp_*.  Equal counts
// keep descending gid: greater<pair<count,gid>>, src/niqki_index.cpp:685.  The pass: radix_pass_desc (nq_sort_blocks.h).
__global__ __launch_bounds__(256) void hits_sort_kernel(HitsArgs a) {
  __shared__ uint32_t curs[4][256];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t q = blockIdx.x * 4 + wave;
  if (q >= a.nq) return;  // wave-private below
  unsigned long long seg0 = a.hit_off[q], seg1 = a.hit_off[q + 1];
  if (seg1 > a.capacity) seg1 = a.capacity;
  if (seg0 >= seg1) return;
  const unsigned long long n = seg1 - seg0;
  uint32_t *tc = a.tmp_counts + seg0, *tg = a.tmp_gids + seg0;
  uint32_t *hc = a.hit_counts + seg0, *hg = a.hit_gids + seg0;
  radix_pass_desc(hc, hg, tc, tg, n, 0, curs[wave], lane);
  __threadfence_block();
  radix_pass_desc(tc, tg, hc, hg, n, 8, curs[wave], lane);
  if (a.counts2) {  // S = 16: a count can be 2^16, 17 bits (two more passes bring the result back into hit_*)
    __threadfence_block();
    radix_pass_desc(hc, hg, tc, tg, n, 16, curs[wave], lane);
    __threadfence_block();
    radix_pass_desc(tc, tg, hc, hg, n, 24, curs[wave], lane);
  }
}

// Candidate genomes of every query: ids with counts[q][g] >= thr, at most `cap`
// per query (unordered), cand[q*cap + i], n[q] = how many there are (may exceed
// cap: the caller must then fall back to the dense exchange).  Used by the
// multi-GPU path: a genome whose summed count reaches min_score has a partial
// count >= ceil(min_score / shards) on at least one shard.
__global__ __launch_bounds__(256) void candidates_kernel(const uint16_t *counts, uint64_t stride, uint32_t n_gids,
                                                        uint32_t thr, uint32_t cap, int32_t *cand, int32_t *n) {
  __shared__ uint32_t s_n;
  const uint32_t q = blockIdx.x;
  if (threadIdx.x == 0) s_n = 0;
  __syncthreads();
  const uint16_t *row = counts + (uint64_t)q * stride;
  for (uint32_t g = threadIdx.x; g < n_gids; g += 256) {
    if (row[g] >= thr) {
      const uint32_t i = atomicAdd(&s_n, 1u);
      if (i < cap) cand[(uint64_t)q * cap + i] = (int32_t)g;
    }
  }
  __syncthreads();
  const uint32_t tot = s_n;
  for (uint32_t i = tot + threadIdx.x; i < cap; i += 256) cand[(uint64_t)q * cap + i] = -1;
  if (threadIdx.x == 0) n[q] = (int32_t)tot;
}

hipError_t launch_candidates(const uint16_t *counts, uint64_t stride, uint32_t nq, uint32_t n_gids, uint32_t thr,
                             uint32_t cap, int32_t *cand, int32_t *n, hipStream_t stream) {
  if (nq == 0) return hipSuccess;
  hipLaunchKernelGGL(candidates_kernel, dim3(nq), dim3(256), 0, stream, counts, stride, n_gids, thr, cap, cand, n);
  return hipGetLastError();
}

__global__ __launch_bounds__(256) void plane_add16_kernel(uint16_t *a, const uint16_t *b, uint64_t n) {
  const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) a[i] = (uint16_t)(a[i] + b[i]);
}
__global__ __launch_bounds__(256) void plane_sum32_kernel(const uint16_t *a, const uint16_t *b, uint32_t *out, uint64_t n) {
  const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) out[i] = (uint32_t)a[i] + (b ? (uint32_t)b[i] : 0u);
}
hipError_t launch_plane_add16(uint16_t *a, const uint16_t *b, uint64_t n, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(plane_add16_kernel, dim3((uint32_t)std::min<uint64_t>((n + 255) / 256, 16384)), dim3(256), 0, stream, a, b, n);
  return hipGetLastError();
}
hipError_t launch_plane_sum32(const uint16_t *a, const uint16_t *b, uint32_t *out, uint64_t n, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(plane_sum32_kernel, dim3((uint32_t)std::min<uint64_t>((n + 255) / 256, 16384)), dim3(256), 0, stream, a, b, out, n);
  return hipGetLastError();
}

// After a gather launch with hit lists (CandOut::hl).
// hitlist_scan_kernel: hit_off[0..nq] = exclusive prefix of n[0..nq), 4096 queries per workgroup -- a workgroup first
// adds up what lies before its block (at most a few hundred KB of u32, from L2), then scans its own 4096 -- and the
// queries whose lists overflowed (n > hl_cap) are collected in over[1 ..], over[0] = how many (preset to 0).
__global__ __launch_bounds__(1024) void hitlist_scan_kernel(const uint32_t *n, uint32_t nq, uint32_t hl_cap, uint32_t k,
                                                            unsigned long long *hit_off, uint32_t *over) {
  __shared__ unsigned long long wave_tot[16];
  __shared__ unsigned long long s_base;
  __shared__ uint32_t s_over, s_over_base;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t q0 = blockIdx.x * 4096u;
  if (tid == 0) s_over = 0;
  unsigned long long part = 0;
  {   // (q0 is a multiple of 4096: whole 16-byte pieces, four independent loads in flight per thread)
    const uint4 *n4 = (const uint4 *)n;
    const uint32_t m = q0 / 4;
    uint32_t i = tid;
    if (k == 0) {
      for (; i + 3 * 1024 < m; i += 4 * 1024) {
        const uint4 a0 = n4[i], a1 = n4[i + 1024], a2 = n4[i + 2048], a3 = n4[i + 3072];
        part += (unsigned long long)a0.x + a0.y + a0.z + a0.w + a1.x + a1.y + a1.z + a1.w;
        part += (unsigned long long)a2.x + a2.y + a2.z + a2.w + a3.x + a3.y + a3.z + a3.w;
      }
    }
    for (; i < m; i += 1024) {   // (top-k: a query's segment holds min(n, k))
      const uint4 a0 = n4[i];
      part += k ? (unsigned long long)min(a0.x, k) + min(a0.y, k) + min(a0.z, k) + min(a0.w, k)
                : (unsigned long long)a0.x + a0.y + a0.z + a0.w;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) part += __shfl_down(part, o, 64);
  if (lane == 0) wave_tot[wave] = part;
  __syncthreads();
  if (tid == 0) {
    unsigned long long b = 0;
    for (uint32_t w = 0; w < 16; ++w) b += wave_tot[w];
    s_base = b;
  }
  __syncthreads();
  const unsigned long long base = s_base;
  const uint32_t q = q0 + 4 * tid;
  unsigned long long x[4];
  uint32_t n_over = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    x[j] = q + j < nq ? n[q + j] : 0ull;
    n_over += x[j] > hl_cap ? 1u : 0u;
  }
  bool ov[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    ov[j] = x[j] > hl_cap;
    if (k && x[j] > k) x[j] = k;
  }
  uint32_t my_over = n_over ? atomicAdd(&s_over, n_over) : 0u;
  const unsigned long long mine = x[0] + x[1] + x[2] + x[3];
  unsigned long long incl = mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long y = __shfl_up(incl, o, 64);
    if (lane >= (uint32_t)o) incl += y;
  }
  __syncthreads();   // (wave_tot is reused; s_over is complete)
  if (lane == 63) wave_tot[wave] = incl;
  if (tid == 0 && s_over) s_over_base = atomicAdd(&over[0], s_over);
  __syncthreads();
  unsigned long long before = 0, total = 0;
#pragma unroll
  for (uint32_t w = 0; w < 16; ++w) {
    const unsigned long long t = wave_tot[w];
    if (w < wave) before += t;
    total += t;
  }
  unsigned long long run = base + before + incl - mine;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (q + j < nq) hit_off[q + j] = run;
    run += x[j];
    if (ov[j]) over[1 + s_over_base + my_over++] = q + j;
  }
  if (tid == 0 && q0 + 4096u >= nq) hit_off[nq] = base + total;
}

// The hits of a counter row of the hit-list form's emit launch (count >= min_score, src/niqki_index.cpp:662-666) as
// keys count << G | gid -- distinct keys whose descending order is greater<pair<count, gid>> (:685) -- in LDS, ordered
// there by a bitonic network of Pq keys (>= the row's hits) and the first n_out unpacked to [seg0, seg0 + n_out).
template <typename K>
__device__ void network_sort(const uint16_t *row, const HitsArgs &a, K *keys, uint32_t &s_n, uint32_t Pq, uint32_t n_out,
                             unsigned long long seg0, uint32_t tid) {
  constexpr uint32_t GB = sizeof(K) * 4;
  if (tid == 0) s_n = 0;
  for (uint32_t i = tid; i < Pq; i += 256) keys[i] = 0;
  __syncthreads();
  // 8 counters per lane and load (rows start on 128-byte lines: NIQKI_ROW_STRIDE)
  const bool vec = (((uintptr_t)row) & 15u) == 0;
  for (uint32_t i0 = tid * 8; i0 < a.n_gids; i0 += 256 * 8) {
    uint32_t c[8];
    if (vec && i0 + 8 <= a.n_gids) {
      const uint4 w = *(const uint4 *)(row + i0);
      c[0] = w.x & 0xFFFFu; c[1] = w.x >> 16; c[2] = w.y & 0xFFFFu; c[3] = w.y >> 16;
      c[4] = w.z & 0xFFFFu; c[5] = w.z >> 16; c[6] = w.w & 0xFFFFu; c[7] = w.w >> 16;
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) c[j] = i0 + j < a.n_gids ? (uint32_t)row[i0 + j] : 0u;
    }
    uint32_t m = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) m |= (uint32_t)(i0 + j < a.n_gids && c[j] >= a.min_score) << j;
    if (m) {
      uint32_t at = atomicAdd(&s_n, (uint32_t)__builtin_popcount(m));
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (m >> j & 1u) keys[at++] = ((K)c[j] << GB) | (K)(a.gid_begin + i0 + j);
    }
  }
  __syncthreads();
  // bitonic sort, descending (the zero keys behind the real ones end up last: a real key 0 -- count 0 of genome 0 at
  // min_score 0 -- is the smallest key and belongs there too), in registers: see bitonic_desc_256
  if (Pq <= 256) bitonic_desc_256<K, 1>(keys, tid, n_out, a.hit_counts + seg0, a.hit_gids + seg0);
  else if (Pq == 512) bitonic_desc_256<K, 2>(keys, tid, n_out, a.hit_counts + seg0, a.hit_gids + seg0);
  else if (Pq == 1024) bitonic_desc_256<K, 4>(keys, tid, n_out, a.hit_counts + seg0, a.hit_gids + seg0);
  else bitonic_desc_256<K, 8>(keys, tid, n_out, a.hit_counts + seg0, a.hit_gids + seg0);
  __syncthreads();
}

// A counter row thresholded into [seg0, ..) in descending gid by a 256-thread workgroup: c > T, and of the genomes with
// c == T the first r met from the top gid down (r = kSkipAllTies: all).  2048 counters per step: thread t takes the 8
// counters [top - 8 (t + 1), top - 8 t) -- thread 0 the largest gids -- and an exclusive scan of ties << 16 | hits over
// the threads places them; the next step's 16 bytes are loaded before this step's scan.  wtot: 4 words of LDS.
__device__ void compact_desc(const uint16_t *row, uint32_t n_gids, uint32_t T, uint32_t r, unsigned long long seg0,
                             const HitsArgs &a, uint32_t *wtot, uint32_t tid) {
  const uint32_t lane = tid & 63u, wave = tid >> 6;
  const bool vec = (((uintptr_t)row) & 15u) == 0;
  auto load = [&](long long lo) {   // counters [lo, lo + 8) as packed pairs, 0 outside the row
    if (vec && lo >= 0 && lo + 8 <= (long long)n_gids) return *(const uint4 *)(row + lo);
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const long long i = lo + j;
      if (i >= 0 && i < (long long)n_gids) w[j >> 1] |= (uint32_t)row[i] << ((j & 1) * 16);
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
  };
  const long long top0 = ((long long)n_gids + 7) & ~7ll;
  unsigned long long run = 0;   // entries written
  uint32_t ties_run = 0;        // genomes of count T met
  uint4 next = load(top0 - 8ll * (tid + 1));
  for (long long top = top0; top > 0; top -= 2048) {
    const long long lo = top - 8ll * (tid + 1);
    const uint4 w = next;
    if (top > 2048) next = load(top - 2048 - 8ll * (tid + 1));
    const uint32_t cw[4] = {w.x, w.y, w.z, w.w};
    uint32_t nh = 0, nt = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const long long i = lo + j;
      const uint32_t c = (cw[j >> 1] >> ((j & 1) * 16)) & 0xFFFFu;
      const bool in = i >= 0 && i < (long long)n_gids;
      nh += (uint32_t)(in && c > T);
      nt += (uint32_t)(in && c == T);
    }
    const uint32_t x = nt << 16 | nh;   // (<= 2048 of each per step)
    uint32_t incl = x;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t y = __shfl_up(incl, o, 64);
      if (lane >= (uint32_t)o) incl += y;
    }
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    uint32_t before = incl - x, total = 0;
#pragma unroll
    for (uint32_t v = 0; v < 4; ++v) {
      const uint32_t t = wtot[v];
      if (v < wave) before += t;
      total += t;
    }
    __syncthreads();   // (wtot is written again by the next step)
    // ties before this thread's: G; the kept ones among them and among those of earlier steps
    uint32_t G = ties_run + (before >> 16);
    const uint32_t kept_run = ties_run < r ? ties_run : r;
    unsigned long long pos = seg0 + run + (before & 0xFFFFu) + ((G < r ? G : r) - kept_run);
#pragma unroll
    for (int j = 7; j >= 0; --j) {
      const long long i = lo + j;
      const uint32_t c = (cw[j >> 1] >> ((j & 1) * 16)) & 0xFFFFu;
      if (i < 0 || i >= (long long)n_gids || c < T) continue;
      bool keep = c > T;
      if (c == T) keep = G++ < r;
      if (keep) {
        if (pos < a.capacity) { a.hit_counts[pos] = c; a.hit_gids[pos] = a.gid_begin + (uint32_t)i; }
        ++pos;
      }
    }
    const uint32_t tt = ties_run + (total >> 16);
    run += (total & 0xFFFFu) + ((tt < r ? tt : r) - kept_run);
    ties_run = tt;
  }
}

// hitlist_emit_kernel, two parts.  First, one wave per query (4 per workgroup, the first nq / 4 workgroups): a query whose list fits -- the usual
// case -- is a copy of its ordered entries to [hit_off[q], hit_off[q+1]).  Then the queries whose lists overflowed, one
// workgroup each (grid-stride over the list the scan made): up to P hits are thresholded from the query's counter row
// into LDS keys and ordered there by a bitonic network (network_sort); more are thresholded into the segment in
// descending gid by the workgroup and ordered by a wave's radix passes (compact_desc).  keys: P words of LDS (P >= 256),
// 2 P beyond 16-bit gids.
__global__ __launch_bounds__(256) void hitlist_emit_kernel(HitsArgs a, const uint32_t *hn, const unsigned long long *hl, uint32_t hl_cap,
                                                            const uint32_t *over, uint32_t P) {
  extern __shared__ __align__(16) uint32_t keys[];   // (top-k: at least kSelBins words, the select's histogram)
  __shared__ uint32_t s_n;
  __shared__ uint32_t s_wtot[4];
  __shared__ SelShared sh;
  const uint32_t tid = threadIdx.x;
  {
    const uint32_t lane = tid & 63u, q = blockIdx.x * 4 + (tid >> 6);
    if (q < a.nq) {
      // the segment: the list, or with top-k its first k entries
      const unsigned long long seg0 = a.hit_off[q], n_all = a.hit_off[q + 1] - seg0;
      if (n_all && hn[q] <= hl_cap) {
        const unsigned long long *src = hl + (uint64_t)q * hl_cap;
        for (uint32_t i = lane; i < (uint32_t)n_all; i += 64) {
          const unsigned long long pos = seg0 + i;
          if (pos < a.capacity) {
            const unsigned long long e = src[i];
            a.hit_counts[pos] = (uint32_t)(e >> 32);
            a.hit_gids[pos] = (uint32_t)e;
          }
        }
      }
    }
  }
  const uint32_t n_over = over[0];
  for (uint32_t k = blockIdx.x; k < n_over; k += gridDim.x) {
    const uint32_t q = over[1 + k];
    // n_hit: the query's hits; n_all: its segment (min(n_hit, top_k) with top-k)
    const unsigned long long seg0 = a.hit_off[q], n_all = a.hit_off[q + 1] - seg0, n_hit = hn[q];
    const uint16_t *row = a.counts + (uint64_t)q * a.stride + a.gid_begin;
    if (n_hit > P) {
      // more hits than the network holds (a threshold that lets a sixth of the index through): the workgroup thresholds
      // the row in descending gid into the segment and one wave orders it with the stable radix passes of
      // hits_sort_kernel, through tmp_*.  With top-k the row keeps c > T and the first r genomes of count T in
      // descending gid (the largest gids): the select's boundary
      uint32_t T = a.min_score, r = kSkipAllTies;
      if (a.top_k && n_hit > a.top_k) sel_boundary<false>(row, nullptr, a.n_gids, a.min_score, a.top_k, keys, sh, nullptr, nullptr, nullptr, T, r);
      compact_desc(row, a.n_gids, T, r, seg0, a, s_wtot, tid);
      __syncthreads();   // (the segment is written: global stores of the workgroup before the wave's loads)
      if (tid < 64) {
        unsigned long long seg1 = seg0 + n_all;
        if (seg1 > a.capacity) seg1 = a.capacity;
        if (seg0 < seg1) {
          const unsigned long long n = seg1 - seg0;
          uint32_t *tc = a.tmp_counts + seg0, *tg = a.tmp_gids + seg0;
          uint32_t *hc = a.hit_counts + seg0, *hg = a.hit_gids + seg0;
          radix_pass_desc(hc, hg, tc, tg, n, 0, keys, tid);
          __threadfence_block();
          radix_pass_desc(tc, tg, hc, hg, n, 8, keys, tid);
        }
      }
      __syncthreads();
      continue;
    }
    // the network's size for this query
    uint32_t Pq = 256;
    while (Pq < n_hit) Pq <<= 1;   // (n_hit <= P here, and P >= 256 is a power of two)
    const unsigned long long room = seg0 < a.capacity ? a.capacity - seg0 : 0ull;
    const uint32_t n_out = (uint32_t)(n_all < room ? n_all : room);
    // (gids of 16 bits: 4-byte keys; a larger index: 8-byte keys, the LDS block holds 2 P words then)
    if (a.gid_begin + a.n_gids <= 65536u) network_sort<uint32_t>(row, a, keys, s_n, Pq, n_out, seg0, tid);
    else network_sort<unsigned long long>(row, a, (unsigned long long *)keys, s_n, Pq, n_out, seg0, tid);
  }
}

hipError_t launch_hitlist_scan(const uint32_t *n, const HitsArgs &a, uint32_t hl_cap, uint32_t *over, hipStream_t stream) {
  if (a.nq == 0) return hipSuccess;   // (over[0] = 0: the gather launch that made n has done it, CandOut::hl_over)
  hipLaunchKernelGGL(hitlist_scan_kernel, dim3((a.nq + 4095u) / 4096u), dim3(1024), 0, stream, n, a.nq, hl_cap, a.top_k, a.hit_off,
                     over);
  return hipGetLastError();
}

hipError_t launch_hitlist_emit(const HitsArgs &a, const uint32_t *n, const unsigned long long *hl, uint32_t hl_cap, const uint32_t *over,
                               hipStream_t stream) {
  if (a.nq == 0) return hipSuccess;
  // (the network: 2048 keys = 8 or 16 KB of LDS, several workgroups per CU; a query with more hits takes compact_desc)
  uint32_t P = 256;
  while (P < a.n_gids && P < 2048u) P <<= 1;
  const uint32_t words = a.gid_begin + a.n_gids > 65536u ? 2 * P : P;   // (8-byte keys beyond 16-bit gids)
  const uint32_t lds = a.top_k && words < kSelBins ? kSelBins : words;
  // (nq workgroups: the first nq / 4 copy the lists; every overflowing query then has a workgroup of its own -- a wave's
  // radix passes over a long segment are the slow part, and the counter-row path runs one wave per query at once too)
  hipLaunchKernelGGL(hitlist_emit_kernel, dim3(a.nq), dim3(256), (size_t)lds * 4, stream, a, n, hl, hl_cap, over, P);
  return hipGetLastError();
}

hipError_t launch_hits_count(const HitsArgs &a, hipStream_t stream) {
  if (a.nq == 0 || a.n_blk == 0) return hipSuccess;
  if (a.top_k) hipLaunchKernelGGL(hits_select_kernel, dim3(a.nq), dim3(256), 0, stream, a);
  else if (a.n_blk >= 8) hipLaunchKernelGGL(hits_count_kernel<true>, dim3(a.nq), dim3(1024), 0, stream, a);
  else hipLaunchKernelGGL(hits_count_kernel<false>, dim3((a.nq + 15) / 16), dim3(1024), 0, stream, a);
  hipLaunchKernelGGL(hits_scan_kernel, dim3(1), dim3(1024), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_hits_emit(const HitsArgs &a, hipStream_t stream) {
  if (a.nq == 0 || a.n_blk == 0) return hipSuccess;
  hipLaunchKernelGGL(hits_compact_kernel, dim3(a.nq * a.n_blk), dim3(256), 0, stream, a);
  hipLaunchKernelGGL(hits_sort_kernel, dim3((a.nq + 3) / 4), dim3(256), 0, stream, a);
  return hipGetLastError();
}

}  // namespace nq
