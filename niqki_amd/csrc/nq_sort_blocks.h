// nq_sort_blocks.h -- the two ordering blocks the hit kernels (nq_hits.hip) and the containment kernels
// (nq_contain.hip) share: a stable 8-bit radix pass of one wave, and a bitonic network over the 256 threads of a
// workgroup.  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nq {

// One wave: a stable LSD radix pass on bits [shift, shift + 8) of in_c, descending, from in_* to out_* (in_g rides
// along).  cur: 256 words of LDS of the wave's own.  Entries with equal digits keep their order.
__device__ inline void radix_pass_desc(const uint32_t *in_c, const uint32_t *in_g, uint32_t *out_c,
                                       uint32_t *out_g, unsigned long long n, uint32_t shift,
                                       uint32_t *cur, uint32_t lane) {
  for (uint32_t i = lane; i < 256; i += 64) cur[i] = 0;
  for (unsigned long long i = lane; i < n; i += 64) atomicAdd(&cur[(in_c[i] >> shift) & 0xFFu], 1u);
  // exclusive scan from digit 255 downwards
  uint32_t running = 0;
  for (int c = 192; c >= 0; c -= 64) {
    uint32_t d = (uint32_t)c + 63u - lane;  // lane 0 holds the largest digit of the chunk
    uint32_t x = cur[d];
    uint32_t incl = x;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      uint32_t y = __shfl_up(incl, o, 64);
      if (lane >= (uint32_t)o) incl += y;
    }
    cur[d] = running + incl - x;
    running += __shfl(incl, 63, 64);
  }
  const uint64_t lt_mask = (1ULL << lane) - 1ULL;
  for (unsigned long long base = 0; base < n; base += 64) {
    unsigned long long i = base + lane;
    bool valid = i < n;
    uint32_t c = valid ? in_c[i] : 0u, g = valid ? in_g[i] : 0u;
    uint32_t dgt = (c >> shift) & 0xFFu;
    uint64_t peers = __ballot(valid);
#pragma unroll
    for (uint32_t b = 0; b < 8; ++b) {
      bool bit = (dgt >> b) & 1u;
      uint64_t bal = __ballot(bit);
      peers &= bit ? bal : ~bal;
    }
    if (valid) {
      uint32_t rank = __popcll(peers & lt_mask), cntp = __popcll(peers);
      uint32_t p = cur[dgt];
      out_c[p + rank] = c;
      out_g[p + rank] = g;
      if (rank == cntp - 1) cur[dgt] = p + cntp;
    }
  }
}

// 256 * ITEMS keys (high half << GB | low half, zero = none) from LDS, ordered descending by a bitonic network over the
// 256 threads of a workgroup, the first n_out unpacked to hc (high halves) / hg (low halves).  Element i = r * 256 + tid
// lives in register k[r]: a stage whose partner i ^ j lies in the same thread (j >= 256) or the same wave (j < 64) needs
// no LDS and no barrier; only the strides 64 and 128 go through LDS (9 of the 66 stages of 2048 keys).
// K = uint32_t: GB = 16 (the hit kernels: count << 16 | gid, gids < 2^16); K = unsigned long long: GB = 32 (count << 32 |
// gid for any gid; the containment kernels: nq_contain_share.h).
template <typename K, int ITEMS>
__device__ __forceinline__ void bitonic_desc_256(K *keys, uint32_t tid, uint32_t n_out, uint32_t *hc, uint32_t *hg) {
  constexpr uint32_t GB = sizeof(K) * 4;   // bits of the gid
  K k[ITEMS];
#pragma unroll
  for (int r = 0; r < ITEMS; ++r) k[r] = keys[r * 256 + tid];
  constexpr uint32_t P = 256u * ITEMS;
#pragma unroll
  for (uint32_t kk = 2; kk <= P; kk <<= 1) {
#pragma unroll
    for (uint32_t j = kk >> 1; j > 0; j >>= 1) {
      if (j >= 256) {   // partner in this thread
#pragma unroll
        for (int r = 0; r < ITEMS; ++r) {
          const int r2 = r ^ (int)(j >> 8);
          if (r2 > r) {
            const bool desc = (((uint32_t)r * 256u) & kk) == 0;   // (kk > j >= 256: bit kk of i is a bit of r)
            const K x = k[r], y = k[r2];
            const K hi = x > y ? x : y, lo = x > y ? y : x;
            k[r] = desc ? hi : lo;
            k[r2] = desc ? lo : hi;
          }
        }
      } else {
        if (j >= 64) {   // partner in another wave: through LDS
          __syncthreads();
#pragma unroll
          for (int r = 0; r < ITEMS; ++r) keys[r * 256 + tid] = k[r];
          __syncthreads();
        }
        const bool lower = (tid & j) == 0;
#pragma unroll
        for (int r = 0; r < ITEMS; ++r) {
          const uint32_t i = (uint32_t)r * 256u + tid;
          const bool desc = (i & kk) == 0;
          const K x = k[r];
          const K y = j >= 64 ? keys[r * 256 + (tid ^ j)] : (K)__shfl_xor(x, (int)j, 64);
          const K hi = x > y ? x : y, lo = x > y ? y : x;
          k[r] = (desc == lower) ? hi : lo;
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < ITEMS; ++r) {
    const uint32_t i = (uint32_t)r * 256u + tid;
    if (i < n_out) { hc[i] = (uint32_t)(k[r] >> GB); hg[i] = (uint32_t)(k[r] & ((K(1) << GB) - 1u)); }
  }
}

}  // namespace nq
