// nq_linkage_key.h -- the edge key of niqki_linkage (nq_cluster.hip, the forest kernels; nq_api_selfjoin.hip).
//
// An undirected edge (lo < hi, count) of the co-occurrence graph is ONE u64:
//     count << 46 | (M - lo) << 23 | (M - hi),        M = 2^23 - 1
// The count has 17 bits (65 536 occurs at S = 16), each id 23.  A LARGER key is EARLIER in the edge order of the header
// (larger count first, among equal counts the smaller lo, then the smaller hi), so a 64-bit atomic maximum picks the
// first edge of a set, a descending sort of keys is the edge order, and the key decodes back to its edge.  No edge has
// key 0: an edge has count >= 1.  Ids above M do not fit: niqki_linkage refuses more than 2^23 genomes.
//
// Host and device share this code: the kernels call it, tests/test_linkage_key_cpu.py compiles it with g++.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define NQ_LK_HD __host__ __device__ __forceinline__
#else
#define NQ_LK_HD inline
#endif

namespace nq {

constexpr uint32_t kLinkageIdBits = 23;
constexpr uint32_t kLinkageIdMax = (1u << kLinkageIdBits) - 1u;   // M: the largest genome id a key holds
constexpr uint32_t kLinkageCountMax = (1u << 17) - 1u;

// genomes an index may hold for niqki_linkage: ids 0 .. M
NQ_LK_HD bool linkage_fits(uint64_t n_genomes) { return n_genomes <= (uint64_t)kLinkageIdMax + 1u; }

NQ_LK_HD uint64_t linkage_pack(uint32_t count, uint32_t lo, uint32_t hi) {
  return (uint64_t)count << (2 * kLinkageIdBits) | (uint64_t)(kLinkageIdMax - lo) << kLinkageIdBits | (uint64_t)(kLinkageIdMax - hi);
}

NQ_LK_HD uint32_t linkage_count(uint64_t key) { return (uint32_t)(key >> (2 * kLinkageIdBits)); }
NQ_LK_HD uint32_t linkage_lo(uint64_t key) { return kLinkageIdMax - ((uint32_t)(key >> kLinkageIdBits) & kLinkageIdMax); }
NQ_LK_HD uint32_t linkage_hi(uint64_t key) { return kLinkageIdMax - ((uint32_t)key & kLinkageIdMax); }

}  // namespace nq
