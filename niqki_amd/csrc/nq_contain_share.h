// nq_contain_share.h -- the share of niqki_query_contained (niqki_hip.h) and the key its lists are ordered by
// (nq_contain.hip, the kernels; nq_api_contain.hip).
//
// A hit with count c of F = 2^S slots (S <= 16), query size q and genome size g (distinct k-mers, below 2^40) shares
//     |A n B| = J (|A| + |B|) / (1 + J),   J = c / F
// k-mers with the query; divided by d -- q, g or min(q, g), the mode -- that is Nn / Dd with
//     Nn = c (q + g),   Dd = (F + c) d,    both below 2^57.
// The share is 0xFFFFFFFF where Nn >= Dd, else floor(Nn 2^32 / Dd): 32 rounds of "double Nn; where it reaches Dd, take
// Dd off and set the bit".  Nn < Dd < 2^57 before every round, so the doubled value stays below 2^58: plain 64-bit
// arithmetic, no division, no floating point.  The caller leaves out the hits without a size (q == 0 or g == 0).
//
// The key of entry `pos` of a query's hit list H is share << 32 | (0xFFFFFFFF - pos): keys are distinct, no key is 0
// (pos < 2^32 - 1), and descending key order is share descending with ties in H's order.
//
// Host and device share this code: the kernels call it, tests/test_contain_ref_cpu.py compiles it with g++.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define NQ_CS_HD __host__ __device__ __forceinline__
#else
#define NQ_CS_HD inline
#endif

namespace nq {

constexpr uint32_t kContainQuery = 0, kContainGenome = 1, kContainMax = 2;   // NIQKI_CONTAIN_*
constexpr uint32_t kContainOne = 0xFFFFFFFFu;                                // NIQKI_CONTAIN_ONE
constexpr uint32_t kContainSizeBits = 40;

NQ_CS_HD bool contain_size_fits(uint64_t size) { return (size >> kContainSizeBits) == 0; }

// c <= F <= 2^16; q and g fit (contain_size_fits) and neither is 0; mode <= 2
NQ_CS_HD uint32_t contain_share(uint32_t c, uint32_t F, uint64_t q, uint64_t g, uint32_t mode) {
  const uint64_t d = mode == kContainQuery ? q : mode == kContainGenome ? g : (q < g ? q : g);
  uint64_t n = (uint64_t)c * (q + g);
  const uint64_t dd = (uint64_t)(F + c) * d;
  if (n >= dd) return kContainOne;
  uint32_t s = 0;
  for (int i = 0; i < 32; ++i) {
    n <<= 1;
    s <<= 1;
    if (n >= dd) {
      n -= dd;
      s |= 1u;
    }
  }
  return s;
}

NQ_CS_HD uint64_t contain_key(uint32_t share, uint32_t pos) { return (uint64_t)share << 32 | (uint64_t)(0xFFFFFFFFu - pos); }
NQ_CS_HD uint32_t contain_key_share(uint64_t key) { return (uint32_t)(key >> 32); }
NQ_CS_HD uint32_t contain_key_pos(uint64_t key) { return 0xFFFFFFFFu - (uint32_t)key; }

}  // namespace nq
