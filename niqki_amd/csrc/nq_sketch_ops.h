// nq_sketch_ops.h -- device helpers that more than one unit of the sketch side uses: the code table's entries, the
// canonical choice and the per-slot min (nq_sketch.hip, nq_sketch_reads.hip), the hash rounds and 64-bit shifts as
// the long-record loop issues them (nq_sketch.hip and its ceiling probe in nq_probe.hip), the wave's LDS ordering
// (nq_sketch_reads.hip and its probe).  A helper with one user lives beside its kernel.  All always inline.
#pragma once
#include "nq_common.h"

namespace nq {

// Per-byte code table, built in LDS by the first 256 threads.
//   bits 1:0  forward code of the rolling update   (:114-123  A0 C1 G2 T3, else 0)
//   bits 3:2  reverse-complement code of the update (:211-221 A3 C2 G1, else 0)
//   bits 5:4  case-insensitive digit of the K-1 prefix (:255-273)
//   bit  6    byte is a legal prefix character (ACGTacgt)
__device__ __forceinline__ uint8_t code_entry(uint32_t c) {
  uint32_t fwd = c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 0u;
  uint32_t rc = c == 'A' ? 3u : c == 'C' ? 2u : c == 'G' ? 1u : 0u;
  uint32_t u = c & 0xDFu;  // fold lower case onto upper case
  uint32_t ok = (u == 'A' || u == 'C' || u == 'G' || u == 'T') ? 1u : 0u;
  uint32_t pd = u == 'C' ? 1u : u == 'G' ? 2u : u == 'T' ? 3u : 0u;
  return (uint8_t)(fwd | (rc << 2) | ((ok ? pd : 0u) << 4) | (ok << 6));
}

// The smaller of two k-mer words as ONE v_min_f64 instead of v_cmp_lt_u64 + 2 x v_cndmask_b32.
// Precondition: a, b < 2^62 (2K <= 62: K is validated once, nq_api.hip derive()).  Then the sign bit is 0 and
// bit 62 is 0, so the exponent field is never all ones (no NaN, no infinity), and for non-negative doubles the
// IEEE order is the integer order of the bit patterns: the instruction returns one of its inputs bit for bit.
// Words below 2^52 are subnormal patterns: kernels are compiled with the 64-bit denormal mode that keeps them
// (.amdhsa_float_denorm_mode_16_64 3, no fast-math or flush option in HIPFLAGS; tests/test_gpu_canonical_min.py
// pins it).  Inline asm, not __builtin_fmin: in IEEE mode the compiler would canonicalise both inputs first.
__device__ __forceinline__ uint64_t min62(uint64_t a, uint64_t b) {
  uint64_t r;
  asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

// slot + fingerprint of a canonical k-mer and the per-slot min (:346-355)
// hsel: 0 = sk holds all F cells; 1 / 2 = sk holds the lower / upper half of the slots (S = 16: the
// cells of a whole sketch do not fit LDS) and k-mers of the other half change nothing
__device__ __forceinline__ void sketch_update(uint64_t canon, const Derived &d, uint32_t *sk, bool live, uint32_t hsel = 0) {
  uint32_t slot = slot_of(canon, d.S);
  uint32_t fp = fingerprint(rev64(canon), d.M, d.mask_m, d.max_rem);
  if (hsel) {  // uniform
    live = live && (slot >> (d.S - 1)) == hsel - 1u;
    slot &= (d.F >> 1) - 1u;
  }
  fp = live ? fp : kEmpty32;  // a min with "empty" changes nothing
  atomicMin(&sk[slot], fp);
}

// a * b (32 x 32 -> 64) and a * b + c as ONE v_mad_u64_u32 each: the empty asm makes the whole 64-bit
// result "used", so the compiler cannot narrow the expression back into v_mul_lo_u32 + adds
__device__ __forceinline__ uint64_t mul64(uint32_t a, uint32_t b) {
  uint64_t r = (uint64_t)a * (uint64_t)b;
  asm("" : "+v"(r));
  return r;
}
__device__ __forceinline__ uint64_t mad64(uint32_t a, uint32_t b, uint64_t c) {
  uint64_t r = (uint64_t)a * (uint64_t)b + c;
  asm("" : "+v"(r));
  return r;
}

// One xorshift-multiply round of mix64 (src/niqki_index.cpp:292,:301): x = ((x >> 32) ^ x) * c with c
// = chi:clo.  The low 32 bits of the product of the high words' cross terms ride in the addend.
__device__ __forceinline__ void mix_round(uint32_t &lo, uint32_t &hi, uint32_t clo, uint32_t chi) {
  const uint32_t y = lo ^ hi;
  const uint64_t t = mul64(hi, clo);
  const uint64_t p = mad64(y, chi, t);   // low word: y * chi + hi * clo
  const uint64_t q = mul64(y, clo);
  lo = (uint32_t)q;
  hi = (uint32_t)p + (uint32_t)(q >> 32);
}
// the same round when only the high word of the product is wanted: lo32(y * chi) + lo32(hi * clo) +
// hi32(y * clo) mod 2^32.  The v_mul_hi rides in the LOW word of the first mad's addend (carries only go
// into the high words, which are dropped), so the addend's high word may hold anything: it is left
// unwritten, no v_mov.  4 instructions instead of 5.
__device__ __forceinline__ uint32_t mix_round_hi(uint32_t lo, uint32_t hi, uint32_t clo, uint32_t chi) {
  typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));
  const uint32_t y = lo ^ hi;
  u32x2_t a = __builtin_nondeterministic_value(a);   // (any value, but a defined one)
  a.x = __umulhi(y, clo);
  const uint64_t t = mad64(hi, clo, __builtin_bit_cast(uint64_t, a));
  return (uint32_t)mad64(y, chi, t);
}
// High word of rev64(canon) as chains of v_mad_u64_u32: the filter hash of the long-record loop without the word it
// hands to its candidate stack (rev64_hi_mad_x1, nq_sketch.hip): nq_probe.hip, tools/ubench_occupancy.hip
__device__ __forceinline__ uint32_t rev64_hi_mad(uint64_t canon) {
  uint32_t lo = (uint32_t)canon, hi = (uint32_t)(canon >> 32);
  mix_round(lo, hi, (uint32_t)kRevMul, (uint32_t)(kRevMul >> 32));
  return mix_round_hi(lo, hi, (uint32_t)kRevMul, (uint32_t)(kRevMul >> 32));
}

// 64-bit shifts the compiler cannot look into (it otherwise re-derives halves of the result with extra
// instructions)
__device__ __forceinline__ uint64_t shl2_64(uint64_t x) {
  uint64_t r;
  asm("v_lshlrev_b64 %0, 2, %1" : "=v"(r) : "v"(x));
  return r;
}
__device__ __forceinline__ uint64_t shr2_64(uint64_t x) {
  uint64_t r;
  asm("v_lshrrev_b64 %0, 2, %1" : "=v"(r) : "v"(x));
  return r;
}
// (x << 2) + e in one instruction: the forward roll with a whole code table entry as the addend
__device__ __forceinline__ uint64_t shl2_add64(uint64_t x, uint64_t e) {
  uint64_t r;
  asm("v_lshl_add_u64 %0, %1, 2, %2" : "=v"(r) : "v"(x), "v"(e));
  return r;
}

// Orders the wave's LDS instructions on either side in the instruction stream without waiting for
// them: the LDS serves one wave's instructions in issue order, so a later instruction of ANY lane
// sees the effect of an earlier one of any lane.
__device__ __forceinline__ void wave_lds_order() {
  __builtin_amdgcn_wave_barrier();
  asm volatile("" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}

}  // namespace nq
