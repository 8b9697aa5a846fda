// nq_sketch.hip -- kernel #1/#2: canonical k-mer rolling hash, per-slot
// HyperMinHash min reduction in LDS, and densification, for gfx950.
//
// Replaces Index::compute_sketch (src/niqki_index.cpp:335-358, with
// update_kmer :225-229, update_kmer_RC :233-236, str2numstrand :255-273,
// rcb :240-250, revhash64/unrevhash64 :291-305, get_fingerprint :277-287) and
// Index::sketch_densification (:313-331).
//
// Shape: one workgroup per sketch (times `splits` for long single records).
// The F = 2^S sketch cells live in LDS as u32 with 0xFFFFFFFF (= int32 -1)
// for "empty", so the per-slot minimum is one unsigned ds_min_u32.  A record
// is cut into chunks of CHUNK k-mers; each lane rolls one chunk: K-1 cheap
// warm-up steps rebuild the forward / reverse-complement words (a k-mer only
// depends on its own K bases, see DESIGN.md "positional codes"), then CHUNK
// hash steps.  The kernel is integer-ALU bound (4 64-bit multiplies per
// k-mer), HBM traffic is 1 byte per base.
//
// This file: sketch_kernel and launch_sketch, which carries out a SketchPlan (nq_sketch_plan.h) with this kernel
// or those of nq_sketch_reads.hip (one wavefront per short record) and nq_densify.hip (densification alone).
#include "nq_kernels.h"
#include "nq_sketch_lines.h"
#include "nq_sketch_ops.h"
#include "../../include/niqki_hip.h"

#include <cstdlib>

namespace nq {

// 16 bytes of a byte stream that starts at an arbitrary address: the stream is
// fetched as dword-aligned uint4 loads and re-aligned with v_alignbyte.  Two loads are
// in flight: the one next16() issues is consumed by the call after it, so a caller that
// does a group's worth of work between calls never waits for memory.  Reads at most 35
// bytes past the last byte handed out (NIQKI_SEQ_PAD covers the end of the buffer).
struct ByteStream {
  const uint32_t *q;  // dword-aligned cursor
  uint32_t sh;        // byte phase 0..3
  uint4 cur, nxt;
  __device__ __forceinline__ void open(const uint8_t *p) {
    uintptr_t a = (uintptr_t)p;
    sh = (uint32_t)(a & 3u);
    q = (const uint32_t *)(a & ~(uintptr_t)3);
    cur = *(const uint4 *)q;  // dword aligned 16-byte loads
    nxt = *(const uint4 *)(q + 4);
    q += 8;
  }
  // returns the next 16 stream bytes as 4 dwords (little endian); loads never go past qmax (a lane
  // that steps through more groups than its own chunk holds, beside lanes with longer chunks)
  __device__ __forceinline__ uint4 next16(const uint32_t *qmax = nullptr) {
    const uint4 nn = *(const uint4 *)((qmax && q > qmax) ? qmax : q);
    q += 4;
    uint4 r;
    r.x = __builtin_amdgcn_alignbyte(cur.y, cur.x, sh);
    r.y = __builtin_amdgcn_alignbyte(cur.z, cur.y, sh);
    r.z = __builtin_amdgcn_alignbyte(cur.w, cur.z, sh);
    r.w = __builtin_amdgcn_alignbyte(nxt.x, cur.w, sh);
    cur = nxt;
    nxt = nn;
    return r;
  }
};

__device__ __forceinline__ uint32_t dword_of(const uint4 &v, int i) {
  return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w;
}

// In-LDS densification, pass-parallel restatement of the serial loop at
// src/niqki_index.cpp:313-331 (equivalence: DESIGN.md "densification").
// Within one pass every cell occupied at pass start proposes itself to its
// target cell with atomicMin of (1<<31 | source index << W | value); real
// values are < 2^W so occupied targets are never changed, and among several
// proposals the smallest source index wins, which is the serial loop's
// first-writer rule.  Returns with cells still empty only where the reference
// would loop forever (F consecutive passes without a fill prove a fixpoint).
template <int BLOCK>
__device__ __forceinline__ void densify_lds(uint32_t *sk, const Derived &d, uint32_t *s_flag) {
  const uint32_t F = d.F;
  const uint32_t tid = threadIdx.x;
  // count empties
  uint32_t local = 0;
  for (uint32_t i = tid; i < F; i += BLOCK) local += (sk[i] == kEmpty32);
  if (tid == 0) { s_flag[0] = 0; s_flag[1] = 0; }
  __syncthreads();
  if (local) atomicAdd(&s_flag[0], local);
  __syncthreads();
  uint32_t empty = s_flag[0];
  if (empty == 0 || empty == F) return;
  uint32_t step = 0, idle = 0;
  while (true) {
    // propose: an empty cell remembers the smallest source cell that points at it (the
    // first writer of the reference's ascending loop); occupied cells hold values below
    // 2^31 and are left alone by the min.  No assumption on the value range: after
    // niqki_select_best_H cells may exceed 2^W.
    for (uint32_t i = tid; i < F; i += BLOCK) {
      uint32_t v = sk[i];
      if (v < 0x80000000u) {
        // hash_family(v, step) % F, src/niqki_index.cpp:308-310,:319 (low bits only)
        uint32_t t = ((uint32_t)unrev64(v) + step * (uint32_t)rev64(v)) & (F - 1u);
        atomicMin(&sk[t], 0x80000000u | i);
      }
    }
    __syncthreads();
    // resolve: copy from the winning source (occupied since before this pass, so no
    // other thread writes it now)
    uint32_t filled = 0;
    for (uint32_t i = tid; i < F; i += BLOCK) {
      uint32_t v = sk[i];
      if (v >= 0x80000000u && v != kEmpty32) { sk[i] = sk[v & 0x7FFFFFFFu]; ++filled; }
    }
    if (filled) atomicAdd(&s_flag[1], filled);
    __syncthreads();
    uint32_t tot = s_flag[1];
    __syncthreads();
    if (tid == 0) s_flag[1] = 0;
    empty -= tot;
    ++step;
    idle = tot ? 0u : idle + 1u;
    if (empty == 0 || idle >= F) break;
    __syncthreads();
  }
}

// Densification over DISTINCT VALUES (short-read path).  A fill copies a value,
// so every copy of a value proposes the same target in a pass and only the copy
// with the smallest index can win: it is enough to track, per fingerprint value v,
// mi[v] = smallest cell index holding v (at pass start), and the two hash words of
// v, which never change.  A pass is then one proposal per distinct value (~120 for a
// 150-base read) instead of one per occupied cell (up to F), with the same result
// as densify_lds.  aux: 3*R words of LDS (mi, A = low word of unrev(v), B = low word
// of rev(v)).
template <int BLOCK>
__device__ __forceinline__ void densify_lds_distinct(uint32_t *sk, const Derived &d, uint32_t *s_flag, uint32_t *aux) {
  const uint32_t F = d.F, R = d.R, W = d.W;
  const uint32_t tid = threadIdx.x;
  uint32_t *mi = aux, *ha = aux + R, *hb = aux + 2 * R;
  uint32_t local = 0;
  for (uint32_t i = tid; i < F; i += BLOCK) local += (sk[i] == kEmpty32);
  for (uint32_t v = tid; v < R; v += BLOCK) mi[v] = kEmpty32;
  if (tid == 0) { s_flag[0] = 0; s_flag[1] = 0; }
  __syncthreads();
  if (local) atomicAdd(&s_flag[0], local);
  for (uint32_t i = tid; i < F; i += BLOCK) {
    uint32_t v = sk[i];
    if (v != kEmpty32) atomicMin(&mi[v], i);
  }
  __syncthreads();
  uint32_t empty = s_flag[0];
  if (empty == 0 || empty == F) return;
  for (uint32_t v = tid; v < R; v += BLOCK)
    if (mi[v] != kEmpty32) { ha[v] = (uint32_t)unrev64(v); hb[v] = (uint32_t)rev64(v); }
  uint32_t step = 0, idle = 0;
  while (true) {
    for (uint32_t v = tid; v < R; v += BLOCK) {
      const uint32_t m = mi[v];
      if (m != kEmpty32) {
        const uint32_t t = (ha[v] + step * hb[v]) & (F - 1u);  // hash_family(v, step) % F, :308-310,:319
        if (sk[t] >= 0x80000000u) atomicMin(&sk[t], 0x80000000u | (m << W) | v);
      }
    }
    __syncthreads();
    uint32_t filled = 0;
    for (uint32_t v = tid; v < R; v += BLOCK) {
      const uint32_t m = mi[v];
      if (m != kEmpty32) {
        const uint32_t t = (ha[v] + step * hb[v]) & (F - 1u);
        if (sk[t] == (0x80000000u | (m << W) | v)) {
          sk[t] = v;
          if (t < m) mi[v] = t;
          ++filled;
        }
      }
    }
    if (filled) atomicAdd(&s_flag[1], filled);
    __syncthreads();
    const uint32_t tot = s_flag[1];  // every proposed-to cell now holds its winner's value
    __syncthreads();
    if (tid == 0) s_flag[1] = 0;
    empty -= tot;
    ++step;
    idle = tot ? 0u : idle + 1u;
    if (empty == 0 || idle >= F) break;
    __syncthreads();
  }
}

// Rolling update of the forward / reverse-complement words with the code-table
// entry `e` of the incoming base (src/niqki_index.cpp:225-236) and the canonical
// k-mer (:345).  KFIX != 0 fixes K at compile time (K = 31: constant shifts).
template <int KFIX>
__device__ __forceinline__ uint64_t roll_step(uint32_t e, uint64_t &fw, uint64_t &rc, const Derived &d,
                                              uint32_t rc_shift) {
  if (KFIX) {
    constexpr uint64_t mask = (1ULL << (2 * KFIX)) - 1ULL;
    fw = ((fw << 2) | (uint64_t)(e & 3u)) & mask;
    rc = (rc >> 2) | ((uint64_t)((e >> 2) & 3u) << (2 * KFIX - 2));
  } else {
    fw = ((fw << 2) | (uint64_t)(e & 3u)) & d.kmer_mask;
    rc = (rc >> 2) | ((uint64_t)((e >> 2) & 3u) << rc_shift);
  }
  return min62(fw, rc);
}

// ---- the filtered long-record path ------------------------------------------------------------
// Issue costs on gfx950 (tools/ubench_opcodes.hip, profiles/r03_opcode_costs.txt): v_add / v_sub /
// v_and / v_or / v_xor / v_mov / v_lshrrev_b32 take ~2.4 SIMD cycles per wave instruction, EVERY other
// vector opcode ~4.3 -- 32-bit multiplies, v_mad_u64_u32 (4.4), 64-bit shifts and compares included.
// So the step below is written for the fewest instructions, multiplies are not what to avoid:
//   * the code table for K = 31 holds 8-byte entries {forward code, rc code << 30}: the forward update is
//     ONE v_lshl_add_u64 with the entry as the 64-bit addend plus the `and` of the high word (the rc code
//     lands in bits 2K, 2K + 1, above the mask), the reverse update an `or` of the high word and one 64-bit
//     shift (4 instructions instead of 7); the canonical choice is one v_min_f64 (min62());
//   * the 64 x 64 -> 64 multiplies run as chains of v_mad_u64_u32 (the addend carries the cross terms);
//   * candidates are stored under the exec mask (compare, 2 x mbcnt, 1 address instruction) into a
//     wave-private LIFO stack whose top lives in a scalar register: no ring wrap, no scratch slot.

typedef __attribute__((address_space(3))) uint32_t lds_u32_t;
typedef __attribute__((address_space(3))) uint64_t lds_u64_t;

// High word of rev64(canon): enough to bound the fingerprint from below.
__device__ __forceinline__ uint32_t rev64_hi(uint64_t canon) {
  uint64_t x = ((canon >> 32) ^ canon) * kRevMul;
  x = ((x >> 32) ^ x) * kRevMul;
  return (uint32_t)(x >> 32);
}

// The same as chains of v_mad_u64_u32, handing out the word after the first round: x1 = ((canon >> 32) ^ canon) * kRevMul.  The filtered fast loops
// push x1, not canon, and candidate_update() finishes both of a candidate's hashes from it.
__device__ __forceinline__ uint32_t rev64_hi_mad_x1(uint64_t canon, uint64_t &x1) {
  uint32_t lo = (uint32_t)canon, hi = (uint32_t)(canon >> 32);
  mix_round(lo, hi, (uint32_t)kRevMul, (uint32_t)(kRevMul >> 32));
  x1 = ((uint64_t)hi << 32) | lo;
  return mix_round_hi(lo, hi, (uint32_t)kRevMul, (uint32_t)(kRevMul >> 32));
}
// mix_round without the xor: x = x * c, a plain 64 x 64 -> 64 product (3 x v_mad_u64_u32 + 1 add)
__device__ __forceinline__ void mul_round(uint32_t &lo, uint32_t &hi, uint32_t clo, uint32_t chi) {
  const uint64_t t = mul64(hi, clo);
  const uint64_t p = mad64(lo, chi, t);   // low word: lo * chi + hi * clo
  const uint64_t q = mul64(lo, clo);
  lo = (uint32_t)q;
  hi = (uint32_t)p + (uint32_t)(q >> 32);
}
// The two multipliers are inverses of each other mod 2^64 (that is what makes unrevhash64 the inverse of revhash64,
// src/niqki_index.cpp:291-305), so with x1 = fold(canon) * kRevMul, fold(x) = x ^ (x >> 32):
//   fold(canon) * kUnrevMul = x1 * kUnrevMul * kUnrevMul = x1 * kUnrevMul2
// and the slot hash's first round is a plain product of the word the filter already has.
constexpr uint64_t kUnrevMul2 = kUnrevMul * kUnrevMul;
static_assert(kRevMul * kUnrevMul == 1ULL, "candidate_update() finishes the slot hash from the filter's first round: the multipliers must be inverses mod 2^64");
static_assert(kUnrevMul2 == 0xEB9041BCFCD1CDD9ULL, "kUnrevMul squared mod 2^64");

constexpr uint32_t kFastKMin = 17;   // smallest K of the fast filtered path: the rc code, at bit 2K - 2 of the reverse word, is in its high word

// Candidate store of one step: lanes whose hash word hh is below thr push canon (the fast loops: the hash's first
// round x1, rev64_hi_mad_x1()) onto the wave's stack (LDS byte address of its top in `top`, wave-uniform, advanced here).  gfx950 wants two wait states
// between a vector compare and a vector instruction that reads its mask as an operand (the mbcnt): the two
// scalar instructions in between are that.
__device__ __forceinline__ void push_candidates(uint32_t hh, uint32_t thr, uint64_t canon, uint32_t &top) {
  uint32_t n, r;
  uint64_t save;
  asm volatile(
      "v_cmp_gt_u32 vcc, %[thr], %[hh]\n\t"
      "s_and_saveexec_b64 %[save], vcc\n\t"
      "s_bcnt1_i32_b64 %[n], vcc\n\t"
      "v_mbcnt_lo_u32_b32 %[r], vcc_lo, 0\n\t"
      "v_mbcnt_hi_u32_b32 %[r], vcc_hi, %[r]\n\t"
      "v_lshl_add_u32 %[r], %[r], 3, %[top]\n\t"
      "ds_write_b64 %[r], %[canon]\n\t"
      "s_mov_b64 exec, %[save]\n\t"
      "s_lshl3_add_u32 %[top], %[n], %[top]"
      : [n] "=&s"(n), [r] "=&v"(r), [save] "=&s"(save), [top] "+s"(top)
      : [thr] "s"(thr), [hh] "v"(hh), [canon] "v"(canon)
      : "vcc", "scc", "memory");
}

// LDS layout of sketch_kernel (byte offsets from the start of its dynamic LDS, which is LDS address 0: the
// kernel has no static LDS): the K = 31 code table first, so that a look-up address is the byte value
// times 8 (one SDWA shift), and the sketch cells at a fixed offset (an instruction immediate).
constexpr uint32_t kLut64Off = 0;       // 256 x {forward code, rc code << 30}
constexpr uint32_t kLutOff = 2048;      // 256 code_entry bytes
constexpr uint32_t kFlagOff = 2304;     // 4 words
constexpr uint32_t kCellOff = 2320;     // the sketch cells; behind them the distinct-value tables or the candidate stacks
                                        // (kStack, kLevelStateWords, kLevelLdsBytes: nq_sketch_plan.h)

// byte B of w, times 8: the offset of its 8-byte code table entry
template <int B>
__device__ __forceinline__ uint32_t byte_x8(uint32_t w) {
  uint32_t r;
  if (B == 0) asm("v_lshlrev_b32_sdwa %0, 3, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_0" : "=v"(r) : "v"(w));
  if (B == 1) asm("v_lshlrev_b32_sdwa %0, 3, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_1" : "=v"(r) : "v"(w));
  if (B == 2) asm("v_lshlrev_b32_sdwa %0, 3, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_2" : "=v"(r) : "v"(w));
  if (B == 3) asm("v_lshlrev_b32_sdwa %0, 3, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_3" : "=v"(r) : "v"(w));
  return r;
}
// the 16 code table entries of 16 stream bytes
__device__ __forceinline__ void lut64_16(const uint4 &v, uint32_t lds0, uint64_t (&e)[16]) {
#define NQ_E(J, W, B) e[J] = *(lds_u64_t *)(uintptr_t)(lds0 + kLut64Off + byte_x8<B>(W));
  NQ_E(0, v.x, 0) NQ_E(1, v.x, 1) NQ_E(2, v.x, 2) NQ_E(3, v.x, 3)
  NQ_E(4, v.y, 0) NQ_E(5, v.y, 1) NQ_E(6, v.y, 2) NQ_E(7, v.y, 3)
  NQ_E(8, v.z, 0) NQ_E(9, v.z, 1) NQ_E(10, v.z, 2) NQ_E(11, v.z, 3)
  NQ_E(12, v.w, 0) NQ_E(13, v.w, 1) NQ_E(14, v.w, 2) NQ_E(15, v.w, 3)
#undef NQ_E
}
// ... of the first (HALF = 0) or last eight of them, into e[0..8) or e[8..16)
template <int HALF>
__device__ __forceinline__ void lut64_8(const uint4 &v, uint32_t lds0, uint64_t (&e)[16]) {
#define NQ_E(J, W, B) e[J] = *(lds_u64_t *)(uintptr_t)(lds0 + kLut64Off + byte_x8<B>(W));
  if (HALF == 0) {
    NQ_E(0, v.x, 0) NQ_E(1, v.x, 1) NQ_E(2, v.x, 2) NQ_E(3, v.x, 3)
    NQ_E(4, v.y, 0) NQ_E(5, v.y, 1) NQ_E(6, v.y, 2) NQ_E(7, v.y, 3)
  } else {
    NQ_E(8, v.z, 0) NQ_E(9, v.z, 1) NQ_E(10, v.z, 2) NQ_E(11, v.z, 3)
    NQ_E(12, v.w, 0) NQ_E(13, v.w, 1) NQ_E(14, v.w, 2) NQ_E(15, v.w, 3)
  }
#undef NQ_E
}
// ... of the four bytes of one dword, into e[0..4) (HALF = 0) or e[4..8)
template <int HALF>
__device__ __forceinline__ void lut64_4(uint32_t w, uint32_t lds0, uint64_t (&e)[8]) {
#define NQ_E(J, B) e[4 * HALF + J] = *(lds_u64_t *)(uintptr_t)(lds0 + kLut64Off + byte_x8<B>(w));
  NQ_E(0, 0) NQ_E(1, 1) NQ_E(2, 2) NQ_E(3, 3)
#undef NQ_E
}

// slot + fingerprint + per-slot min of up to 64 candidates (:346-355), whole sketch in LDS at kCellOff
// upwards (S <= 15).  A candidate comes off the stack as x1, the word after the first round of its revhash64
// (rev64_hi_mad_x1()): the hash takes its second round from there (passing the filter's second round through the
// stack as well would cost more register traffic than those 5 instructions), and the slot hash's first round is
// x1 * kUnrevMul2, 4 instructions.  22 vector instructions per drain of 64 candidates, 27 when both hashes started
// from canon (profiles/r10_sketch_cost_model.txt).
__device__ __forceinline__ void candidate_update(uint64_t x1, const Derived &d, uint32_t lds0, bool live) {
  uint32_t lo = (uint32_t)x1, hi = (uint32_t)(x1 >> 32);
  uint32_t ulo = lo, uhi = hi;
  mul_round(ulo, uhi, (uint32_t)kUnrevMul2, (uint32_t)(kUnrevMul2 >> 32));
  const uint32_t uh = mix_round_hi(ulo, uhi, (uint32_t)kUnrevMul, (uint32_t)(kUnrevMul >> 32));
  mix_round(lo, hi, (uint32_t)kRevMul, (uint32_t)(kRevMul >> 32));
  // get_fingerprint (:277-287) of h = hi : lo ^ hi.  A candidate's high word is below 2^29 and, but for one
  // hash in 2^29, not 0: its leading zeros are those of the high word (one v_ffbh); the rare zero high word
  // takes the general form for the whole wave.
  const uint32_t hl = lo ^ hi;
  uint32_t lz = (uint32_t)__builtin_clz(hi);
  if (__builtin_expect(__any(hi == 0u), 0)) lz = clz64(((uint64_t)hi << 32) | hl);
  const uint32_t rem = lz < d.max_rem ? d.max_rem - lz : 0u;
  uint32_t fp = (hl & d.mask_m) + (rem << d.M);
  fp = live ? fp : kEmpty32;  // a min with "empty" changes nothing
  const uint32_t cell = (uh >> (30u - d.S)) & ~3u;   // byte offset of the slot's cell
  __hip_atomic_fetch_min((lds_u32_t *)(uintptr_t)(lds0 + kCellOff + cell), fp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// All records of one sketch, this workgroup's share of the chunks.
// FILTER (long inputs only): a k-mer whose hash has fewer than T leading zeros
// (hi word >= thr) has a larger fingerprint than any k-mer with at least T, so it
// can only matter for a slot that no such k-mer reaches.  Those k-mers (7 of 8 at
// T = 3) skip the slot hash and the LDS min; the others are pushed onto a
// wave-private stack and finished 64 at a time.  The caller re-runs the records
// unfiltered if any slot is still empty afterwards, so the result is exact.
// GROUPS: most 16-base groups per chunk; a record's chunks are sized so that its last round of
// chunks over the workgroup's lanes is nearly full (5 Mbp over 1024 lanes: 10 rounds of 496 k-mers).
// FAST_OK: the fast form of the filtered loop is allowed -- the workgroup keeps all F cells (no half of the slots)
// and the kernel's LDS layout starts at LDS address 0 (checked at kernel entry), so the fast path addresses the
// code table and the cells with instruction immediates.
// (always inline: a call would put the kernel's arguments in scratch memory and their values in vector registers)
template <int BLOCK, int GROUPS, int KFIX, bool FILTER, bool FAST_OK>
__device__ __forceinline__ void roll_records(const SketchArgs &a, uint32_t entry, uint32_t part, uint32_t *sk, const uint8_t *lut,
                             uint64_t *stack_base, uint32_t thr, uint32_t hsel) {
  const Derived &d = a.d;
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  const uint32_t Km1 = d.K - 1u;
  const uint32_t rc_shift = 2u * d.K - 2u;
  // 8-byte code table, mad chains, S <= 15.  K = 31 is a compile-time specialisation; the KFIX = 0 kernel takes
  // the same path for any K in 17..31 (kFastKMin: the rc code of a table entry must sit in its high word): the
  // shifts by 2 are immediates whatever K, only the table's contents, the mask of the forward word's high half
  // and the position the warm-up starts at depend on K.
  constexpr bool FAST = FILTER && FAST_OK && (KFIX == 31 || KFIX == 0);
  const bool fast_k = KFIX == 31 || (d.K >= kFastKMin && d.K <= 31u);
  const uint32_t mask_hi = KFIX == 31 ? 0x3FFFFFFFu : __builtin_amdgcn_readfirstlane((uint32_t)(d.kmer_mask >> 32));
  const uint64_t fw_mask = ((uint64_t)mask_hi << 32) | 0xFFFFFFFFull;
  const uint32_t warm_back = KFIX == 31 ? 0u : 31u - d.K;   // the 30 warm-up steps start this many bases before the chunk
  constexpr uint32_t lds0 = 0;
  uint64_t *stack = stack_base + (tid >> 6) * kStack;
  // LDS byte address of the stack's bottom / top (wave-uniform: scalar registers)
  const uint32_t bottom = FILTER ? __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(lds_u64_t *)stack) : 0u;
  uint32_t top = bottom;
  const uint32_t lane8 = lane * 8u;
  auto drain64 = [&]() {   // the 64 youngest candidates
    const uint64_t c = *(lds_u64_t *)(uintptr_t)(top - 512u + lane8);
    if (FAST) candidate_update(c, d, lds0, true);
    else sketch_update(c, d, sk, true, hsel);
    top -= 512u;
  };
  auto drain_rest = [&]() {   // fewer than 64 left
    const uint32_t n = (top - bottom) >> 3;
    const bool live = lane < n;
    const uint64_t c = live ? stack[lane] : 0ull;
    if (FAST) candidate_update(c, d, lds0, live);
    else sketch_update(c, d, sk, live, hsel);
    top = bottom;
  };

  uint32_t r0 = a.entry_rec ? a.entry_rec[entry] : entry;
  uint32_t r1 = a.entry_rec ? a.entry_rec[entry + 1] : entry + 1;
  for (uint32_t rec = r0; rec < r1; ++rec) {
    const uint64_t b0 = a.rec_off[rec], b1 = a.rec_off[rec + 1];
    const uint64_t len = b1 - b0;
    if (len <= d.K) continue;              // src/niqki_index.cpp:395,:450
    const uint64_t n_kmers = len - d.K;    // last k-mer skipped, :342
    // chunk length: the fewest rounds of GROUPS-group chunks, then the shortest chunks that still fit them
    uint32_t groups = 1;
    if (GROUPS > 1) {
      const uint64_t share = n_kmers / a.splits + 1u;
      const uint64_t rounds = (share + (uint64_t)BLOCK * 16u * GROUPS - 1u) / ((uint64_t)BLOCK * 16u * GROUPS);
      groups = (uint32_t)((share + rounds * BLOCK * 16u - 1u) / (rounds * BLOCK * 16u));
      groups = groups < 1u ? 1u : groups > (uint32_t)GROUPS ? (uint32_t)GROUPS : groups;
      groups = __builtin_amdgcn_readfirstlane(groups);
    }
    const uint32_t CHUNK = 16u * groups;
    const uint64_t n_chunks = (n_kmers + CHUNK - 1) / CHUNK;
    const uint64_t c_lo = n_chunks * part / a.splits;
    const uint64_t c_hi = n_chunks * (part + 1) / a.splits;
    const uint8_t *base = a.seqs + b0;
    // Whole waves step together (uniform loop control: the filtered path's stack
    // is wave-collective and its top lives in a scalar register).
    const uint32_t wave0 = __builtin_amdgcn_readfirstlane(tid & ~63u);
    for (uint64_t cb = c_lo + wave0; cb < c_hi; cb += BLOCK) {
      const uint64_t c = cb + lane;
      const bool alive = c < c_hi;
      const uint64_t i0 = (alive ? c : c_lo) * CHUNK;
      const uint64_t left = n_kmers - i0;
      const uint32_t cnt = alive ? (left < CHUNK ? (uint32_t)left : CHUNK) : 0u;
      // ---- warm-up: K-1 rolling updates from zero rebuild both words ----
      // Positions < K-1 of a record carry the str2numstrand digits
      // (case-insensitive; any other byte among the first K-1 zeroes all of
      // them, :255-273) and their complements (rcb, :240-250); every later
      // position carries the codes of the rolling tables.
      uint64_t fw = 0, rc = 0;
      if (FAST && fast_k && __all(i0 >= Km1 + warm_back)) {
        // no lane of the wave starts inside a record's first K-1 positions (all chunks but a record's
        // first): the 30 steps are plain rolling updates from the 8-byte code table, 3 instructions each.
        // (K < 31: 30 steps all the same, from 31 - K bases further back -- the reverse word's older codes
        // leave at the bottom.  The forward word is left unmasked: the entries' rc codes and the older
        // forward codes sit at bit 2K and above, where sums only carry upwards, and both forms of the hash
        // step mask the word after their own shift.)
        ByteStream ws;
        ws.open(base + i0 - warm_back);
        uint64_t ew[32];
        {
          uint64_t e16[16];
          lut64_16(ws.next16(), lds0, e16);
#pragma unroll
          for (int j = 0; j < 16; ++j) ew[j] = e16[j];
          lut64_16(ws.next16(), lds0, e16);
#pragma unroll
          for (int j = 0; j < 16; ++j) ew[16 + j] = e16[j];
        }
#pragma unroll
        for (int j = 0; j < 30; ++j) {
          fw = shl2_add64(fw, ew[j]);
          rc = shr2_64(rc | (ew[j] & 0xFFFFFFFF00000000ULL));   // (rc < 2^2K: the code's two bits are free)
        }
      } else {
        uint32_t ok = 1;
        if (i0 < Km1) {
          ByteStream ps;
          ps.open(base);
          uint4 p0 = ps.next16(), p1 = ps.next16();
#pragma unroll
          for (int j = 0; j < 32; ++j) {
            uint32_t w = dword_of(j < 16 ? p0 : p1, (j & 15) >> 2);
            uint32_t e = lut[(w >> (8 * (j & 3))) & 0xFFu];
            if ((uint32_t)j < Km1) ok &= (e >> 6) & 1u;
          }
        }
        ByteStream ws;
        ws.open(base + i0);
        uint4 g0 = ws.next16(), g1 = ws.next16();
        uint32_t ew[32];  // all table look-ups first, then the dependent updates
#pragma unroll
        for (int j = 0; j < 32; ++j) {
          uint32_t w = dword_of(j < 16 ? g0 : g1, (j & 15) >> 2);
          ew[j] = lut[(w >> (8 * (j & 3))) & 0xFFu];
        }
#pragma unroll
        for (int j = 0; j < 32; ++j) {
          if ((uint32_t)j < Km1) {
            const uint32_t e = ew[j];
            const bool pfx = i0 + (uint32_t)j < Km1;
            uint32_t dgt = ok ? ((e >> 4) & 3u) : 0u;
            uint32_t cf = pfx ? dgt : (e & 3u);
            uint32_t cr = pfx ? (3u - dgt) : ((e >> 2) & 3u);
            fw = (fw << 2) | cf;
            rc = (rc >> 2) | ((uint64_t)cr << rc_shift);
          }
        }
      }
      // ---- CHUNK hash steps, bases i0+K-1 .. ----
      // Per 16-byte group the 16 table look-ups are issued together and one group
      // ahead of their use (LDS answers in order, so they return before the LDS
      // traffic of the group in between).
      if (FAST && fast_k && __all(cnt == CHUNK)) {
        // Every lane of the wave has a full chunk: no per-step liveness at all.  Group g's 16 bytes sit
        // in the five dwords at qa + 4g at byte phase sh; they are loaded a group ahead, and the eight
        // table entries of a half group are reloaded into their own registers as soon as the half is
        // used up (eight steps before they are needed again), so nothing is copied at the loop's end.
        // The loop reads at most 40 bytes past the chunk's last base (NIQKI_SEQ_PAD).
        const uintptr_t a0 = (uintptr_t)(base + i0 + Km1);
        const uint32_t sh = (uint32_t)(a0 & 3u);
        const uint32_t *qa = (const uint32_t *)(a0 & ~(uintptr_t)3);
        uint64_t e[16];
        {
          const uint4 A = *(const uint4 *)qa;
          const uint32_t B = qa[4];
          uint4 w;
          w.x = __builtin_amdgcn_alignbyte(A.y, A.x, sh);
          w.y = __builtin_amdgcn_alignbyte(A.z, A.y, sh);
          w.z = __builtin_amdgcn_alignbyte(A.w, A.z, sh);
          w.w = __builtin_amdgcn_alignbyte(B, A.w, sh);
          lut64_16(w, lds0, e);
        }
        auto step = [&](uint64_t ent, bool check) {
          // :225-229 and :233-236 with the entry's pre-placed codes
          // (the entry's rc code and any carry out of it land at bit 2K and above: the `and` clears them)
          rc = shr2_64(rc | (ent & 0xFFFFFFFF00000000ULL));
          fw = shl2_add64(fw, ent) & fw_mask;   // (only the high word's `and` is an instruction)
          uint64_t x1;
          const uint32_t hh = rev64_hi_mad_x1(min62(fw, rc), x1);   // :345
          push_candidates(hh, thr, x1, top);
          // two steps add at most 128 to fewer than 64.  Unlikely: the drain is laid out behind the loop,
          // the common path has no taken branch
          if (check && __builtin_expect(top >= bottom + 512u, 0)) {
            drain64();
            if (top >= bottom + 512u) drain64();
          }
        };
        for (uint32_t g = 0; g < groups; ++g) {
          qa += 4;
          const uint4 A = *(const uint4 *)qa;   // the next group's bytes
          const uint32_t B = qa[4];
#pragma unroll
          for (int j = 0; j < 8; ++j) step(e[j], (j & 1) != 0);
          uint4 w;
          w.x = __builtin_amdgcn_alignbyte(A.y, A.x, sh);
          w.y = __builtin_amdgcn_alignbyte(A.z, A.y, sh);
          w.z = __builtin_amdgcn_alignbyte(A.w, A.z, sh);
          w.w = __builtin_amdgcn_alignbyte(B, A.w, sh);
          lut64_8<0>(w, lds0, e);
#pragma unroll
          for (int j = 8; j < 16; ++j) step(e[j], (j & 1) != 0);
          lut64_8<1>(w, lds0, e);
        }
        continue;
      }
      ByteStream bs;
      bs.open(base + i0 + Km1);
      // last dword-aligned address a 16-byte load may start at: the record's end plus the pad
      const uint32_t *qmax = (const uint32_t *)(((uintptr_t)(base + len) + NIQKI_SEQ_PAD - 16) & ~(uintptr_t)3);
      uint32_t en[16];
      {
        const uint4 v = bs.next16(qmax);
#pragma unroll
        for (int j = 0; j < 16; ++j) en[j] = lut[(dword_of(v, j >> 2) >> (8 * (j & 3))) & 0xFFu];
      }
      // filtered: all lanes of the wave run the groups its longest chunk needs (the stack is wave-collective);
      // no lane reads more than two groups past its own bases
      uint32_t cnt_wave = cnt;
      if (FILTER) {
#pragma unroll
        for (int dd = 32; dd >= 1; dd >>= 1) {
          const uint32_t o = (uint32_t)__shfl_xor((int)cnt_wave, dd, 64);
          cnt_wave = o > cnt_wave ? o : cnt_wave;
        }
        cnt_wave = __builtin_amdgcn_readfirstlane(cnt_wave);
      }
      for (uint32_t g = 0; g < groups; ++g) {
        if (g * 16u >= cnt_wave) break;
        uint32_t e[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) e[j] = en[j];
        if ((g + 1) * 16u < cnt_wave) {
          const uint4 v = bs.next16(qmax);
#pragma unroll
          for (int j = 0; j < 16; ++j) en[j] = lut[(dword_of(v, j >> 2) >> (8 * (j & 3))) & 0xFFu];
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const uint64_t canon = roll_step<KFIX>(e[j], fw, rc, d, rc_shift);
          const bool live = g * 16u + (uint32_t)j < cnt;
          if (!FILTER) {
            sketch_update(canon, d, sk, live, hsel);
          } else {
            // dead steps get an all-ones hash word and never pass.  The stack's word is the one its drain takes:
            // x1 where that is candidate_update() (this loop serves the fast form's partial chunks too)
            if (FAST) {
              uint64_t x1;
              const uint32_t hh = rev64_hi_mad_x1(canon, x1);
              push_candidates(live ? hh : 0xFFFFFFFFu, thr, x1, top);
            } else {
              push_candidates(live ? rev64_hi(canon) : 0xFFFFFFFFu, thr, canon, top);
            }
            if (top >= bottom + 512u) drain64();
          }
        }
      }
    }
  }
  if (FILTER && top != bottom) drain_rest();
}

// ---- the line-aligned form of the fast filtered loop (1024 x 32 launch shape, K in 17..31) --------------------
// 16 bytes from any byte address (the hardware takes unaligned vector loads); loads exactly [p, p + 16)
__device__ __forceinline__ uint4 load16u(const uint8_t *p) {
  uint4 v;
  __builtin_memcpy(&v, p, 16);
  return v;
}
typedef uint32_t u32x32_t __attribute__((ext_vector_type(32)));   // a line in 32 registers that a uniform index reaches

// the 16 bytes at address x, of which only [x + dlt, ...) (dlt > 0) or (..., x + 16 + dlt) (dlt < 0) could be
// loaded, from x + dlt: moved back to their places, zeroes where nothing was loaded
__device__ __forceinline__ uint4 replace16(const uint4 &v, int dlt) {
  uint64_t lo = (uint64_t)v.x | ((uint64_t)v.y << 32), hi = (uint64_t)v.z | ((uint64_t)v.w << 32);
  if (dlt >= 16 || dlt <= -16) {
    lo = hi = 0;
  } else if (dlt > 0) {
    const uint32_t s = 8u * (uint32_t)dlt;
    if (s >= 64u) { hi = lo << (s - 64u); lo = 0; }
    else { hi = (hi << s) | (lo >> (64u - s)); lo <<= s; }
  } else if (dlt < 0) {
    const uint32_t s = 8u * (uint32_t)(-dlt);
    if (s >= 64u) { lo = hi >> (s - 64u); hi = 0; }
    else { lo = (lo >> s) | (hi << (64u - s)); hi >>= s; }
  }
  return make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
}

#ifdef NQ_SKETCH_CLOCK
// per workgroup of the line form: the 100 MHz tick before the loop, the one behind the barrier after it, and the tick at
// which each of its 16 waves leaves roll_records_lines (tools/ubench_sketch.hip: finish times per SIMD)
constexpr uint32_t kWaveTraceWgs = 512;
__device__ unsigned long long nq_sketch_wave[18 * kWaveTraceWgs];
#endif

// All records of one sketch, this workgroup's part, with the geometry of nq_sketch_lines.h: every lane owns one run
// of whole 128-byte lines of a record part, fetches each line once with eight back-to-back 16-byte loads and takes
// its 128 hash steps from registers: no re-alignment, no line shared between lanes, one warm-up per lane and
// record.  A round is one line per lane; the wave's lanes step together (the candidate stack is wave-collective).
//   * the plain round (every lane's whole line is hash bytes): the step of the chunked fast loop;
//   * the predicated round (a record's first and last line, lanes with one line fewer than their neighbours, lanes
//     without lines): the same step, but a dead step leaves the rolling words alone and its hash word is all ones, so
//     it never passes the filter.
// A line that does not lie inside the buffer (the buffer's alignment is unknown: its first and last line may not be
// whole) is loaded in 16-byte pieces clamped to [seqs, seqs + rec_off[end of this sketch's records] + NIQKI_SEQ_PAD):
// no byte outside is ever loaded.  Every load address comes from the helpers of nq_sketch_lines.h (warm_load, round_line,
// line_inside, clamp_piece), which the CPU test walks against the buffer.  Addresses become pointers as offsets from
// a.seqs: a pointer made from a bare integer would lose the global address space, and its loads would be flat loads,
// which the LDS look-ups' lgkmcnt waits wait for too.
// LEVELING (nq_sketch_lines.h): at the head of a round at which its progress has moved a step, and only there, a wave
// writes the progress to its word of the sixteen at LDS address `level_lds`, reads the four words of its SIMD and sets
// its issue priority by level_prio().  No wave waits for a word and no branch depends on another wave's: the words
// only choose the operand of s_setprio.  n_entry: the entry's hash bytes, the n the filter strength comes from.
template <int BLOCK, int KFIX>
__device__ __forceinline__ void roll_records_lines(const SketchArgs &a, uint32_t entry, uint32_t part, const uint8_t *lut,
                                   uint64_t *stack_base, uint32_t thr, uint64_t n_entry, uint32_t level_lds) {
  const Derived &d = a.d;
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  const uint32_t Km1 = d.K - 1u;
  const uint32_t rc_shift = 2u * d.K - 2u;
  const uint32_t mask_hi = KFIX == 31 ? 0x3FFFFFFFu : __builtin_amdgcn_readfirstlane((uint32_t)(d.kmer_mask >> 32));
  const uint64_t fw_mask = ((uint64_t)mask_hi << 32) | 0xFFFFFFFFull;
  constexpr uint32_t lds0 = 0;
  uint64_t *stack = stack_base + (tid >> 6) * (kStack + kLevelStateWords / 2);   // (behind every stack: the wave's leveling state)
  const uint32_t bottom = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(lds_u64_t *)stack);
  uint32_t top = bottom;
  const uint32_t lane8 = lane * 8u;
  auto drain64 = [&]() {   // the 64 youngest candidates
    const uint64_t c = *(lds_u64_t *)(uintptr_t)(top - 512u + lane8);
    candidate_update(c, d, lds0, true);
    top -= 512u;
  };

  const uint32_t r0 = a.entry_rec ? a.entry_rec[entry] : entry;
  const uint32_t r1 = a.entry_rec ? a.entry_rec[entry + 1] : entry + 1;
  // the pad behind this sketch's last record belongs to the buffer whatever follows: a bound that needs no record count
  const uint64_t end_off = a.rec_off[r1];
  // (the empty asm hides where the number came from: the compiler would otherwise fold a.seqs + (x - seqs_addr) back
  // into a pointer made from the integer x)
  uint64_t seqs_addr = (uint64_t)(uintptr_t)a.seqs;
  asm("" : "+s"(seqs_addr));
  const uint64_t buf_lo = seqs_addr, buf_hi = seqs_addr + end_off + NIQKI_SEQ_PAD;
  auto gptr = [&](uint64_t addr) { return a.seqs + (int64_t)(addr - seqs_addr); };
  // leveling: the wave's own state lives in LDS too, in the eight words behind its candidate stack; its address comes from
  // `bottom`, which the steps keep anyway.  The kernel has no register to spare across the rounds: state kept in scalar
  // registers takes a second vector register for spilled scalars, an address kept in a vector register takes that one,
  // and so do more than a handful of vector temporaries at the head of a round -- either way the drains then reload their
  // lane offset from scratch.  So a look loads a few words at a time, makes scalars of them at once (all lanes of the wave
  // read and write the same words with the same values) and computes on those.
  //   words 0, 1: hash bytes of the records the wave is through; 2, 3: those of the current record;
  //   4, 5: level_next(), the bytes into the record at which its progress moves next;
  //   6: the scale's shift | the progress published last << 8; 7: LDS address of its progress word.
  //   (The progress never passes 63 -- level_shift() puts the entry's last step there at most -- so it fits the byte and
  //   0xFF in it means "none yet".  The SIMD's four words are the 16 bytes around the wave's own: level_word() puts them
  //   side by side, and `level_lds` and every wave's state start at multiples of 16 bytes, as everything before them in
  //   the layout does: kCellOff, 4 F bytes of cells (launch_sketch gives this shape no sketch of fewer than 4 cells)
  //   and the stacks with their state.)
  static_assert(kCellOff % 16 == 0 && (8 * kStack + 4 * kLevelStateWords) % 16 == 0 && kLevelStateWords == 8 && kLevelWords == 16,
                "leveling: sixteen progress words and eight words of state per wave, all at multiples of 16 bytes");
  typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));
  typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
  typedef __attribute__((address_space(3))) u32x2_t lds_u32x2_t;
  typedef __attribute__((address_space(3))) u32x4_t lds_u32x4_t;
  auto lv_fence = [&]() { asm volatile("" ::: "memory"); };   // (keeps the loads of one group apart from the next one's)
  auto lv_pair = [&](uint32_t addr, uint64_t &x) {
    lv_fence();
    const u32x2_t v = *(lds_u32x2_t *)(uintptr_t)addr;
    x = (uint64_t)__builtin_amdgcn_readfirstlane(v.x) | ((uint64_t)__builtin_amdgcn_readfirstlane(v.y) << 32);
    lv_fence();
  };
  auto lv_quad = [&](uint32_t addr, uint32_t (&w)[4]) {
    lv_fence();
    const u32x4_t v = *(lds_u32x4_t *)(uintptr_t)addr;
    w[0] = __builtin_amdgcn_readfirstlane(v.x); w[1] = __builtin_amdgcn_readfirstlane(v.y);
    w[2] = __builtin_amdgcn_readfirstlane(v.z); w[3] = __builtin_amdgcn_readfirstlane(v.w);
    lv_fence();
  };
  auto lv_put = [&](uint32_t addr, uint64_t x) {
    u32x2_t v;
    v.x = (uint32_t)x; v.y = (uint32_t)(x >> 32);
    *(lds_u32x2_t *)(uintptr_t)addr = v;
  };
  auto lv_own = [&]() { return bottom + 8u * kStack; };
  lv_put(lv_own(), 0);
  lv_put(lv_own() + 24u, (uint64_t)(level_shift(n_entry) | 0xFF00u) | ((uint64_t)(level_lds + 4u * level_word(tid >> 6)) << 32));
  // the look at the head of round rd of the current record
  auto level = [&](uint32_t rd) {
    const uint64_t in = level_round_bytes(rd, BLOCK, a.splits);
    uint64_t next;
    lv_pair(lv_own() + 16u, next);
    if (in >= next) {   // (uniform)
      uint32_t q[4];
      uint64_t sw;
      lv_quad(lv_own(), q);
      lv_pair(lv_own() + 24u, sw);
      const uint64_t done = (uint64_t)q[0] | ((uint64_t)q[1] << 32), rec_n = (uint64_t)q[2] | ((uint64_t)q[3] << 32);
      const uint32_t shift = (uint32_t)sw & 0xFFu, last = ((uint32_t)sw >> 8) & 0xFFu, word = (uint32_t)(sw >> 32);
      const uint32_t p = level_progress(done, rec_n, rd, BLOCK, a.splits, shift);
      lv_put(lv_own() + 16u, level_next(done, rec_n, p, shift));
      if (p != last) {   // a step boundary of its own progress (a record's first round is looked at whatever it brings)
        lv_put(lv_own() + 24u, (uint64_t)(shift | (p << 8)) | ((uint64_t)word << 32));
        *(lds_u32_t *)(uintptr_t)word = p;
        uint32_t w[4];
        lv_quad(word & ~15u, w);
        const uint32_t pr = level_prio(p, w);
        if (pr == 0u) __builtin_amdgcn_s_setprio(0);   // (the instruction takes an immediate)
        else if (pr == 1u) __builtin_amdgcn_s_setprio(1);
        else if (pr == 2u) __builtin_amdgcn_s_setprio(2);
        else __builtin_amdgcn_s_setprio(3);
      }
    }
  };
  auto level_record = [&](uint64_t rec_n) { lv_put(lv_own() + 8u, rec_n); lv_put(lv_own() + 16u, 0); };
  auto level_record_done = [&]() {
    uint32_t q[4];
    lv_quad(lv_own(), q);
    lv_put(lv_own(), ((uint64_t)q[0] | ((uint64_t)q[1] << 32)) + ((uint64_t)q[2] | ((uint64_t)q[3] << 32)));
  };
  for (uint32_t rec = r0; rec < r1; ++rec) {
    const uint64_t b0 = a.rec_off[rec], b1 = a.rec_off[rec + 1];
    if (b1 - b0 <= d.K) continue;          // src/niqki_index.cpp:395,:450
    level_record(b1 - b0 - d.K);
    const LaneLines g = lane_lines(seqs_addr, b0, b1, d.K, a.splits, part, BLOCK,
                                   __builtin_amdgcn_readfirstlane(tid >> 6), lane);
    const uint32_t nl = g.n_lines;
    uint32_t nl_max = nl;
#pragma unroll
    for (int dd = 32; dd >= 1; dd >>= 1) {
      const uint32_t o = (uint32_t)__shfl_xor((int)nl_max, dd, 64);
      nl_max = o > nl_max ? o : nl_max;
    }
    nl_max = __builtin_amdgcn_readfirstlane(nl_max);
    if (nl_max == 0) { level_record_done(); continue; }   // (uniform) no line of this record for the wave
    const uint8_t *const base = a.seqs + b0;
    // ---- warm-up, once per lane and record (see roll_records; the 32 bytes come as two unaligned loads) ----
    uint64_t fw = 0, rc = 0;
    const bool wave_fast = __all(g.warm_fast != 0u || nl == 0u) != 0;   // (a lane without lines rolls the record's first bytes, for nothing)
    const uint8_t *const wp = gptr(warm_load(g, d.K, wave_fast));
    if (wave_fast) {
      uint64_t ew[32];
      {
        uint64_t e16[16];
        lut64_16(load16u(wp), lds0, e16);
#pragma unroll
        for (int j = 0; j < 16; ++j) ew[j] = e16[j];
        lut64_16(load16u(wp + 16), lds0, e16);
#pragma unroll
        for (int j = 0; j < 16; ++j) ew[16 + j] = e16[j];
      }
#pragma unroll
      for (int j = 0; j < 30; ++j) {
        fw = shl2_add64(fw, ew[j]);
        rc = shr2_64(rc | (ew[j] & 0xFFFFFFFF00000000ULL));
      }
    } else {
      // a lane of the fast form beside one that starts inside the prefix: its K - 1 bases are the last of its 30
      const uint8_t *const gp = wp;
      const uint64_t i0 = g.first_kmer;
      uint32_t ok = 1;
      if (reads_prefix(g, d.K)) {
        const uint4 p0 = load16u(base), p1 = load16u(base + 16);
#pragma unroll
        for (int j = 0; j < 32; ++j) {
          uint32_t w = dword_of(j < 16 ? p0 : p1, (j & 15) >> 2);
          uint32_t e = lut[(w >> (8 * (j & 3))) & 0xFFu];
          if ((uint32_t)j < Km1) ok &= (e >> 6) & 1u;
        }
      }
      const uint4 g0 = load16u(gp), g1 = load16u(gp + 16);
      uint32_t ew[32];
#pragma unroll
      for (int j = 0; j < 32; ++j) {
        uint32_t w = dword_of(j < 16 ? g0 : g1, (j & 15) >> 2);
        ew[j] = lut[(w >> (8 * (j & 3))) & 0xFFu];
      }
#pragma unroll
      for (int j = 0; j < 32; ++j) {
        if ((uint32_t)j < Km1) {
          const uint32_t e = ew[j];
          const bool pfx = i0 + (uint32_t)j < Km1;
          uint32_t dgt = ok ? ((e >> 4) & 3u) : 0u;
          uint32_t cf = pfx ? dgt : (e & 3u);
          uint32_t cr = pfx ? (3u - dgt) : ((e >> 2) & 3u);
          fw = (fw << 2) | cf;
          rc = (rc >> 2) | ((uint64_t)cr << rc_shift);
        }
      }
    }
    // ---- the rounds ----
    // The round's line: 32 registers that the pass loop indexes with its (uniform) counter -- one v_mov in
    // register-index mode per dword, so the loop's body stays 16 steps, not a line of 128.
    u32x32_t L;
    // whole: (uniform) every lane may load all of the line at `line`.  Otherwise every 16-byte piece is clamped to the
    // buffer and moved back to its place.
    auto load_line = [&](uint64_t line, bool whole) {
      if (whole) {
        const uint8_t *const p = gptr(line);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const uint4 v = *(const uint4 *)(p + 16 * q);
          L[4 * q] = v.x; L[4 * q + 1] = v.y; L[4 * q + 2] = v.z; L[4 * q + 3] = v.w;
        }
      } else {
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const uint64_t x = line + 16u * q, c = clamp_piece(x, buf_lo, buf_hi);
          uint4 v = load16u(gptr(c));
          if (c != x) v = replace16(v, (int)(int64_t)(c - x));
          L[4 * q] = v.x; L[4 * q + 1] = v.y; L[4 * q + 2] = v.z; L[4 * q + 3] = v.w;
        }
      }
    };
    auto is_whole = [&](uint64_t line, bool want) { return __all(want && line_inside(line, buf_lo, buf_hi)) != 0; };
    auto dword_at = [&](uint32_t i) { return L[__builtin_amdgcn_readfirstlane(i)]; };   // (i uniform)
    const uint64_t rec_addr = seqs_addr + b0;
    // the lane's hash bytes, counted from the start of its first line
    const uint32_t rel_lo = (uint32_t)(g.hash_lo - (g.line0 << kLineLog2)), rel_hi = (uint32_t)(g.hash_hi - (g.line0 << kLineLog2));
    {
      const uint64_t line = round_line(g, 0, rec_addr);
      load_line(line, is_whole(line, nl != 0u));
    }
    // the entries of the next eight steps: four are looked up (one dword of the line) as soon as four have been used up
    uint64_t e[8];
    lut64_4<0>(L[0], lds0, e);
    lut64_4<1>(L[1], lds0, e);
    auto step = [&](uint64_t ent, bool check) {
      // :225-229 and :233-236 with the entry's pre-placed codes (see roll_records)
      rc = shr2_64(rc | (ent & 0xFFFFFFFF00000000ULL));
      fw = shl2_add64(fw, ent) & fw_mask;
      uint64_t x1;
      const uint32_t hh = rev64_hi_mad_x1(min62(fw, rc), x1);   // :345
      push_candidates(hh, thr, x1, top);
      if (check && __builtin_expect(top >= bottom + 512u, 0)) {
        drain64();
        if (top >= bottom + 512u) drain64();
      }
    };
    // the same step for a lane whose hash bytes in the line are [wlo, wlo + wn): pos = the step's byte - wlo (wraps below
    // wlo).  The empty asm keeps the compare inside its step: sixteen lane masks computed ahead would take 32 scalar registers.
    auto step_pred = [&](uint64_t ent, uint32_t &pos, uint32_t wn, bool check) {
      asm volatile("" : "+v"(pos));
      const bool live = pos < wn;
      pos += 1u;
      const uint64_t rc2 = shr2_64(rc | (ent & 0xFFFFFFFF00000000ULL));
      const uint64_t fw2 = shl2_add64(fw, ent) & fw_mask;
      rc = live ? rc2 : rc;
      fw = live ? fw2 : fw;
      uint64_t x1;
      const uint32_t hh = rev64_hi_mad_x1(min62(fw, rc), x1);
      push_candidates(live ? hh : 0xFFFFFFFFu, thr, x1, top);
      if (check && __builtin_expect(top >= bottom + 512u, 0)) {
        drain64();
        if (top >= bottom + 512u) drain64();
      }
    };
    for (uint32_t rd = 0; rd < nl_max; ++rd) {
      level(rd);
      // the lane's hash bytes in this line: [wlo, wlo + wn)
      const uint32_t off = rd << kLineLog2;   // (a lane's run is far shorter than 4 GB)
      const uint32_t wlo = rel_lo > off ? rel_lo - off : 0u;
      const uint32_t whi = rel_hi > off ? (rel_hi - off < (uint32_t)kLineBytes ? rel_hi - off : (uint32_t)kLineBytes) : 0u;
      const uint32_t wn = rd < nl && whi > wlo ? whi - wlo : 0u;
      const bool plain = __all(wn == (uint32_t)kLineBytes) != 0;
      // the next round's line, requested in this line's last pass
      auto request_next = [&]() {
        if (rd + 1u < nl_max) {   // (uniform)
          const uint64_t line = round_line(g, rd + 1u, rec_addr);
          load_line(line, is_whole(line, rd + 1u < nl));
        }
      };
      // A pass of the loops below is 16 steps = four dwords of the line; the entries of dword n are looked up behind
      // the steps of dword n - 2.  The line's last pass looks up its last two dwords from copies and the next line's
      // first two from the registers that the next line is loaded into: the request goes out 12 steps before its first
      // bytes are needed, and with every byte of this line already looked up or copied.
#define NQ_LINE_PASS(STEP, D0, D1, D2, D3)                 \
  do {                                                     \
    _Pragma("unroll") for (int j = 0; j < 4; ++j) STEP(j); \
    lut64_4<0>(D0, lds0, e);                               \
    _Pragma("unroll") for (int j = 4; j < 8; ++j) STEP(j); \
    lut64_4<1>(D1, lds0, e);                               \
    _Pragma("unroll") for (int j = 0; j < 4; ++j) STEP(j); \
    lut64_4<0>(D2, lds0, e);                               \
    _Pragma("unroll") for (int j = 4; j < 8; ++j) STEP(j); \
    lut64_4<1>(D3, lds0, e);                               \
  } while (0)
      if (plain) {
#define NQ_STEP(J) step(e[J], ((J) & 1) != 0)
        for (uint32_t it = 0; it < 7u; ++it)
          NQ_LINE_PASS(NQ_STEP, dword_at(4u * it + 2u), dword_at(4u * it + 3u), dword_at(4u * it + 4u), dword_at(4u * it + 5u));
        const uint32_t t0 = L[30], t1 = L[31];
        request_next();
        NQ_LINE_PASS(NQ_STEP, t0, t1, L[0], L[1]);
#undef NQ_STEP
      } else {
        uint32_t pos = 0u - wlo;
#define NQ_STEP(J) step_pred(e[J], pos, wn, ((J) & 1) != 0)
        for (uint32_t it = 0; it < 7u; ++it)
          NQ_LINE_PASS(NQ_STEP, dword_at(4u * it + 2u), dword_at(4u * it + 3u), dword_at(4u * it + 4u), dword_at(4u * it + 5u));
        const uint32_t t0 = L[30], t1 = L[31];
        request_next();
        NQ_LINE_PASS(NQ_STEP, t0, t1, L[0], L[1]);
#undef NQ_STEP
      }
#undef NQ_LINE_PASS
    }
    level_record_done();
  }
  // out of the loop: the word no longer counts for the SIMD's least, and the drain and the barriers run at the kernel's own priority
  {
    uint64_t sw;
    lv_pair(lv_own() + 24u, sw);
    *(lds_u32_t *)(uintptr_t)(uint32_t)(sw >> 32) = kLevelDone;
  }
  __builtin_amdgcn_s_setprio(0);
  if (top != bottom) {   // fewer than 64 left
    const uint32_t n = (top - bottom) >> 3;
    const bool live = lane < n;
    const uint64_t c = live ? stack[lane] : 0ull;
    candidate_update(c, d, lds0, live);
  }
#ifdef NQ_SKETCH_CLOCK
  if (lane == 0 && blockIdx.x < kWaveTraceWgs) nq_sketch_wave[18 * blockIdx.x + 2 + (tid >> 6)] = wall_clock64();
#endif
}

// GROUPS 16-byte groups of hash steps per chunk: CHUNK = 16*GROUPS k-mers.
#ifdef NQ_SKETCH_CLOCK
__device__ unsigned long long nq_sketch_clk[2];   // shader cycles / 100 MHz ticks spent by one workgroup (tools/ubench_sketch.hip)
__device__ unsigned long long nq_sketch_trace[3 * 8192];   // per workgroup: start, end (100 MHz ticks), hardware id
#endif

template <int BLOCK, int GROUPS, int KFIX>
__global__ __launch_bounds__(BLOCK) void sketch_kernel(SketchArgs a) {
  extern __shared__ __align__(16) uint32_t smem[];
#ifdef NQ_SKETCH_CLOCK
  const unsigned long long clk_c0 = __builtin_readcyclecounter(), clk_r0 = wall_clock64();
#endif
  const Derived &d = a.d;
  const uint32_t Fc = d.F / a.halves;               // cells this workgroup keeps
  uint2 *lut64 = (uint2 *)(smem + kLut64Off / 4);   // 256 x {forward code, rc code << 30} (K = 31 filtered path)
  uint8_t *lut = (uint8_t *)(smem + kLutOff / 4);   // 256 bytes
  uint32_t *s_flag = smem + kFlagOff / 4;           // 4 words
  uint32_t *sk = smem + kCellOff / 4;               // Fc cells
  uint32_t *aux = sk + Fc;                          // distinct-value tables or the candidate stacks
  const uint32_t lds0 = (uint32_t)(uintptr_t)(lds_u32_t *)smem;   // LDS address of the layout's start
  const uint32_t tid = threadIdx.x;
  const uint32_t part = blockIdx.x % a.splits;
  const uint32_t half = (blockIdx.x / a.splits) % a.halves;
  const uint32_t entry = blockIdx.x / (a.splits * a.halves);
  const uint32_t hsel = a.halves > 1 ? half + 1u : 0u;
  if (a.redo_only && a.redo[entry] != a.redo_only) return;   // (uniform) not this launch's sketch

  for (uint32_t i = tid; i < 256; i += BLOCK) {
    const uint32_t e = code_entry(i);
    lut[i] = (uint8_t)e;
    // rc code at bit 2K of the reverse word BEFORE its shift = bit 2K - 32 of the entry's high word (K >= 17;
    // else unused); added into the forward word it sits above the k-mer mask
    lut64[i] = make_uint2(e & 3u, d.K >= kFastKMin ? ((e >> 2) & 3u) << (2u * d.K - 32u) : 0u);
  }
  // the leveling words of the line form, behind the candidate stacks (only a filtered launch of that shape has them)
  if (BLOCK == 1024 && GROUPS == 32 && a.filter && tid < kLevelWords) aux[(2 * kStack + kLevelStateWords) * (BLOCK / 64) + tid] = 0;
  if (a.accumulate) {
    const uint32_t *src = (const uint32_t *)a.sketches + (uint64_t)entry * d.F + (uint64_t)half * Fc;
    for (uint32_t i = tid; i < Fc; i += BLOCK) sk[i] = src[i];
  } else {
    for (uint32_t i = tid; i < Fc; i += BLOCK) sk[i] = kEmpty32;
  }
  __syncthreads();

  if (a.seqs != nullptr) {  // nullptr = densify-only launch
    // Filter strength from the k-mers per slot: expected undecided slots
    // F*(1-2^-T)^(n/F) must be negligible (a miss only costs the exact re-run below).
    uint32_t thr = 0;
    uint64_t n = 0;   // the entry's k-mers = its hash bytes
    if (a.filter) {
      const uint32_t r0 = a.entry_rec ? a.entry_rec[entry] : entry;
      const uint32_t r1 = a.entry_rec ? a.entry_rec[entry + 1] : entry + 1;
      for (uint32_t rec = r0; rec < r1; ++rec) {
        const uint64_t len = a.rec_off[rec + 1] - a.rec_off[rec];
        if (len > d.K) n += len - d.K;
      }
      // every part of a split record must be exact on its own share
      const uint64_t per_slot = (n / a.splits) >> d.S;
      uint32_t T = per_slot >= 240 ? 4u : per_slot >= 115 ? 3u : per_slot >= 55 ? 2u : 0u;
      if (a.filter >= 2) T = a.filter - 1;  // forced strength (tests)
      // the ordering argument needs a non-saturated HyperLogLog part: 2^H - 1 >= T
      if (T > d.max_rem || T > 16) T = 0;
      thr = T ? (1u << (32 - T)) : 0u;
    }
    thr = __builtin_amdgcn_readfirstlane(thr);
    if (thr) {
      // the generic filtered form also serves a layout that does not start at LDS address 0
      if (hsel || lds0 != 0) roll_records<BLOCK, GROUPS, KFIX, true, false>(a, entry, part, sk, lut, (uint64_t *)aux, thr, hsel);
      // the longest records' shape: whole lines per lane
      else if (GROUPS == 32 && (KFIX == 31 || (d.K >= kFastKMin && d.K <= kLineFastKMax))) {
#ifdef NQ_SKETCH_CLOCK
        if (tid == 0 && blockIdx.x < kWaveTraceWgs) nq_sketch_wave[18 * blockIdx.x] = wall_clock64();
#endif
        roll_records_lines<BLOCK, KFIX>(a, entry, part, lut, (uint64_t *)aux, thr, n,
                                         kCellOff + 4u * d.F + (8u * kStack + 4u * kLevelStateWords) * (BLOCK / 64));   // (halves = 1 here: Fc = F, a kernel argument)
      }
      else roll_records<BLOCK, GROUPS, KFIX, true, true>(a, entry, part, sk, lut, (uint64_t *)aux, thr, 0);
      __syncthreads();
#ifdef NQ_SKETCH_CLOCK
      if (tid == 0 && blockIdx.x < kWaveTraceWgs) nq_sketch_wave[18 * blockIdx.x + 1] = wall_clock64();
#endif
      uint32_t local = 0;
      for (uint32_t i = tid; i < Fc; i += BLOCK) local += (sk[i] == kEmpty32);
      if (tid == 0) s_flag[2] = 0;
      __syncthreads();
      if (local) atomicAdd(&s_flag[2], local);
      __syncthreads();
      // a slot without a candidate may still have skipped k-mers: exact re-run.
      // (With splits > 1 another part may hold the candidates, so every part re-runs.)
      if (s_flag[2] != 0) roll_records<BLOCK, GROUPS, KFIX, false, false>(a, entry, part, sk, lut, nullptr, 0, hsel);
    } else {
      roll_records<BLOCK, GROUPS, KFIX, false, false>(a, entry, part, sk, lut, nullptr, 0, hsel);
    }
  }
  __syncthreads();

  uint32_t *out = (uint32_t *)a.sketches + (uint64_t)entry * d.F + (uint64_t)half * Fc;
  if (a.splits > 1 || a.halves > 1) {
    // partial sketch (a part of a split record, or one half of the slots): merged in global
    // memory, densified by a second launch once all workgroups are in
    for (uint32_t i = tid; i < Fc; i += BLOCK) {
      uint32_t v = sk[i];
      if (v != kEmpty32) atomicMin(&out[i], v);
    }
    return;
  }
  if (a.densify) {
    if (a.distinct) densify_lds_distinct<BLOCK>(sk, d, s_flag, aux);
    else densify_lds<BLOCK>(sk, d, s_flag);
  }
  __syncthreads();
  for (uint32_t i = tid; i < d.F; i += BLOCK) out[i] = sk[i];
#ifdef NQ_SKETCH_CLOCK
  if (blockIdx.x == gridDim.x / 2 && tid == 0) {
    nq_sketch_clk[0] = __builtin_readcyclecounter() - clk_c0;
    nq_sketch_clk[1] = wall_clock64() - clk_r0;
  }
  if (tid == 0 && blockIdx.x < 8192) {
    uint32_t hw, xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    nq_sketch_trace[3 * blockIdx.x] = clk_r0;
    nq_sketch_trace[3 * blockIdx.x + 1] = wall_clock64();
    nq_sketch_trace[3 * blockIdx.x + 2] = ((unsigned long long)xcc << 32) | hw;
  }
#endif
}

// NIQKI_SKETCH_WAVE=0 switches the one-wavefront kernel off; NIQKI_SKETCH_FILTER: 0 = off, unset/1 = automatic,
// n >= 2 = force n-1 leading zeros (tests)
SketchSwitches sketch_switches() {
  const char *wv = std::getenv("NIQKI_SKETCH_WAVE"), *fv = std::getenv("NIQKI_SKETCH_FILTER");
  return SketchSwitches{!(wv && std::atoi(wv) == 0), fv ? (uint32_t)std::atoi(fv) : 1u};
}

hipError_t launch_sketch(const SketchArgs &a_in, uint32_t n_entry, const SketchPlan &p, hipStream_t stream) {
  if (n_entry == 0) return hipSuccess;
  if (p.shape == kShapeRefused) return hipErrorInvalidValue;
  SketchArgs a = a_in;
  a.halves = p.halves;
  a.distinct = p.distinct;
  a.filter = p.filter;
  a.read_entries = p.read_entries;
  if (p.late_distinct) a.densify = 0;   // the kernel stores the cells as they are
  if (p.shape == kShapeDensifyGlobal) return launch_densify_global(a, n_entry, stream);
  if (p.shape == kShapeWave) return launch_sketch_reads(a, n_entry, p.lds_bytes, stream);
  const size_t lds = p.lds_bytes;
  dim3 grid(n_entry * a.splits * a.halves);
#define NQ_LAUNCH_SKETCH(B, G, KF)                                                              \
  do {                                                                                           \
    auto k = sketch_kernel<B, G, KF>;                                                            \
    hipError_t e = hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
    if (e != hipSuccess) return e;                                                               \
    hipLaunchKernelGGL(k, grid, dim3(B), lds, stream, a);                                        \
  } while (0)
  if (p.shape == kShape256x1) {
    if (a.d.K == 31) NQ_LAUNCH_SKETCH(256, 1, 31); else NQ_LAUNCH_SKETCH(256, 1, 0);
  } else if (p.shape == kShape1024x2) {
    if (a.d.K == 31) NQ_LAUNCH_SKETCH(1024, 2, 31); else NQ_LAUNCH_SKETCH(1024, 2, 0);
  } else if (p.shape == kShape1024x8) {
    if (a.d.K == 31) NQ_LAUNCH_SKETCH(1024, 8, 31); else NQ_LAUNCH_SKETCH(1024, 8, 0);
  } else {
    if (a.d.K == 31) NQ_LAUNCH_SKETCH(1024, 32, 31); else NQ_LAUNCH_SKETCH(1024, 32, 0);
  }
#undef NQ_LAUNCH_SKETCH
  if (p.late_distinct) return launch_densify_distinct(a, n_entry, sketch_late_lds_bytes(a.d), stream);
  return hipGetLastError();
}

__global__ void fill_u32_kernel(uint32_t *p, uint64_t n, uint32_t v) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) p[i] = v;
}

hipError_t launch_fill_u32(uint32_t *p, uint64_t n, uint32_t v, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  uint64_t blocks = (n + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(fill_u32_kernel, dim3((uint32_t)blocks), dim3(256), 0, stream, p, n, v);
  return hipGetLastError();
}

}  // namespace nq
