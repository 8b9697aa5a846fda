// nq_lookup.hip -- the slot-major look-up pre-pass of a query launch, for gfx950: lookup_kernel, lookup_rows_kernel and
// pack_entries_kernel, which makes the packed copy of the table that the second one streams.  Which of them a launch takes
// is the plan's to say (nq_gather_plan.h: lookup_form); launch_lookup carries it out.
#include "nq_gather_ops.h"

#include <algorithm>

namespace nq {

// ---- slot-major look-up pre-pass ---------------------------------------------------------
// In gather_kernel's own look-up every (query, slot) costs one random 128-byte table line of
// which 8 * n_tiles bytes are used: 4.2 MB of a 14 MB query at the north-star shape.  For a real
// batch the table is better walked slot block by slot block for all queries of the launch:
//   lookup_kernel  one workgroup = PS consecutive slots x 256 queries (one per thread).  A thread
//                  reads its query's PS fingerprints (one whole 128-byte line of the sketch for
//                  PS = 32), looks each one up with one 8 * n_tiles byte load, 8 slots in flight
//                  at a time, packs the results and stores, per tile, PS words = one whole line
//                  of pre[q][t][s].
// All workgroups of one slot block (nq / 256 of them) are neighbours in one XCD's dispatch order
// (block ids x, x+8, ...): they run at the same time on that XCD and walk the block's rows in
// the same order, so a table line is fetched from HBM once and served from the XCD's L2 to the
// other queries that need it (4096 queries into 512 lines per slot).
// Packed word: (bucket start - first unit of its slot) << 16 | length; launch_lookup_usable()
// says whether both halves fit 16 bits for the index at hand.
// HBM traffic per launch: the table once + 4 bytes per (query, slot) in and 4 * n_tiles out,
// instead of 128 bytes per (query, slot).
constexpr uint32_t kPreFlight = 8;       // look-ups in flight per thread (kXcds, kPreBlock: nq_gather_plan.h)

// NT tiles from tile t0 on per launch: an index of more than 4 tiles takes several launches.
template <int NT, int PS>
__global__ __launch_bounds__(kPreBlock) void lookup_kernel(IndexView v, const int32_t *sketches, uint32_t nq,
                                                           uint32_t n_qchunk, uint32_t *pre, uint32_t t0) {
  const uint32_t tid = threadIdx.x;
  const uint32_t n_sb = v.f_local / PS;
  const uint32_t x = blockIdx.x % kXcds, k = blockIdx.x / kXcds;
  const uint32_t sb = (k / n_qchunk) * kXcds + x;
  if (sb >= n_sb) return;   // padding block (uniform)
  const uint32_t q = (k % n_qchunk) * kPreBlock + tid;
  if (q >= nq) return;      // no barrier below
  const uint32_t R = v.d.R;
  // this thread's fingerprints (src/niqki_index.cpp:654: anything outside [0, R) has no bucket)
  int32_t fp[PS];
  {
    const int4 *src = (const int4 *)(sketches + (uint64_t)q * v.q_stride + v.q_off + (uint64_t)sb * PS);
#pragma unroll
    for (int u = 0; u < PS / 4; ++u) {
      const int4 a = src[u];
      fp[4 * u] = a.x; fp[4 * u + 1] = a.y; fp[4 * u + 2] = a.z; fp[4 * u + 3] = a.w;
    }
  }
  uint32_t res[NT][PS];
#pragma unroll
  for (int i0 = 0; i0 < PS; i0 += kPreFlight) {
    Entry en[kPreFlight][NT];
#pragma unroll
    for (int j = 0; j < (int)kPreFlight; ++j) {   // all loads of the group first
      const int i = i0 + j;
      const bool ok = fp[i] >= 0 && (uint32_t)fp[i] < R;
      const Entry *e = v.entries + ((uint64_t)(sb * PS + i) * R + (ok ? (uint32_t)fp[i] : 0u)) * v.n_tiles + t0;
#pragma unroll
      for (int t = 0; t < NT; ++t) en[j][t] = e[t];
    }
#pragma unroll
    for (int j = 0; j < (int)kPreFlight; ++j) {
      const int i = i0 + j;
      const bool ok = fp[i] >= 0 && (uint32_t)fp[i] < R;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const uint32_t base = v.slot_units[(uint64_t)(t0 + t) * (v.f_local + 1) + sb * PS + i];
        res[t][i] = ok ? (((en[j][t].start - base) << 16) | en[j][t].len) : 0u;
      }
    }
  }
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    uint4 *dst = (uint4 *)(pre + ((uint64_t)q * v.n_tiles + t0 + t) * v.f_local + (uint64_t)sb * PS);
#pragma unroll
    for (int u = 0; u < PS / 4; ++u) dst[u] = make_uint4(res[t][4 * u], res[t][4 * u + 1], res[t][4 * u + 2], res[t][4 * u + 3]);
  }
}

// The same pre-pass with the table rows staged in LDS (1 or 2 tiles, R * tiles * 4 = 16 or 32 KB),
// from the PACKED copy of the table (IndexView::ptab: the 4-byte word of every entry): one workgroup
// = 32 consecutive slots x 1024 queries (one per thread).  Slot by slot the 1024 threads copy the
// slot's whole row (coalesced 16-byte loads straight into LDS: the table is streamed, not hit at
// random), three rows ahead, and every thread picks its query's word(s) with one LDS read.  At the end the 32 words per (query, tile) go through LDS once more so that
// eight neighbouring lanes store one 128-byte line of pre[q][t][s] together.  The workgroups of one
// slot block (nq / 1024) are neighbours in one XCD's dispatch order: the row comes from HBM once.
// (kRowSlots, kRowBlock: nq_gather_plan.h; the packed table's layout: packed_table_offset, nq_gather_ops.h)
// NT tiles from tile t0 on per launch (a tile GROUP: the packed table keeps the rows of a group together, see
// packed_table_offset): an index of more than 2 tiles takes ceil(n_tiles / 2) launches, each streaming its group's
// part of the table once.
template <int NT, int PER>   // PER: 16-byte pieces of a packed row per thread (R * NT / 4096)
__global__ __launch_bounds__(kRowBlock) void lookup_rows_kernel(IndexView v, const int32_t *sketches, uint32_t nq,
                                                                uint32_t n_qchunk, uint32_t *pre, uint32_t t0) {
  extern __shared__ __align__(16) uint32_t rows[];   // 4 buffers of R * NT words; at the end 1024 x 17 words
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  const uint32_t n_sb = v.f_local / kRowSlots;
  const uint32_t x = blockIdx.x % kXcds, k = blockIdx.x / kXcds;
  const uint32_t sb = (k / n_qchunk) * kXcds + x;
  if (sb >= n_sb) return;   // padding block (uniform)
  const uint32_t q0 = (k % n_qchunk) * kRowBlock, q = q0 + tid;
  const bool live = q < nq;   // the others still help to stage the rows
  const uint32_t R = v.d.R, RW = R * NT;
  int32_t fp[kRowSlots];
  {
    const int4 *src = (const int4 *)(sketches + (uint64_t)(live ? q : 0u) * v.q_stride + v.q_off + (uint64_t)sb * kRowSlots);
#pragma unroll
    for (int u = 0; u < (int)kRowSlots / 4; ++u) {
      const int4 a = src[u];
      fp[4 * u] = a.x; fp[4 * u + 1] = a.y; fp[4 * u + 2] = a.z; fp[4 * u + 3] = a.w;
    }
  }
  // Rows travel memory -> LDS directly (global_load_lds_dwordx4: a wave's 64 lanes fill 1 KB of LDS from
  // the wave-uniform base on, no registers, no ds_write).  The compiler would wait for ALL such loads in
  // flight before any LDS read it can see, so the pipeline's waits and the look-up read are written by
  // hand: loads of one kind retire in issue order (vmcnt), and a wave passes the row's barrier only when
  // its own pieces of that row have landed.
  const uint4 *row0 = (const uint4 *)(v.ptab + packed_table_offset(v, t0) + (uint64_t)sb * kRowSlots * RW) + tid;
  const uint32_t row_u4 = RW / 4;   // 16-byte pieces per row
  const uint32_t wbase = tid & ~63u;
  auto request = [&](int i) {
    uint32_t *dst = rows + (uint32_t)(i & 3) * RW;
#pragma unroll
    for (int j = 0; j < PER; ++j)
      __builtin_amdgcn_global_load_lds((glb_cvoid *)(row0 + (uint64_t)i * row_u4 + (uint32_t)j * kRowBlock),
                                       (lds_void *)(dst + ((uint32_t)j * kRowBlock + wbase) * 4u), 16, 0, 0);
  };
  const uint32_t lds0 = (uint32_t)(uintptr_t)(lds_void *)rows;   // LDS byte address of the row buffers
  uint32_t res[NT][kRowSlots];
  request(0);
  request(1);
  request(2);
  // step I: own pieces of row I landed (only the 2 newer rows' loads may be outstanding) -> barrier: the
  // whole row is in LDS and everybody is done with row I - 1, whose buffer row I + 3 may now overwrite
#define NQ_ROW_STEP(I)                                                                                \
  {                                                                                                   \
    if ((I) + 2 < (int)kRowSlots) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * PER) : "memory");      \
    else if ((I) + 1 < (int)kRowSlots) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PER) : "memory");     \
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                             \
    lds_barrier();                                                                                    \
    if ((I) + 3 < (int)kRowSlots) request((I) + 3);                                                   \
    const bool ok = fp[(I)] >= 0 && (uint32_t)fp[(I)] < R; /* src/niqki_index.cpp:654 */              \
    const uint32_t at = lds0 + ((uint32_t)((I) & 3) * RW + (ok ? (uint32_t)fp[(I)] : 0u) * NT) * 4u;   \
    uint32_t w0, w1 = 0;                                                                              \
    if (NT == 2) {                                                                                    \
      uint2 w;                                                                                        \
      asm volatile("ds_read_b64 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(w) : "v"(at) : "memory");      \
      w0 = w.x; w1 = w.y;                                                                             \
    } else {                                                                                          \
      asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(w0) : "v"(at) : "memory");     \
    }                                                                                                 \
    res[0][(I)] = ok ? w0 : 0u;                                                                       \
    res[NT - 1][(I)] = ok ? (NT == 2 ? w1 : w0) : 0u;                                                 \
  }
#define NQ_ROW_STEP8(B) NQ_ROW_STEP((B)) NQ_ROW_STEP((B) + 1) NQ_ROW_STEP((B) + 2) NQ_ROW_STEP((B) + 3) \
                        NQ_ROW_STEP((B) + 4) NQ_ROW_STEP((B) + 5) NQ_ROW_STEP((B) + 6) NQ_ROW_STEP((B) + 7)
  NQ_ROW_STEP8(0) NQ_ROW_STEP8(8) NQ_ROW_STEP8(16) NQ_ROW_STEP8(24)
#undef NQ_ROW_STEP8
#undef NQ_ROW_STEP
  static_assert(kRowSlots == 32, "the steps above are written out");
  // Out: thread q holds 32 words per tile = one 128-byte line of pre[q][t][s]; lanes 8j .. 8j + 7 of a
  // wave store the eight 16-byte pieces of query (wave base + 8 r + j)'s line, r = 0 .. 7, so one store
  // instruction writes 8 whole lines.  The transposition goes through LDS (33-word rows: no bank conflicts).
  lds_barrier();   // all look-ups of the last row are done: the row buffers are free
  uint32_t *mine = rows + tid * (kRowSlots + 1u);
#define NQ_STORE_TILE(T)                                                                                             \
  {                                                                                                                  \
    _Pragma("unroll") for (int i = 0; i < (int)kRowSlots; ++i) mine[i] = res[(T)][i];                               \
    wave_lds_fence(); /* (one wave reads what its own lanes wrote) */                                                \
    _Pragma("unroll") for (int r = 0; r < 8; ++r) {                                                                  \
      const uint32_t src_t = (tid & ~63u) + 8u * (uint32_t)r + (lane >> 3); /* whose line this lane helps to store */ \
      const uint32_t piece = lane & 7u;                                                                              \
      const uint32_t *sp = rows + src_t * (kRowSlots + 1u) + piece * 4u;                                             \
      const uint4 w = make_uint4(sp[0], sp[1], sp[2], sp[3]);                                                        \
      const uint32_t qq = q0 + src_t;                                                                                \
      if (qq < nq) *(uint4 *)(pre + ((uint64_t)qq * v.n_tiles + t0 + (T)) * v.f_local + (uint64_t)sb * kRowSlots + piece * 4u) = w; \
    }                                                                                                                \
    wave_lds_fence(); /* before the next tile overwrites the wave's words */                                         \
  }
  NQ_STORE_TILE(0)
  if (NT == 2) NQ_STORE_TILE(NT - 1)
#undef NQ_STORE_TILE
}

__global__ __launch_bounds__(256) void pack_entries_kernel(IndexView v, uint32_t *ptab) {
  const uint64_t n = (uint64_t)v.f_local * v.d.R * v.n_tiles, step = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
    const uint32_t t = (uint32_t)(i % v.n_tiles);
    const uint64_t sf = i / v.n_tiles;   // slot * R + fp
    const uint32_t s = (uint32_t)(sf / v.d.R);
    const Entry e = v.entries[i];
    const uint32_t t0 = t & ~1u, nt = v.n_tiles - t0 >= 2 ? 2u : 1u;   // the tile's group
    ptab[packed_table_offset(v, t0) + sf * nt + (t - t0)] = ((e.start - v.slot_units[(uint64_t)t * (v.f_local + 1) + s]) << 16) | e.len;
  }
}
hipError_t launch_pack_entries(const IndexView &v, uint32_t *ptab, hipStream_t stream) {
  const uint64_t n = (uint64_t)v.f_local * v.d.R * v.n_tiles;
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(pack_entries_kernel, dim3((uint32_t)std::min<uint64_t>((n + 255) / 256, 65536)), dim3(256), 0, stream, v, ptab);
  return hipGetLastError();
}

namespace {
struct LookupArgs {
  const IndexView &v;
  const int32_t *sketches;
  uint32_t nq, n_qchunk, grid;
  uint32_t *pre;
  hipStream_t stream;
};
template <int NT, int PER>
hipError_t launch_rows(const LookupArgs &a, uint32_t t0) {
  static_assert(lookup_launch_exists(true, kRowSlots, NT, PER), "nq_gather_plan.h lists the instantiations");
  const size_t lds = std::max<size_t>((size_t)a.v.d.R * NT * 4 * 4, (size_t)kRowBlock * (kRowSlots + 1) * 4);
  const hipError_t e = hipFuncSetAttribute((const void *)lookup_rows_kernel<NT, PER>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((lookup_rows_kernel<NT, PER>), dim3(a.grid), dim3(kRowBlock), lds, a.stream, a.v, a.sketches, a.nq, a.n_qchunk, a.pre, t0);
  return hipSuccess;
}
template <int NT, int PS>
hipError_t launch_random(const LookupArgs &a, uint32_t t0) {
  static_assert(lookup_launch_exists(false, PS, NT, 0), "nq_gather_plan.h lists the instantiations");
  hipLaunchKernelGGL((lookup_kernel<NT, PS>), dim3(a.grid), dim3(kPreBlock), 0, a.stream, a.v, a.sketches, a.nq, a.n_qchunk, a.pre, t0);
  return hipSuccess;
}
// one kernel launch of the form: the tiles from t0 on
hipError_t launch_tiles(const LookupForm &f, const LookupArgs &a, uint32_t t0) {
  const LookupLaunch l = lookup_launch(f, a.v.n_tiles, a.v.d.R, t0);
  if (!lookup_launch_exists(f.rows, f.slots, l.nt, l.per)) return hipErrorInvalidValue;
  if (f.rows) return l.nt == 1 ? (l.per == 1 ? launch_rows<1, 1>(a, t0) : launch_rows<1, 2>(a, t0))
                               : (l.per == 1 ? launch_rows<2, 1>(a, t0) : launch_rows<2, 2>(a, t0));
  if (f.slots == 32) return l.nt == 1 ? launch_random<1, 32>(a, t0) : launch_random<2, 32>(a, t0);
  switch (l.nt) {   // (blocks of 16 slots whenever there are more than 2 tiles)
    case 1: return launch_random<1, 16>(a, t0);
    case 2: return launch_random<2, 16>(a, t0);
    case 3: return launch_random<3, 16>(a, t0);
    default: return launch_random<4, 16>(a, t0);
  }
}
}  // namespace

hipError_t launch_lookup(const IndexView &v, const int32_t *sketches, uint32_t nq, uint32_t *pre, const LookupForm &form,
                         hipStream_t stream) {
  if (nq == 0 || !launch_lookup_usable(gather_facts(v)) || (form.rows && !v.ptab)) return hipErrorInvalidValue;
  const uint32_t block = form.rows ? kRowBlock : kPreBlock;
  const uint32_t n_sb = v.f_local / form.slots, n_qchunk = (nq + block - 1) / block;
  const uint64_t grid = (uint64_t)((n_sb + kXcds - 1) / kXcds * kXcds) * n_qchunk;
  if (grid > 0x7FFFFFFFull) return hipErrorInvalidValue;
  const LookupArgs a{v, sketches, nq, n_qchunk, (uint32_t)grid, pre, stream};
  for (uint32_t t0 = 0; t0 < v.n_tiles; t0 += form.step) {   // tile groups (rows: those of packed_table_offset)
    const hipError_t e = launch_tiles(form, a, t0);
    if (e != hipSuccess) return e;
  }
  return hipGetLastError();
}

}  // namespace nq
