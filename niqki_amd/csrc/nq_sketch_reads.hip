// nq_sketch_reads.hip -- short records: one wavefront per sketch (sketch_reads_kernel), k-mers and densification.
// launch_sketch (nq_sketch.hip) takes it where the plan says kShapeWave (nq_sketch_plan.h).
//
// A 150-base read holds ~120 k-mers but its densification takes ~350 passes
// (SURVEY.md 8a a8), so the short-record kernel is built around the passes: one wave
// owns one sketch, nothing is synchronised across waves, and a pass costs one LDS round
// trip.  Each occupied cell of the sketch becomes an ENTRY held in registers
// (up to kReadEntries per lane): T = running low word of hash_family(v, step) (the target
// is T mod F and T += B per pass, B = low word of revhash64(v), src/niqki_index.cpp:308-310),
// mi = smallest cell index known to hold v.  A pass: every entry proposes
// 2^31 | mi to its target cell with an LDS min (occupied cells hold values below 2^31
// and stay as they are, the smallest source index wins = the first writer of the
// reference's ascending loop, :313-331); then every entry reads its target back, and the
// one that finds its own proposal writes the value and lowers its mi.  Copies of a value
// propose the same target, so the entries present at the start are all that ever
// matter; two entries with the same value are harmless (the lower index always wins).
#include "nq_kernels.h"
#include "nq_sketch_ops.h"

namespace nq {

// plain pass over all cells (more occupied cells than register entries: long records,
// few passes)
__device__ void densify_wave_cells(uint32_t *sk, const Derived &d, uint32_t empty) {
  const uint32_t F = d.F, lane = threadIdx.x;
  uint32_t step = 0, idle = 0;
  for (;;) {
    for (uint32_t i = lane; i < F; i += 64) {
      const uint32_t v = sk[i];
      if (v < 0x80000000u) {
        const uint32_t t = ((uint32_t)unrev64(v) + step * (uint32_t)rev64(v)) & (F - 1u);
        atomicMin(&sk[t], 0x80000000u | i);
      }
    }
    __syncthreads();
    uint32_t filled = 0;
    for (uint32_t i = lane; i < F; i += 64) {
      const uint32_t v = sk[i];
      if (v >= 0x80000000u && v != kEmpty32) { sk[i] = sk[v & 0x7FFFFFFFu]; ++filled; }
    }
    __syncthreads();
    uint32_t tot = filled;
#pragma unroll
    for (int dd = 32; dd >= 1; dd >>= 1) tot += __shfl_xor(tot, dd, 64);
    empty -= tot;
    ++step;
    idle = tot ? 0u : idle + 1u;
    if (empty == 0 || idle >= F) break;
  }
}

// all LDS traffic of the wave issued so far has completed, and the compiler keeps the
// accesses on either side apart (one wave: the LDS serves its instructions in order)
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_wave_barrier();
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}

// Sum of a per-lane count over the wave (the usual DPP ladder: shifts inside the rows of 16 lanes, then the rows' last
// lanes broadcast onward; lane 63 ends up with the total).  No LDS instruction, unlike a __shfl reduction.
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true);    // row_shr:1
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true);    // row_shr:2
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xe, true);    // row_shr:4, lanes 4..15 of a row
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xc, true);    // row_shr:8, lanes 8..15 of a row
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);   // row_bcast:15 into rows 1 and 3
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);   // row_bcast:31 into rows 2 and 3
  return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

// Minimum of a per-lane word over the wave (the same DPP ladder as wave_sum_u32; lanes the ladder leaves out bring
// the identity 2^32 - 1).
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
#define NQ_DPP_MIN(CTRL, ROWS, BANKS)                                                                      \
  {                                                                                                        \
    const uint32_t o = (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v, CTRL, ROWS, BANKS, false);        \
    v = o < v ? o : v;                                                                                     \
  }
  NQ_DPP_MIN(0x111, 0xf, 0xf)   // row_shr:1
  NQ_DPP_MIN(0x112, 0xf, 0xf)   // row_shr:2
  NQ_DPP_MIN(0x114, 0xf, 0xe)   // row_shr:4, lanes 4..15 of a row
  NQ_DPP_MIN(0x118, 0xf, 0xc)   // row_shr:8, lanes 8..15 of a row
  NQ_DPP_MIN(0x142, 0xa, 0xf)   // row_bcast:15 into rows 1 and 3
  NQ_DPP_MIN(0x143, 0xc, 0xf)   // row_bcast:31 into rows 2 and 3
#undef NQ_DPP_MIN
  return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

// ---- the last cells of a short record's densification in closed form --------------------------------------------
// Going from E empty cells to E - 1 takes F / (n E) passes (coupon collector; more where only few orbits reach a cell),
// so more than half of a 150-base read's ~420 passes fill its last 16 cells, and a pass costs its LDS instructions
// whatever it fills.  Once at most kTailCells cells are empty the passes stop.  An entry's target is affine in the
// pass (src/niqki_index.cpp:308-310): T_k + s B_k = c (mod F) with B_k = 2^j odd has the solution
//     s_k(c) = ((c - T_k) >> j) odd^-1  mod (F >> j)      if 2^j divides c - T_k, none otherwise
// (odd^-1 by Newton steps, once per entry).  Cell c is filled in pass s* = min_k s_k(c) by the entry that reaches it
// then -- among several, by the one whose value sits at the smallest cell index at the start of that pass (:313-331:
// the first writer of the ascending loop).  The lanes keep their entries; the cells are taken one after another:
// every lane solves for its own entries, one wave-wide minimum of (s << 15 | index at the start of the tail) names
// pass and winner.  An index can still drop during the tail (an entry wins a cell below its own), which matters only
// to a cell that several entries reach in its pass s*, and only if one of the LOSING ones has won some cell in an
// earlier pass of the tail: that case (a few reads in a hundred) is detected and handed back to the passes, which
// are exact for anything -- nothing is written before the check.  Cells no orbit reaches stay empty, as after the F
// fruitless passes that end the loop (documented divergences).  Pinned by tests/test_gpu_densify_designed.py
// (designed cells: every instantiation with and without ties, hand-backs the closed form would get wrong, unreachable
// cells), the goldens, tests/test_gpu_fuzz.py, tests/test_gpu_reads_config.py.
constexpr uint32_t kTailCells = 16;   // (8 .. 24 measure the same; 48: 3 % slower)

// T: every entry's target of the NEXT pass, B its stride, mk = 2^31 | the smallest index that holds its value, V its
// value (lanes without an entry: an occupied cell as T, B = 0 -- they reach no empty cell).  scratch: 2 x 64 words.
// true: every reachable empty cell is filled; false: nothing was touched, the passes go on.
template <int R>
__device__ __forceinline__ bool densify_tail(uint32_t *sk, uint32_t *scratch, uint32_t F, const uint32_t (&T)[R],
                                             const uint32_t (&B)[R], const uint32_t (&mk)[R], const uint32_t (&V)[R]) {
  const uint32_t lane = threadIdx.x, Fm = F - 1u;
  uint32_t *list = scratch, *vals = scratch + 64;
  // ---- the empty cells (F is a multiple of 256 on this path) ----
  uint32_t n_e = 0;
  vals[lane] = kEmpty32;
  for (uint32_t c0 = 0; c0 < F; c0 += 256) {
    const uint4 v = *(const uint4 *)(sk + c0 + 4 * lane);
    const uint32_t m01 = v.x > v.y ? v.x : v.y, m23 = v.z > v.w ? v.z : v.w;
    if (__any((m01 > m23 ? m01 : m23) == kEmpty32)) {   // (wave uniform, rare: the sketch is nearly full)
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const bool e = w[i] == kEmpty32;
        const uint64_t bal = __builtin_amdgcn_ballot_w64(e);
        const uint32_t at = n_e + __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
        if (e && at < 64u) list[at] = c0 + 4 * lane + (uint32_t)i;
        n_e += (uint32_t)__builtin_popcountll(bal);
      }
    }
  }
  wave_lds_sync();
  if (n_e > 64u) return false;   // (cannot happen: the caller counted)
  const uint32_t cells = lane < n_e ? list[lane] : 0u;
  // ---- the entries' orbits: stride = 2^j odd; B = 0 (mod F): the orbit is the one cell T (j = log2 F, s = 0) ----
  uint32_t low[R], jsh[R], inv[R], win_min[R], lose_max[R];
#pragma unroll
  for (int k = 0; k < R; ++k) {
    const uint32_t j = (uint32_t)__builtin_ctz((B[k] & Fm) | F);
    const uint32_t odd = (B[k] >> j) | 1u;
    uint32_t x = odd;                       // correct to 3 bits; every step doubles them
#pragma unroll
    for (int i = 0; i < 3; ++i) x *= 2u - odd * x;
    low[k] = (1u << j) - 1u;
    jsh[k] = j;
    inv[k] = x;
    win_min[k] = 0xFFFFFFFFu;
    lose_max[k] = 0u;
  }
  // one cell: its keys per entry (s << 15 | index; all ones: the orbit never reaches it) and the lane's smallest
  auto solve = [&](uint32_t c, uint32_t (&key)[R]) -> uint32_t {
    uint32_t best = 0xFFFFFFFFu;
#pragma unroll
    for (int k = 0; k < R; ++k) {
      const uint32_t x = c - T[k];
      const uint32_t s = ((x * inv[k]) & Fm) >> jsh[k];   // valid when 2^j divides x
      key[k] = (x & low[k]) == 0u ? ((s << 15) | (mk[k] & 0x7FFFu)) : 0xFFFFFFFFu;
      best = key[k] < best ? key[k] : best;
    }
    return best;
  };
  // ... and what follows from the wave's smallest key: the winner's value, the passes of wins and of lost ties
  auto settle = [&](uint32_t ci, uint32_t wkey, const uint32_t (&key)[R]) {
    if (wkey == 0xFFFFFFFFu) return;        // no orbit reaches the cell: it stays empty
    const uint32_t s_star = wkey >> 15, top = wkey | 0x7FFFu;
    uint32_t n_tied = 0;
#pragma unroll
    for (int k = 0; k < R; ++k) {
      n_tied += (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(key[k] <= top));
      if (key[k] == wkey) {
        vals[ci] = V[k];
        win_min[k] = s_star < win_min[k] ? s_star : win_min[k];
      }
    }
    if (n_tied > 1u) {   // (wave uniform, rare) the entries that reach the cell in its pass and lose it
#pragma unroll
      for (int k = 0; k < R; ++k)
        if (key[k] <= top && key[k] != wkey) lose_max[k] = s_star > lose_max[k] ? s_star : lose_max[k];
    }
  };
  for (uint32_t ci = 0; ci < n_e; ++ci) {   // (wave uniform; two cells per round are no faster)
    uint32_t key[R];
    const uint32_t best = solve((uint32_t)__builtin_amdgcn_readlane((int)cells, (int)ci), key);
    settle(ci, wave_min_u32(best), key);
  }
  bool bad = false;
#pragma unroll
  for (int k = 0; k < R; ++k) bad |= win_min[k] < lose_max[k];
  if (__any(bad)) return false;
  wave_lds_sync();
  if (lane < n_e) {
    const uint32_t v = vals[lane];
    if (v != kEmpty32) sk[cells] = v;
  }
  wave_lds_sync();
  return true;
}

// The passes over R register entries per lane (entry e = k*64 + lane of elist), targets read a window ahead.
//
// A pass of the reference's loop (src/niqki_index.cpp:313-331) changes a cell only where an entry's target is EMPTY,
// and in the coupon-collector tail (half of a read's ~420 passes run with fewer than 256 of the 4096 cells empty)
// almost no target is.  So the targets of the next U passes are read first -- U x R plain LDS reads per lane in ONE
// round trip -- and a pass then costs LDS traffic only for the entries whose target was empty in that window read:
// they alone propose (ds_min), read back and, where they won, write; a pass without such an entry anywhere in the
// wave costs one ballot.  The window read may be stale for the later passes of its window in one direction only: a
// cell it saw empty may have been filled by an earlier pass of the window (cells never go back to empty); the
// proposal that follows is then a ds_min on an occupied cell, which changes nothing, and its read-back is not the
// proposer's own word.  Exactly the passes of the plain loop it replaced (every entry proposing in every pass);
// 1.05 x its speed on 150- and 300-base reads (profiles/r06_densify_forms.txt, form a: the passes are paid in LDS
// instructions, and this form issues fewer only where no lane proposes).
template <int R, int U>
__device__ __forceinline__ void densify_wave_entries_window(uint32_t *sk, const uint32_t *elist, uint32_t n_ent,
                                                            uint32_t F, uint32_t empty, uint32_t *scratch, bool tail) {
  const uint32_t lane = threadIdx.x, Fm = F - 1u;
  uint32_t T[R], B[R], mk[R], V[R];
  // A lane without an entry in round k watches a cell that is occupied from the start (entry 0's own) and never
  // moves on (B = 0): its window reads never show "empty", so it never proposes and the passes need no validity test.
  const uint32_t cell0 = elist[0];
#pragma unroll
  for (int k = 0; k < R; ++k) {
    const uint32_t e = (uint32_t)k * 64u + lane;
    const bool valid = e < n_ent;
    const uint32_t v = valid ? elist[2 * e + 1] : 0u;
    V[k] = v;
    mk[k] = valid ? (0x80000000u | elist[2 * e]) : kEmpty32;
    T[k] = valid ? (uint32_t)unrev64(v) : cell0;
    B[k] = valid ? (uint32_t)rev64(v) : 0u;
  }
  uint32_t idle = 0;
  for (;;) {
    uint32_t pre[U][R];
    {
      uint32_t t[R];
#pragma unroll
      for (int k = 0; k < R; ++k) t[k] = T[k];
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int k = 0; k < R; ++k) {
          pre[u][k] = sk[t[k] & Fm];
          t[k] += B[k];
        }
    }
    wave_lds_order();
    // The exit tests run once per window: a pass behind the one that filled the last cell finds no empty target
    // (or a stale "empty", whose proposal changes nothing), and fruitless passes beyond the F that prove a fixpoint
    // change nothing either -- the cells are those of the loop that stops at the pass itself.
    uint32_t wins = 0;   // per lane; summed over the wave once per window
#pragma unroll
    for (int u = 0; u < U; ++u) {
      bool prop[R], any = false;
#pragma unroll
      for (int k = 0; k < R; ++k) {
        prop[k] = pre[u][k] == kEmpty32;
        any |= prop[k];
      }
      if (__any(any)) {   // wave uniform
#pragma unroll
        for (int k = 0; k < R; ++k)
          if (prop[k]) atomicMin(&sk[T[k] & Fm], mk[k]);
        wave_lds_order();
        // all proposals of the wave are issued before any read-back: a read sees the surviving proposal of its cell
        // (which names exactly one entry: the markers of two entries never agree), or a value -- another pass's or,
        // behind its winner's write, this pass's.  (Read by all lanes: the LDS is paid per instruction, and a mask
        // around it costs two scalar instructions.)
        uint32_t back[R];
#pragma unroll
        for (int k = 0; k < R; ++k) back[k] = sk[T[k] & Fm];
        wave_lds_order();
#pragma unroll
        for (int k = 0; k < R; ++k) {
          const uint32_t t = T[k] & Fm;
          const bool won = prop[k] && back[k] == mk[k];
          if (won) {
            sk[t] = V[k];
            const uint32_t m = 0x80000000u | t;
            mk[k] = m < mk[k] ? m : mk[k];
            ++wins;
          }
        }
        wave_lds_order();
      }
#pragma unroll
      for (int k = 0; k < R; ++k) T[k] += B[k];
    }
    const uint32_t tot_w = wave_sum_u32(wins);
    empty -= tot_w;
    idle = tot_w ? 0u : idle + (uint32_t)U;
    if (empty == 0 || idle >= F) return;
    if (tail && empty <= kTailCells) {   // (wave uniform) the last cells in closed form; once
      if (densify_tail<R>(sk, scratch, F, T, B, mk, V)) return;
      tail = false;
    }
  }
}

__global__ __launch_bounds__(64) void sketch_reads_kernel(SketchArgs a) {
  extern __shared__ __align__(16) uint32_t smem[];
  const Derived &d = a.d;
  const uint32_t F = d.F, lane = threadIdx.x;
  uint32_t *sk = smem;                                       // F cells
  // one region behind the cells: position codes + code table while the k-mers are hashed, then the entry list
  uint32_t *elist = smem + F;                                // a.read_entries x {cell, value}
  uint8_t *codes = (uint8_t *)elist;                         // kReadTile position codes
  uint8_t *lut = codes + kReadTile;                          // 256-byte code table
  const uint32_t cap = a.read_entries;
  const uint32_t entry = blockIdx.x;
  const uint32_t K = d.K, Km1 = d.K - 1u;
  if (a.redo_only && a.redo[entry] != a.redo_only) return;   // (one wave: uniform) not this launch's sketch

  for (uint32_t i = lane; i < 256; i += 64) lut[i] = code_entry(i);
  // (the kernel's time is its LDS instructions: the passes over all cells move 16 bytes per lane; F is a multiple
  // of 256 on this path -- S >= 8 -- or the loops below fall back to single cells)
  const bool quads = (F & 255u) == 0u && ((uintptr_t)a.sketches & 15u) == 0u;   // (the caller's rows: 16-byte aligned as a rule)
  if (a.accumulate) {
    const uint32_t *src = (const uint32_t *)a.sketches + (uint64_t)entry * F;
    if (quads) for (uint32_t i = 4 * lane; i < F; i += 256) *(uint4 *)(sk + i) = *(const uint4 *)(src + i);
    else for (uint32_t i = lane; i < F; i += 64) sk[i] = src[i];
  } else {
    if (quads) for (uint32_t i = 4 * lane; i < F; i += 256) *(uint4 *)(sk + i) = make_uint4(kEmpty32, kEmpty32, kEmpty32, kEmpty32);
    else for (uint32_t i = lane; i < F; i += 64) sk[i] = kEmpty32;
  }
  __syncthreads();

  // ---- k-mers: positions are coded tile by tile (forward code | rc code << 2 per position,
  // "positional codes" of DESIGN.md), every lane then assembles whole k-mers from K codes ----
  if (a.seqs != nullptr) {
    const uint32_t r0 = a.entry_rec ? a.entry_rec[entry] : entry;
    const uint32_t r1 = a.entry_rec ? a.entry_rec[entry + 1] : entry + 1;
    for (uint32_t rec = r0; rec < r1; ++rec) {
      const uint64_t b0 = a.rec_off[rec], b1 = a.rec_off[rec + 1];
      const uint64_t len = b1 - b0;
      if (len <= K) continue;                 // src/niqki_index.cpp:395,:450
      const uint64_t n_kmers = len - K;       // last k-mer skipped, :342
      const uint8_t *base = a.seqs + b0;
      // the K-1 prefix digits are zeroed together when one of them is no base (:255-273)
      uint32_t ok = 1;
      if (lane < Km1) ok = (lut[base[lane]] >> 6) & 1u;
      ok = __all(ok) ? 1u : 0u;
      const uint32_t per_tile = kReadTile - Km1;   // k-mers served by one tile of positions
      for (uint64_t k0 = 0; k0 < n_kmers; k0 += per_tile) {
        __syncthreads();  // the previous tile's codes are no longer read
        for (uint32_t j = lane; j < kReadTile; j += 64) {
          const uint64_t pos = k0 + j;
          uint32_t c = 0;
          if (pos < len) {
            const uint32_t e = lut[base[pos]];
            if (pos < Km1) {
              const uint32_t dgt = ok ? ((e >> 4) & 3u) : 0u;
              c = dgt | ((3u - dgt) << 2);      // digit and its complement (rcb, :240-250)
            } else {
              c = e & 15u;                       // rolling tables (:114-123, :211-221)
            }
          }
          codes[j] = (uint8_t)c;
        }
        __syncthreads();
        const uint64_t left = n_kmers - k0;
        const uint32_t n_here = left < per_tile ? (uint32_t)left : per_tile;
        for (uint32_t q = lane; q < ((n_here + 63u) & ~63u); q += 64) {
          const bool live = q < n_here;
          uint64_t fw = 0, rc = 0;
          if (live) {
            for (uint32_t j = 0; j < K; ++j) {
              const uint32_t c = codes[q + j];
              fw = (fw << 2) | (c & 3u);
              rc |= (uint64_t)(c >> 2) << (2u * j);
            }
          }
          const uint64_t canon = min62(fw, rc);   // :345
          sketch_update(canon, d, sk, live);
        }
      }
    }
  }
  __syncthreads();

  uint32_t *out = (uint32_t *)a.sketches + (uint64_t)entry * F;
  if (a.densify) {
    // ---- entries: the occupied cells, dealt to the lanes (any order: an entry only knows its own cell and value) ----
    uint32_t n_ent = 0;
    if (quads) {
      for (uint32_t c0 = 0; c0 < F; c0 += 256) {
        const uint4 q4 = *(const uint4 *)(sk + c0 + 4 * lane);
        const uint32_t w[4] = {q4.x, q4.y, q4.z, q4.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const uint64_t bal = __ballot(w[i] != kEmpty32);
          if (bal) {   // (wave uniform: a read's sketch is nearly empty here)
            const uint32_t at = n_ent + __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
            if (w[i] != kEmpty32 && at < cap) { elist[2 * at] = c0 + 4 * lane + (uint32_t)i; elist[2 * at + 1] = w[i]; }
            n_ent += (uint32_t)__popcll(bal);
          }
        }
      }
    } else {
      for (uint32_t c0 = 0; c0 < F; c0 += 64) {
        const uint32_t c = c0 + lane;
        const uint32_t v = c < F ? sk[c] : kEmpty32;
        const uint64_t bal = __ballot(v != kEmpty32);
        const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
        const uint32_t at = n_ent + rank;
        if (v != kEmpty32 && at < cap) { elist[2 * at] = c; elist[2 * at + 1] = v; }
        n_ent += (uint32_t)__popcll(bal);
      }
    }
    __syncthreads();
    const uint32_t empty0 = F - n_ent;
    if (empty0 != 0 && n_ent != 0) {
      if (n_ent > cap && a.redo_mark) {
        // more occupied cells than the entry list holds (a record far longer than the batch's average): a later
        // launch -- the long list, then the workgroup kernel -- sketches it again; the plain pass over all cells
        // would take fifty times a read's time.  Nothing of this sketch is stored here.
        if (lane == 0) a.redo[entry] = a.redo_mark;
        return;
      }
      if (n_ent > cap) {
        densify_wave_cells(sk, d, empty0);
      } else {
        const uint32_t rounds = (n_ent + 63u) >> 6;   // wave uniform
        // (the entries are in registers by then: their list's space holds the tail's two lists; the closed-form
        // tail runs where the cells are moved as quads)
        uint32_t *scratch = elist;
        static_assert(192 * 8 >= 2 * 64 * 4, "the tail's lists live in the entry list's space");
        if (rounds <= 1) densify_wave_entries_window<1, 8>(sk, elist, n_ent, F, empty0, scratch, quads);
        else if (rounds <= 2) densify_wave_entries_window<2, 8>(sk, elist, n_ent, F, empty0, scratch, quads);
        else if (rounds <= 3) densify_wave_entries_window<3, 4>(sk, elist, n_ent, F, empty0, scratch, quads);
        else if (rounds <= 4) densify_wave_entries_window<4, 4>(sk, elist, n_ent, F, empty0, scratch, quads);
        else densify_wave_entries_window<6, 4>(sk, elist, n_ent, F, empty0, scratch, quads);
        static_assert(kReadEntries == 6, "dispatch above covers 1..6 rounds");
      }
    }
    __syncthreads();
  }
  if (quads) for (uint32_t i = 4 * lane; i < F; i += 256) *(uint4 *)(out + i) = *(const uint4 *)(sk + i);
  else for (uint32_t i = lane; i < F; i += 64) out[i] = sk[i];
}

hipError_t launch_sketch_reads(const SketchArgs &a, uint32_t n_entry, size_t lds, hipStream_t stream) {
  hipError_t e = hipFuncSetAttribute((const void *)sketch_reads_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(sketch_reads_kernel, dim3(n_entry), dim3(64), lds, stream, a);
  return hipGetLastError();
}

}  // namespace nq
