// nq_gather.hip -- kernel #4: gather-histogram query over the inverted index, for gfx950.
//
// Replaces the counting loop of Index::query_sketch (src/niqki_index.cpp:652-661): gather_kernel.  What follows
// it in the reference, the threshold and the order of the hits, is nq_hits.hip.
//
// gather_kernel: one workgroup per query, the genome tiles walked one after
// another.  The tile's per-genome hit counters live in LDS as packed u16 pairs (a
// count never exceeds F <= 2^15, so the two halves of a word cannot carry into
// each other) and are bumped with ds_add_u32.  Each wave takes 64 sketch slots at
// a time: every lane looks up the bucket of its slot for ALL tiles with one random
// table access (the other tiles' entries are parked in a coalesced stash), then
// the wave walks the 64 buckets one after another, all lanes reading consecutive
// u16 genome ids of one 128-byte aligned bucket.  HBM-bound by design:
// algorithmic bytes per query = 4T + 20F.  On large indexes the
// queries of a launch are first put into a locality order (probe_kernel,
// order_kernel): similar queries then run on the same XCD at the same time and
// share their table and bucket lines through its L2.  For real batches the table
// look-ups are taken out of the kernel altogether by a pre-pass (lookup_rows_kernel
// / lookup_kernel) that walks the table slot block by slot block for all queries of
// the launch; the gather kernel then reads one packed word per (tile, slot).
#include "nq_kernels.h"

#include <algorithm>
#include <cstdlib>

namespace nq {

typedef __attribute__((address_space(3))) uint32_t lds_u32;
typedef __attribute__((address_space(3))) void lds_void;
typedef __attribute__((address_space(1))) const void glb_cvoid;

__device__ __forceinline__ void bump(uint32_t *cnt, uint32_t g) {
  atomicAdd(&cnt[g >> 1], 1u << ((g & 1u) * 16u));  // ds_add_u32, result unused
}
// Branch-free form for the bucket walks: lanes past the end of the bucket add 0 to a
// word of their own (no exec-mask juggling, no same-address serialisation).
__device__ __forceinline__ void bump_if(uint32_t *cnt, uint32_t g, bool on, uint32_t lane) {
  const uint32_t gg = on ? g : 2u * lane;
  const uint32_t inc = on ? (1u << ((g << 4) & 31u)) : 0u;   // 1 << 16 * (g & 1): the shifter takes the low 5 bits
  atomicAdd(&cnt[gg >> 1], inc);
}

// A bucket chunk: up to 64 consecutive ids at unit `pos` (1 << align_log2 ids per
// unit, counted from the tile's base).
struct Item {
  uint32_t pos, len;
};
constexpr uint32_t kQueue = 256;  // items per wave-private LDS work queue
static_assert(hit_list_lds(0, 0) == kPadWords * 4 + 16 * kQueue * sizeof(Item), "hit_list_lds (nq_kernels.h) counts these queues");

// Walks 64 chunks held one per lane (pos, len <= 64): all lanes read consecutive
// u16 ids of one chunk, UNROLL chunks per round trip, two rounds in flight (the
// loads of round r+1 are issued before the LDS atomics of round r; unconditional
// loads, lanes past a chunk's end read what follows it and are masked).
// The form of indexes that are not padded; padded ones take PairWalk below.
// n (wave uniform, PARTIAL only): how many of the 64 lanes hold a chunk -- the last batch of a tile's walk; a short
// read's whole walk is such a batch of ~10 chunks per wave, and walking all 64 places cost it half of its instructions.
template <int UNROLL, bool PARTIAL = false>
__device__ __forceinline__ void walk64(const uint16_t *gl, uint32_t a, uint32_t pos, uint32_t len,
                                       uint32_t lane, uint32_t *cnt, uint32_t n = 64) {
  uint32_t ga[UNROLL], gb[UNROLL];
  auto fetch = [&](uint32_t j0, uint32_t (&g)[UNROLL]) {
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const uint32_t b = __builtin_amdgcn_readlane(pos, j0 + u);
      g[u] = (gl + ((uint64_t)b << a))[lane];
    }
  };
  auto apply = [&](uint32_t j0, uint32_t (&g)[UNROLL]) {
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const uint32_t l = __builtin_amdgcn_readlane(len, j0 + u);
      bump_if(cnt, g[u], lane < l, lane);
    }
  };
  fetch(0, ga);
  if constexpr (PARTIAL) {
#pragma unroll
    for (uint32_t j0 = 0; j0 < 64; j0 += 2 * UNROLL) {
      const bool more1 = j0 + UNROLL < n;   // (wave uniform)
      if (more1) fetch(j0 + UNROLL, gb);
      apply(j0, ga);
      if (!more1) break;
      const bool more2 = j0 + 2 * UNROLL < 64 && j0 + 2 * UNROLL < n;
      if (more2) fetch(j0 + 2 * UNROLL, ga);
      apply(j0 + UNROLL, gb);
      if (!more2) break;
    }
    return;
  }
#pragma unroll
  for (uint32_t j0 = 0; j0 < 64; j0 += 2 * UNROLL) {
    fetch(j0 + UNROLL, gb);
    apply(j0, ga);
    if (j0 + 2 * UNROLL < 64) fetch(j0 + 2 * UNROLL, ga);
    apply(j0 + UNROLL, gb);
  }
}

// The padded walk's form (PAD, 64-id lines): ONE load instruction fetches TWO lines -- lanes 0..31 read
// the 32 dwords of one chunk's line, lanes 32..63 those of the next chunk's -- and every lane counts the two
// ids of its dword.  The CU's texture-address unit takes a wave-wide load every ~7.7 cycles whatever its
// width (tools/ubench_lines.hip: 271 loads per microsecond and CU from L2, ushort or dword), so at one
// line per instruction the walk was bound by load issue (31 SIMD cycles per line) before HBM; the lanes
// take their chunk's position straight from the wave's LDS queue (one ds_read_b32 per load, its queue
// slot in the instruction's offset field) instead of a v_readlane + s_lshl per line.  Per line now:
// 0.5 load, 0.5 LDS read, ~5 vector ALU ops, 1 LDS atomic per lane and id (2 per load).
// Beside the sketch kernel the launch runs on a quarter of the CUs and the CU's LDS pipe counts: an atomic costs what its
// active lanes and their bank conflicts cost (tools/ubench_lds_atomics.hip, rows 6 and 7), so the lanes that hold nothing
// but padding ids (39 % at the bench's fill) leave both atomics of their load (apply).
template <int UNROLL>
struct PairWalk {
  static_assert(UNROLL == 16 || UNROLL == 32, "a round is UNROLL lines = UNROLL / 2 loads; two or four rounds per batch");
  static constexpr int L = UNROLL / 2;   // loads per round
  const uint8_t *lane_base;              // tile's ids + this lane's dword within a line
  uint32_t half;                         // lane >> 5: which chunk of a pair this lane reads
  uint32_t ga[L], gb[L];

  uint32_t tile;                         // ids from here on are padding ids (IndexView::padded)

  __device__ __forceinline__ void init(const uint16_t *gl, uint32_t lane, uint32_t tile_ids) {
    lane_base = (const uint8_t *)gl + (lane & 31u) * 4u;
    half = lane >> 5;
    tile = tile_ids;
  }
  // loads of the chunks [j0, j0 + UNROLL) of the batch whose items start at `items` (LDS, this wave's queue)
  __device__ __forceinline__ void fetch(uint32_t (&g)[L], const Item *items, uint32_t j0) {
    const Item *mine = items + half;
    uint32_t pos[L];   // line index within the tile (align_log2 = 6); all LDS reads first, one wait for them
#pragma unroll
    for (int k = 0; k < L; ++k) pos[k] = mine[j0 + 2 * k].pos;
    asm volatile("" ::: "memory");
#pragma unroll
    for (int k = 0; k < L; ++k) {
      uint64_t addr;   // lane_base + 128 * pos in one vector op
      asm("v_mad_u64_u32 %0, vcc, %1, %2, %3" : "=v"(addr) : "v"(pos[k]), "s"(128u), "v"((uint64_t)lane_base) : "vcc");
      g[k] = *(const __attribute__((address_space(1))) uint32_t *)addr;   // (global_load, not flat)
    }
  }
  __device__ __forceinline__ void apply(uint32_t (&g)[L]) {
#pragma unroll
    for (int k = 0; k < L; ++k) {
      // per id: word g >> 1, increment 1 << 16 * (g & 1); the counters start at LDS address 0, so the word's
      // byte offset IS its LDS address.  and / add issue in 2.8 cycles on gfx950, the mad in 4.4
      // (profiles/r03_opcode_costs.txt).
      uint32_t even, addr, odd, inc, hi;
      asm("v_and_b32 %0, 0xfffe, %1" : "=v"(even) : "v"(g[k]));
      // A chunk's ids stand at the front of its line, padding ids (tile + 2 * position, the tile even) behind them: a
      // dword whose first id is a padding id lies wholly beyond the chunk's length, and its lane leaves both atomics
      // (it would add to dummy words that nobody reads).  The lane with the last id of an odd-length chunk stays, its
      // second id lands in the dummy words as before; a "no chunk" line of the last batch has no lane left.
      if (even < tile) {
        asm("v_add_u32 %0, %1, %1" : "=v"(addr) : "v"(even));
        asm("v_and_b32 %0, 1, %1" : "=v"(odd) : "v"(g[k]));
        asm("v_mad_u32_u24 %0, %1, %2, 1" : "=v"(inc) : "v"(odd), "s"(0xFFFFu));
        __hip_atomic_fetch_add((lds_u32 *)(uintptr_t)addr, inc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        asm("v_lshrrev_b32 %0, 16, %1" : "=v"(hi) : "v"(g[k]));
        asm("v_and_b32 %0, 0xfffe, %1" : "=v"(even) : "v"(hi));
        asm("v_add_u32 %0, %1, %1" : "=v"(addr) : "v"(even));
        asm("v_and_b32 %0, 1, %1" : "=v"(odd) : "v"(hi));
        asm("v_mad_u32_u24 %0, %1, %2, 1" : "=v"(inc) : "v"(odd), "s"(0xFFFFu));
        __hip_atomic_fetch_add((lds_u32 *)(uintptr_t)addr, inc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
    }
  }
  // 64 chunks: items[0 .. 64) of the wave's queue; all their lines in flight before the first id is counted
  // (keeping a round in flight across batches, over the cutting of the next buckets, gained nothing: measured)
  __device__ __forceinline__ void batch(const Item *items) {
    constexpr int R = 64 / UNROLL;
    fetch(ga, items, 0);
#pragma unroll
    for (int r = 0; r < R; r += 2) {
      fetch(gb, items, (r + 1) * UNROLL);
      apply(ga);
      if (r + 2 < R) fetch(ga, items, (r + 2) * UNROLL);
      apply(gb);
    }
  }
};

// One pass of a workgroup over all slots of one tile.
//   STASH_OUT: the lookup fetched the entries of NT tiles at once; tile 0 is
//              walked now, the others are parked in `stash` (coalesced) for the
//              later passes, so every slot costs ONE random table line per query.
//   STASH_IN : entries come from the stash (coalesced 8-byte loads).
// Each wave takes 64 slots per iteration; lookups run one iteration ahead,
// fingerprints two.  Buckets are cut into chunks of <= 64 ids that go through a
// wave-private LDS queue, so the walk always runs on full batches of 64 chunks
// whatever the bucket lengths are.
//   PRE      : entries come from the slot-major look-up pre-pass (lookup_kernel below): one
//              packed word per (query, tile, slot) = bucket start relative to the slot's first
//              unit << 16 | length, read coalesced; no table access in this kernel at all.
//   PAD      : padded index (whole-line chunks): batches go through PairWalk (two lines per load), and the four
//              waves of a SIMD take turns at the top issue priority; otherwise walk64 with explicit lengths.
//   ahead    : (PRE) this wave's first two look-ups of the tile, issued a tile earlier by the caller / this function.
template <int BLOCK, int UNROLL, int NT, bool STASH_OUT, bool STASH_IN, bool PRE = false, bool PAD = false>
__device__ __forceinline__ void walk_tile(const IndexView &v, const int32_t *sk, uint32_t q, uint32_t t,
                                          uint32_t *cnt, Item *queue, Entry *stash,
                                          uint32_t it_lo, uint32_t n_it, const uint32_t *pre = nullptr,
                                          Entry *ahead = nullptr) {
  // slots [64 * it_lo, min(64 * n_it, f_local)): one pass of the kernel
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  constexpr uint32_t NW = BLOCK / 64;
  constexpr int NE = STASH_OUT ? NT : 1;  // entries fetched per lookup
  const uint32_t R = v.d.R, a = v.align_log2;
  const uint16_t *gl = v.gids + v.tile_base[t];
  Entry *my_stash = PRE ? nullptr : stash + (uint64_t)q * (v.n_tiles - 1) * v.f_local;
  const uint32_t *my_pre = PRE ? pre + ((uint64_t)q * v.n_tiles + t) * v.f_local : nullptr;
  const uint32_t *my_units = v.slot_units + (uint64_t)t * (v.f_local + 1);
  Item *wq = queue + wave * kQueue;
  uint32_t q_head = 0, q_count = 0;  // wave-uniform
  constexpr bool PAIR = PAD && (UNROLL == 16 || UNROLL == 32);
  uint32_t prio_turn = wave >> 2;   // the four waves of a SIMD take turns at the issue arbiter's top priority (PAIR)
  PairWalk<PAIR ? UNROLL : 32> pw;
  pw.init(gl, lane, v.tile);

  struct Look { Entry e[NE]; };
  // HM: a single-tile index with its per-slot class mask (IndexView::hmask): a fingerprint whose class holds no
  // bucket in its slot is never looked up, its table line never requested (the masked loop below).
  constexpr bool HM_FORM = NE == 1 && NT == 1 && !STASH_IN && !PRE;
  const uint16_t *hm = HM_FORM ? v.hmask : nullptr;
  auto slot_ok = [&](uint32_t it) -> bool { return it < n_it && it * 64 + lane < v.f_local; };
  auto load_fp = [&](uint32_t it) -> int32_t {
    if (STASH_IN || PRE) return 0;
    const uint32_t s = it * 64 + lane;
    return sk[s < v.f_local ? s : v.f_local - 1];
  };
  auto valid_of = [&](uint32_t it, int32_t fp) -> bool {
    if (STASH_IN || PRE) return slot_ok(it);
    return slot_ok(it) && fp >= 0 && (uint32_t)fp < R;  // src/niqki_index.cpp:654
  };
  // unconditional loads from clamped addresses: they stay in flight across the walk
  auto lookup = [&](uint32_t it, int32_t fp) -> Look {
    Look L;
    uint32_t s = it * 64 + lane;
    if (s >= v.f_local) s = v.f_local - 1;
    if (PRE) {
      const uint32_t w = my_pre[s];
      L.e[0] = Entry{my_units[s] + (w >> 16), w & 0xFFFFu};
    } else if (STASH_IN) {
      L.e[0] = my_stash[(uint64_t)(t - 1) * v.f_local + s];
    } else {
      const bool ok = fp >= 0 && (uint32_t)fp < R;
      const Entry *p = v.entries + ((uint64_t)s * R + (ok ? (uint32_t)fp : 0u)) * v.n_tiles + (STASH_OUT ? 0u : t);
#pragma unroll
      for (int k = 0; k < NE; ++k) L.e[k] = p[k];
    }
    return L;
  };
  auto drain = [&]() {
    while (q_count >= 64) {
      if constexpr (PAIR) {
        // the issue arbiter serves the oldest wave of a SIMD first: left alone, the four waves of a SIMD finish
        // a tile 3 us apart (18 / 20 / 23 / 26 us) and the youngest runs the last stretch alone
        prio_turn = (prio_turn + 1) & 3;
        if (prio_turn == 0) __builtin_amdgcn_s_setprio(0);
        else if (prio_turn == 1) __builtin_amdgcn_s_setprio(1);
        else if (prio_turn == 2) __builtin_amdgcn_s_setprio(2);
        else __builtin_amdgcn_s_setprio(3);
        pw.batch(wq + q_head);             // (q_head is a multiple of 64: a batch never wraps; a wave's LDS traffic is in order)
        q_head = (q_head + 64) & (kQueue - 1);
        q_count -= 64;
        continue;
      }
      const Item x = wq[(q_head + lane) & (kQueue - 1)];
      q_head = (q_head + 64) & (kQueue - 1);
      q_count -= 64;
      walk64<UNROLL>(gl, a, x.pos, x.len, lane, cnt);
    }
  };

  // cut the wave's 64 buckets (start `pos`, `rem` ids left; rem = 0: none) into chunks of <= 64 ids, at most 3 per
  // lane and round (q_count < 64 on entry, so at most 63 + 192 items are ever queued), and walk full batches
  auto cut_and_walk = [&](uint32_t pos, uint32_t rem) {
    const uint32_t step = 64u >> a;  // units per 64 ids (align_log2 <= 6)
    do {
      uint32_t nch = (rem + 63) >> 6;
      if (nch > 3) nch = 3;
      // exclusive prefix of nch (two bits) over the lanes from two ballots: bit counts below the lane (v_mbcnt) instead
      // of a six-step shuffle scan through the LDS crossbar
      const uint64_t b0 = __ballot((nch & 1u) != 0), b1 = __ballot((nch & 2u) != 0);
      const uint32_t excl = __builtin_amdgcn_mbcnt_hi((uint32_t)(b0 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b0, 0u)) +
                            2u * __builtin_amdgcn_mbcnt_hi((uint32_t)(b1 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b1, 0u));
      const uint32_t total = (uint32_t)__popcll(b0) + 2u * (uint32_t)__popcll(b1);
      uint32_t slot = q_head + q_count + excl;
#pragma unroll
      for (uint32_t k = 0; k < 3; ++k)
        if (k < nch) {
          const uint32_t left = rem - 64 * k;
          wq[(slot + k) & (kQueue - 1)] = Item{pos + step * k, left < 64 ? left : 64u};
        }
      q_count += total;
      pos += step * nch;
      rem -= rem < 192 ? rem : 192u;
      drain();
    } while (__any(rem != 0));
  };

  if (HM_FORM && hm) {
    // Masked form (single-tile index with its per-slot class mask): most of a query's fingerprints fall into
    // classes that hold no bucket in their slot -- for a short read against a genome index, ~99 % -- so the loop
    // is bound by the latency of its own input.  All loads of kDeep iterations are issued before any is used:
    // fingerprints and mask words first, then (only for lanes that still hold a fingerprint, only in iterations
    // where some lane does) the table entries.
    constexpr int kDeep = 8;
    for (uint32_t it0 = it_lo + wave; it0 < n_it; it0 += kDeep * NW) {
      int32_t fpv[kDeep];
      uint32_t mw[kDeep];
#pragma unroll
      for (int k = 0; k < kDeep; ++k) {
        uint32_t s = (it0 + k * NW) * 64 + lane;
        s = s < v.f_local ? s : v.f_local - 1;
        fpv[k] = sk[s];
        mw[k] = hm[s];
      }
      Entry en[kDeep];
      bool live[kDeep];
#pragma unroll
      for (int k = 0; k < kDeep; ++k) {
        const uint32_t itk = it0 + k * NW;
        const int32_t fp = fpv[k];
        const bool ok = slot_ok(itk) && fp >= 0 && (uint32_t)fp < R && ((mw[k] >> ((uint32_t)fp >> v.hmask_shift)) & 1u);   // :654
        live[k] = __any(ok);
        en[k] = Entry{0u, 0u};
        if (ok) {
          uint32_t s = itk * 64 + lane;
          en[k] = v.entries[((uint64_t)s * R + (uint32_t)fp) * v.n_tiles + t];
        }
      }
#pragma unroll
      for (int k = 0; k < kDeep; ++k)
        if (live[k]) cut_and_walk(en[k].start, en[k].len);   // (wave-uniform)
    }
    if (q_count) {  // the last partial batch; "no chunk" = the tile's spare line of padding ids
      if constexpr (PAIR) {
        if (lane >= q_count) wq[q_head + lane] = Item{my_units[v.f_local], 0u};
        pw.batch(wq + q_head);
      } else {
        Item x = wq[(q_head + lane) & (kQueue - 1)];
        if (lane >= q_count) x = Item{PAD ? my_units[v.f_local] : 0u, 0u};
        walk64<(UNROLL > 8 ? 8 : UNROLL), true>(gl, a, x.pos, x.len, lane, cnt, q_count);
      }
    }
    return;
  }

  // software pipeline: table look-ups run two iterations ahead of the walk, fingerprints
  // three (a pass over short buckets has little walk work to hide a look-up behind)
  uint32_t it = it_lo + wave;
  int32_t fp0 = load_fp(it);
  int32_t fp1 = load_fp(it + NW);
  int32_t fp2 = load_fp(it + 2 * NW);
  Look cur, nxt;
  if (PRE && ahead) {
    // `ahead`: this wave's first two look-ups of the tile, issued during the walk of the tile before
    // (a slot shard has only a few iterations per tile: nothing else hides their latency); the ones of
    // the next tile are put on their way now
    cur.e[0] = ahead[0];
    nxt.e[0] = ahead[1];
    if (t + 1 < v.n_tiles) {
      const uint32_t *np = my_pre + v.f_local, *nu = my_units + (v.f_local + 1);
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        uint32_t s = (it + k * NW) * 64 + lane;
        if (s >= v.f_local) s = v.f_local - 1;
        const uint32_t w = np[s];
        ahead[k] = Entry{nu[s] + (w >> 16), w & 0xFFFFu};
      }
    }
  } else {
    cur = lookup(it, fp0);
    nxt = lookup(it + NW, fp1);
  }
  bool cur_ok = valid_of(it, fp0);
  bool nxt_ok = valid_of(it + NW, fp1);

  for (; it < n_it; it += NW) {
    const Look nxt2 = lookup(it + 2 * NW, fp2);
    const bool nxt2_ok = valid_of(it + 2 * NW, fp2);
    fp2 = load_fp(it + 3 * NW);
    uint32_t pos = cur.e[0].start, rem = cur_ok ? cur.e[0].len : 0u;
    if (STASH_OUT) {
      const uint32_t s = it * 64 + lane;
      if (s < v.f_local) {
#pragma unroll
        for (int k = 1; k < NE; ++k)
          my_stash[(uint64_t)(k - 1) * v.f_local + s] = Entry{cur.e[k].start, cur_ok ? cur.e[k].len : 0u};
      }
    }
    cut_and_walk(pos, rem);
    cur = nxt;
    cur_ok = nxt_ok;
    nxt = nxt2;
    nxt_ok = nxt2_ok;
  }
  if (q_count) {  // the last partial batch; "no chunk" = the tile's spare line of padding ids
    if constexpr (PAIR) {
      if (lane >= q_count) wq[q_head + lane] = Item{my_units[v.f_local], 0u};
      pw.batch(wq + q_head);
    } else {
      Item x = wq[(q_head + lane) & (kQueue - 1)];
      if (lane >= q_count) x = Item{PAD ? my_units[v.f_local] : 0u, 0u};
      walk64<(UNROLL > 8 ? 8 : UNROLL), true>(gl, a, x.pos, x.len, lane, cnt, q_count);
    }
  }
}

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
constexpr uint32_t kXcds = 8;
constexpr uint32_t kPreBlock = 256;      // queries per lookup workgroup, one per thread
constexpr uint32_t kPreFlight = 8;       // look-ups in flight per thread

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
constexpr uint32_t kRowSlots = 32, kRowBlock = 1024;
// The packed table (IndexView::ptab, one word per entry) keeps the tiles in GROUPS of two: the words of tiles
// t0, t0 + 1 (t0 even) of all slots lie together as [f_local][R][2] from this word on ([f_local][R][1] for a last
// odd tile) -- a launch over one group streams exactly its own rows.  With <= 2 tiles this is the whole table.
__host__ __device__ inline uint64_t packed_table_offset(const IndexView &v, uint32_t t0) { return (uint64_t)v.f_local * v.d.R * t0; }
__device__ __forceinline__ void wave_lds_fence() {   // this wave's LDS traffic so far has completed
  __builtin_amdgcn_wave_barrier();
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ void lds_barrier() {   // a workgroup barrier that waits for LDS traffic only:
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // the row loads in flight stay in flight
}
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
// Packed rows that the LDS buffers hold, dealt to 1024 threads in whole 16-byte loads: tiles are taken two at a
// time (rows of 2 R words = 32 KB at W = 12), a last odd tile alone.
bool lookup_wants_packed(const IndexView &v) {
  if (!launch_lookup_usable(v) || v.f_local % kRowSlots) return false;
  auto row_ok = [&](uint32_t nt) {   // a group's packed row: within 32 KB, whole 16-byte pieces per thread, 1 or 2 of them
    const uint32_t rw = v.d.R * nt;
    if (rw * 4u > 32768u || rw % (4u * kRowBlock)) return false;
    const uint32_t per = rw / (4u * kRowBlock);
    return per == 1 || per == 2;
  };
  if (v.n_tiles >= 2 && !row_ok(2)) return false;
  if ((v.n_tiles & 1u) && !row_ok(1)) return false;
  return true;
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

static uint32_t lookup_slots(const IndexView &v) { return v.n_tiles <= 2 ? 32u : 16u; }

// Can the pre-pass serve this index?  Whole slot blocks, and both halves of the packed word
// within 16 bits (bucket lengths <= tile, starts relative to the slot <= tile / unit + R units).
bool launch_lookup_usable(const IndexView &v) {
  if (v.n_tiles < 1 || v.f_local % lookup_slots(v)) return false;
  if (v.tile > 65535u) return false;
  return (uint64_t)(v.tile >> v.align_log2) + v.d.R + 1 <= 65535u;
}

size_t lookup_pre_bytes(const IndexView &v, uint32_t nq) { return (size_t)v.f_local * nq * v.n_tiles * 4; }

hipError_t launch_lookup(const IndexView &v, const int32_t *sketches, uint32_t nq, uint32_t *pre, hipStream_t stream) {
  if (nq == 0 || !launch_lookup_usable(v)) return hipErrorInvalidValue;
  if (v.ptab && lookup_wants_packed(v) && nq >= kRowBlock / 2) {
    const uint32_t n_sb = v.f_local / kRowSlots, n_qchunk = (nq + kRowBlock - 1) / kRowBlock;
    const uint64_t grid = (uint64_t)((n_sb + kXcds - 1) / kXcds * kXcds) * n_qchunk;
    if (grid > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipError_t e = hipSuccess;
#define NQ_LAUNCH_ROWS(NT, PER)                                                                                        \
  do {                                                                                                                 \
    e = hipFuncSetAttribute((const void *)lookup_rows_kernel<NT, PER>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
    if (e != hipSuccess) return e;                                                                                     \
    hipLaunchKernelGGL((lookup_rows_kernel<NT, PER>), dim3((uint32_t)grid), dim3(kRowBlock), lds, stream, v, sketches, nq, n_qchunk, pre, t0); \
  } while (0)
    for (uint32_t t0 = 0; t0 < v.n_tiles; t0 += 2) {   // tile groups (packed_table_offset)
      const uint32_t nt = v.n_tiles - t0 >= 2 ? 2u : 1u;
      const size_t lds = std::max<size_t>((size_t)v.d.R * nt * 4 * 4, (size_t)kRowBlock * (kRowSlots + 1) * 4);
      const uint32_t per = v.d.R * nt / (4u * kRowBlock);
      if (nt == 1) { if (per == 1) NQ_LAUNCH_ROWS(1, 1); else NQ_LAUNCH_ROWS(1, 2); }
      else { if (per == 1) NQ_LAUNCH_ROWS(2, 1); else NQ_LAUNCH_ROWS(2, 2); }
    }
#undef NQ_LAUNCH_ROWS
    return hipGetLastError();
  }
  const uint32_t ps = lookup_slots(v);
  const uint32_t n_sb = v.f_local / ps, n_qchunk = (nq + kPreBlock - 1) / kPreBlock;
  const uint64_t grid = (uint64_t)((n_sb + kXcds - 1) / kXcds * kXcds) * n_qchunk;
  if (grid > 0x7FFFFFFFull) return hipErrorInvalidValue;
#define NQ_LAUNCH_LOOKUP(NT, PS) \
  hipLaunchKernelGGL((lookup_kernel<NT, PS>), dim3((uint32_t)grid), dim3(kPreBlock), 0, stream, v, sketches, nq, n_qchunk, pre, t0)
  for (uint32_t t0 = 0; t0 < v.n_tiles; t0 += 4) {   // (blocks of 16 slots whenever there are more than 2 tiles)
    const uint32_t nt = v.n_tiles - t0 < 4 ? v.n_tiles - t0 : 4;
    if (ps == 32) { if (nt == 1) NQ_LAUNCH_LOOKUP(1, 32); else NQ_LAUNCH_LOOKUP(2, 32); }
    else if (nt == 1) NQ_LAUNCH_LOOKUP(1, 16);
    else if (nt == 2) NQ_LAUNCH_LOOKUP(2, 16);
    else if (nt == 3) NQ_LAUNCH_LOOKUP(3, 16);
    else NQ_LAUNCH_LOOKUP(4, 16);
  }
#undef NQ_LAUNCH_LOOKUP
  return hipGetLastError();
}

// ---- locality order of a query batch -----------------------------------------------------
// Queries that hit the same genomes read the same table and bucket lines.  When they run on
// the same XCD at the same time those lines are fetched from HBM once (measured: 13 % off the
// launch when the 4 queries of a family sit 8 blocks apart).  So a batch is ordered by its
// best probable hit: probe_kernel counts the first kProbeSlots slots only and takes the genome
// with the most hits as the query's key, order_kernel sorts (key, query), and gather_kernel
// maps sorted neighbours to one XCD.  Only the order of the work changes, never a result.
constexpr uint32_t kOrderGroup = 8;
constexpr uint32_t kProbeSlots = 16;
constexpr uint32_t kOrderMax = 4096;   // queries per launch (12 index bits next to a 20-bit key)

// Counters per block of kProbeBlock consecutive genomes (a key only has to bring the queries of one
// family together): a few KB of LDS instead of the gather kernel's whole tile, so many probes share
// a CU and hide each other's three dependent memory round trips (sketch -> entry -> ids).
constexpr uint32_t kProbeBlock = 64;
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void probe_kernel(IndexView v, const int32_t *sketches, uint32_t *keys) {
  extern __shared__ __align__(16) uint32_t cnt[];
  __shared__ uint32_t s_best;
  const uint32_t q = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const int32_t *sk = sketches + (uint64_t)q * v.q_stride + v.q_off;
  const uint32_t n_probe = v.f_local < kProbeSlots ? v.f_local : kProbeSlots;
  const uint32_t n_blocks = (v.n_genomes + kProbeBlock - 1) / kProbeBlock;
  if (tid == 0) s_best = 0;
  for (uint32_t i = tid; i < n_blocks; i += BLOCK) cnt[i] = 0;
  __syncthreads();
  for (uint32_t w = wave; w < n_probe * v.n_tiles; w += BLOCK / 64) {
    const uint32_t s = w / v.n_tiles, t = w % v.n_tiles;
    const int32_t fp = sk[s];
    if (fp < 0 || (uint32_t)fp >= v.d.R) continue;  // wave uniform
    const Entry e = v.entries[((uint64_t)s * v.d.R + (uint32_t)fp) * v.n_tiles + t];
    const uint16_t *b = v.gids + v.tile_base[t] + ((uint64_t)e.start << v.align_log2);
    for (uint32_t o = lane; o < e.len; o += 64) atomicAdd(&cnt[tile_gid(v, t, b[o]) / kProbeBlock], 1u);
  }
  __syncthreads();
  uint32_t best = 0;  // count << 20 | block
  for (uint32_t i = tid; i < n_blocks; i += BLOCK) {
    const uint32_t c = cnt[i] < 4095u ? cnt[i] : 4095u;
    const uint32_t a = (c << 20) | i;
    best = best > a ? best : a;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t y = __shfl_xor(best, o, 64);
    best = best > y ? best : y;
  }
  if (lane == 0) atomicMax(&s_best, best);
  __syncthreads();
  if (tid == 0) {
    const uint32_t c = s_best >> 20;
    const uint32_t key = c >= 2 ? (s_best & 0xFFFFFu) : 0xFFFFFu;  // unrelated queries: one group at the end
    keys[q] = (key << 12) | q;
  }
}

// keys[0..nq) -> order[0..nq): ascending (key, query index); one workgroup, bitonic in LDS
__global__ __launch_bounds__(1024) void order_kernel(const uint32_t *keys, uint32_t nq, uint32_t *order) {
  __shared__ uint32_t a[kOrderMax];
  const uint32_t tid = threadIdx.x;
  for (uint32_t i = tid; i < kOrderMax; i += 1024) a[i] = i < nq ? keys[i] : 0xFFFFFFFFu;
  __syncthreads();
  for (uint32_t k = 2; k <= kOrderMax; k <<= 1) {
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      for (uint32_t i = tid; i < kOrderMax; i += 1024) {
        const uint32_t l = i ^ j;
        if (l > i) {
          const uint32_t x = a[i], y = a[l];
          const bool up = (i & k) == 0;
          if ((x > y) == up) { a[i] = y; a[l] = x; }
        }
      }
      __syncthreads();
    }
  }
  for (uint32_t i = tid; i < nq; i += 1024) order[i] = a[i] & 0xFFFu;
}

#ifdef NQ_GATHER_CLOCK   // measurement builds only (tools/gather_clock.py): per-workgroup phase times
__device__ unsigned long long *g_gclk;
extern "C" int nq_debug_gather_clock(unsigned long long *buf) { return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_gclk), &buf, sizeof(buf)); }
#define NQ_GCLK(k) do { if (threadIdx.x == 0 && g_gclk) g_gclk[(uint64_t)blockIdx.x * 64 + (k)] = wall_clock64(); } while (0)
#define NQ_GCLK_WAVE(k) do { if ((threadIdx.x & 63u) == 0 && g_gclk) g_gclk[(uint64_t)blockIdx.x * 64 + (k) + (threadIdx.x >> 6)] = wall_clock64(); } while (0)
#else
#define NQ_GCLK(k)
#define NQ_GCLK_WAVE(k)
#endif

// One workgroup per query; the genome tiles are walked one after another with
// the tile's hit counters (packed u16 pairs) in LDS.
// Its barriers order LDS traffic only (lds_barrier): threads never read each other's global writes here,
// and the look-ups already on their way for the next tile must not be waited for.
// NT = -1: every tile's entries come from the look-up pre-pass (`stash` then holds its packed words)
template <int BLOCK, int UNROLL, int NT, bool PAD = false>
__global__ __launch_bounds__(BLOCK) void gather_kernel(IndexView v, const int32_t *sketches,
                                                       uint16_t *counts, uint16_t *counts2, uint64_t stride, Entry *stash,
                                                       const uint32_t *order, uint32_t nq, CandOut co) {
  extern __shared__ __align__(16) uint32_t cnt[];
  uint32_t q = blockIdx.x;
  if (order) {
    // Locality order (see order_queries below): block b runs on XCD b % 8 as the (b / 8)-th
    // workgroup of that XCD; kOrderGroup consecutive entries of the sorted order share an XCD
    // and sit next to each other in its dispatch queue.
    const uint32_t x = blockIdx.x % kXcds, k = blockIdx.x / kXcds;
    const uint32_t i = ((k / kOrderGroup) * kXcds + x) * kOrderGroup + k % kOrderGroup;
    if (i >= nq) return;  // padding block (uniform)
    q = order[i];
  }
  const uint32_t tid = threadIdx.x;
  NQ_GCLK(0);
#ifdef NQ_GATHER_CLOCK
  if (tid == 0 && g_gclk) {
    uint32_t hw, xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    g_gclk[(uint64_t)blockIdx.x * 64 + 15] = ((uint64_t)xcc << 32) | hw;
  }
#endif
  // (PAD: the padded walk addresses the counters from LDS address 0 -- gather_shape checks that this
  // instantiation has no static LDS in front of its dynamic block and otherwise launches the form without PAD)
  const int32_t *sk = NT < 0 ? nullptr : sketches + (uint64_t)q * v.q_stride + v.q_off;
  Item *queue = (Item *)(cnt + (v.tile + 1) / 2 + (PAD ? kPadWords : 0u));  // behind the counters: kQueue items per wave
  const bool want_cand = co.cand != nullptr;
  const bool want_surv = co.surv != nullptr;
  const uint32_t emit_thr = want_surv ? co.surv_thr : co.thr;   // surv_thr <= thr
  // List lengths of this query: only this workgroup appends to them during the launch, so they are counted
  // in LDS (same-address global atomics serialise in L2: ~45 entries per tile cost 5 us) and written back once.
  // The two words are wave 0's queue head, idle between two walks (the LDS is full: kPadMaxTile): thread 0
  // parks the running totals there before the barrier that ends a walk and takes them back after the scan.
  uint32_t *lds_n = (uint32_t *)queue;
  uint32_t n_surv = 0, n_cand = 0;
  if (co.hl_over && blockIdx.x == 0 && tid == 0) co.hl_over[0] = 0u;   // the scan that follows counts the overflowing lists here
  if (want_cand && tid == 0) {
    n_cand = (uint32_t)co.n[q];
    if (want_surv) n_surv = (uint32_t)co.surv_n[q];
  }
  auto emit = [&](uint32_t c, uint32_t col) {   // col: column of the row = genome id - g_base
    if (c >= emit_thr) {
      if (want_surv) {
        const uint32_t i = atomicAdd(&lds_n[0], 1u);
        if (i < co.surv_cap) co.surv[(uint64_t)q * co.surv_cap + i] = make_int2((int)(v.g_base + col), (int)c);
      }
      if (c >= co.thr) {
        const uint32_t i = atomicAdd(&lds_n[1], 1u);
        if (i < co.cap) co.cand[(uint64_t)q * co.cap + i] = (int32_t)(v.g_base + col);
      }
    }
  };
  uint32_t t_emit = 0;   // the tile being scanned / written out
  // The eight counters of a quad (words 4k .. 4k+3 of tile t) at once: ONE LDS atomic per list claims the places
  // of all its entries, then the lane stores them.  (Survivors come in runs -- the genomes of a family sit next
  // to each other -- and one atomic per entry made a lane with eight of them wait eight LDS round trips.)
  auto emit_quad = [&](const uint4 &c, uint32_t k, uint32_t n_t) {
    const uint32_t o = c.x | c.y | c.z | c.w;
    if ((o & 0xFFFFu) < emit_thr && (o >> 16) < emit_thr) return;   // no half of the quad can reach the threshold
    const uint32_t cw[4] = {c.x, c.y, c.z, c.w};
    uint32_t ms = 0, mc = 0;   // halves that go to the survivor / candidate list
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const uint32_t h = (i & 1) ? cw[i >> 1] >> 16 : cw[i >> 1] & 0xFFFFu;
      const bool in = 8 * k + i < n_t;
      ms |= (uint32_t)(in && h >= emit_thr) << i;
      mc |= (uint32_t)(in && h >= co.thr) << i;
    }
    uint32_t bs = 0, bc = 0;
    if (want_surv && ms) bs = atomicAdd(&lds_n[0], (uint32_t)__builtin_popcount(ms));
    if (mc) bc = atomicAdd(&lds_n[1], (uint32_t)__builtin_popcount(mc));
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const uint32_t h = (i & 1) ? cw[i >> 1] >> 16 : cw[i >> 1] & 0xFFFFu;
      const uint32_t gid = v.g_base + tile_gid(v, t_emit, 8 * k + i);
      if (want_surv && (ms >> i & 1u)) {
        if (bs < co.surv_cap) co.surv[(uint64_t)q * co.surv_cap + bs] = make_int2((int)gid, (int)h);
        ++bs;
      }
      if (mc >> i & 1u) {
        if (bc < co.cap) co.cand[(uint64_t)q * co.cap + bc] = (int32_t)gid;
        ++bc;
      }
    }
  };
  const uint32_t n_it_all = (v.f_local + 63) / 64, it_pass = kPassSlots / 64;
  for (uint32_t it_lo = 0; it_lo < n_it_all; it_lo += it_pass) {   // one pass unless f_local > 2^15 (S = 16)
  const uint32_t n_it = it_lo + it_pass < n_it_all ? it_lo + it_pass : n_it_all;
  uint16_t *plane = it_lo ? counts2 : counts;
  Entry ahead[2];
  if constexpr (NT < 0) {   // the first tile's first look-ups (walk_tile keeps `ahead` one tile ahead from here on)
    const uint32_t *p0 = (const uint32_t *)stash + (uint64_t)q * v.n_tiles * v.f_local;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      uint32_t s = (it_lo + (tid >> 6) + k * (BLOCK / 64)) * 64 + (tid & 63u);
      if (s >= v.f_local) s = v.f_local - 1;
      const uint32_t w = p0[s];
      ahead[k] = Entry{v.slot_units[s] + (w >> 16), w & 0xFFFFu};
    }
  }
  bool zeroed = false;   // the scan of the tile before left this tile's counters at zero
  uint32_t hl_total = 0;  // hit lists: the query's hits in the tiles before this one (the same in every thread)
  for (uint32_t t = 0; t < v.n_tiles; ++t) {
    const uint32_t n_t = tile_count(v, t);
    const uint32_t n_words = (n_t + 1) / 2;
    t_emit = t;
    if (!zeroed) {
      uint4 *c4 = (uint4 *)cnt;   // (the dynamic LDS block is 16-byte aligned)
      for (uint32_t i = tid; i < n_words / 4; i += BLOCK) c4[i] = make_uint4(0, 0, 0, 0);
      for (uint32_t i = (n_words & ~3u) + tid; i < n_words; i += BLOCK) cnt[i] = 0;
      if (co.hl && t == 0)   // (the list gathers the hits of every tile)
        for (uint32_t i = tid; i < co.hl_cap; i += BLOCK) ((unsigned long long *)(queue + (BLOCK / 64) * kQueue))[i] = 0ull;
      lds_barrier();
    }
    zeroed = false;
    NQ_GCLK(1 + 4 * (t & 1));
    if constexpr (NT < 0) {
      walk_tile<BLOCK, UNROLL, 1, false, false, true, PAD>(v, sk, q, t, cnt, queue, nullptr, it_lo, n_it, (const uint32_t *)stash, ahead);
    } else if constexpr (NT >= 2) {
      if (t == 0) walk_tile<BLOCK, UNROLL, NT, true, false, false, PAD>(v, sk, q, t, cnt, queue, stash, it_lo, n_it);
      else walk_tile<BLOCK, UNROLL, NT, false, true, false, PAD>(v, sk, q, t, cnt, queue, stash, it_lo, n_it);
    } else {
      walk_tile<BLOCK, UNROLL, 1, false, false, false, PAD>(v, sk, q, t, cnt, queue, stash, it_lo, n_it);
    }
    if (want_cand && tid == 0) { lds_n[0] = n_surv; lds_n[1] = n_cand; }
    if (co.hl && tid == 0) lds_n[0] = hl_total;
    NQ_GCLK_WAVE(16 + 16 * (t & 1));
    NQ_GCLK(2 + 4 * (t & 1));
    lds_barrier();
    NQ_GCLK(3 + 4 * (t & 1));
    if (plane == nullptr) {
      // no counter row (survivor output only): the tile's counters are scanned where they are
      // ... and left at zero for the next tile (whose counters are no more than this one's)
      zeroed = t + 1 < v.n_tiles && tile_count(v, t + 1) <= n_t;
      // 16 bytes per LDS access, four accesses in flight per thread; a quad whose OR-ed halves stay under
      // the threshold holds no survivor
      uint4 *c4 = (uint4 *)cnt;
      const uint32_t n_quads = n_words / 4;
      auto word = [&](uint32_t c, uint32_t w) {
        if ((c & 0xFFFFu) >= emit_thr) emit(c & 0xFFFFu, tile_gid(v, t, 2 * w));
        if (2 * w + 1 < n_t && (c >> 16) >= emit_thr) emit(c >> 16, tile_gid(v, t, 2 * w + 1));
      };
      for (uint32_t k0 = tid; k0 < n_quads; k0 += 4 * BLOCK) {
        uint4 c[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const uint32_t k = k0 + j * BLOCK;
          c[j] = k < n_quads ? c4[k] : make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const uint32_t k = k0 + j * BLOCK;
          if (zeroed && k < n_quads) c4[k] = make_uint4(0, 0, 0, 0);
          emit_quad(c[j], k, n_t);
        }
      }
      for (uint32_t w = 4 * n_quads + tid; w < n_words; w += BLOCK) {
        const uint32_t c = cnt[w];
        if (zeroed) cnt[w] = 0;
        word(c, w);
      }
      lds_barrier();
      if (tid == 0) { n_surv = lds_n[0]; n_cand = lds_n[1]; }
      NQ_GCLK(4 + 4 * (t & 1));
      continue;
    }
    if (co.hl) {
      // Hit lists (launch_gather: one plane, one segment, nothing to add to): the query's hits are picked while a tile's
      // counters are in LDS -- count >= min_score, src/niqki_index.cpp:662-666 -- into one LDS list for all tiles, and
      // ordered after the last tile, by rank: the keys count << 32 | gid are distinct, so an entry's place under
      // greater<pair<count, gid>> (:685) is the number of entries with a larger key.  The key holds the global gid (the
      // genomes of striped tiles interleave).  A query with a few dozen hits writes no 2N-byte counter row and reads
      // none again.  A query with more than hl_cap hits (min_score 0: every genome) leaves through its counter row as
      // before, and launch_hitlist_emit orders it.  Its total may pass hl_cap only at a later tile: that tile first
      // writes the row's other tiles -- zeros, then the hits of the tiles before, which the list holds in full -- and it
      // and every tile after it write their counters there as the counter-row form does (below).
      unsigned long long *list = (unsigned long long *)(queue + (BLOCK / 64) * kQueue);   // hl_cap keys
      const uint32_t cap = co.hl_cap, ms = co.hl_min;
      // (hits are few: an LDS atomic each; ballot ranking was slower.  The counters are read eight at a time -- the
      // workgroup's clock showed 2.7 of a read's 14.6 us in this scan when it took them word by word -- and a quad
      // whose OR-ed halves stay under the threshold holds no hit)
      auto pick = [&](uint32_t c, uint32_t i) {
        const uint32_t lo = c & 0xFFFFu, hi = c >> 16;
        if (lo >= ms) {
          const uint32_t at = atomicAdd(&lds_n[0], 1u);
          if (at < cap) list[at] = (unsigned long long)lo << 32 | (v.g_base + tile_gid(v, t, 2 * i));
        }
        if (2 * i + 1 < n_t && hi >= ms) {
          const uint32_t at = atomicAdd(&lds_n[0], 1u);
          if (at < cap) list[at] = (unsigned long long)hi << 32 | (v.g_base + tile_gid(v, t, 2 * i + 1));
        }
      };
      const uint32_t n_quads = n_words / 4;
      const uint4 *c4 = (const uint4 *)cnt;   // (the dynamic LDS block is 16-byte aligned)
      for (uint32_t k = tid; k < n_quads; k += BLOCK) {
        const uint4 c = c4[k];
        const uint32_t o = c.x | c.y | c.z | c.w;
        if ((o & 0xFFFFu) < ms && (o >> 16) < ms) continue;
        pick(c.x, 4 * k); pick(c.y, 4 * k + 1); pick(c.z, 4 * k + 2); pick(c.w, 4 * k + 3);
      }
      for (uint32_t i = 4 * n_quads + tid; i < n_words; i += BLOCK) pick(cnt[i], i);
      lds_barrier();
      const uint32_t total = lds_n[0];   // (hl_total: the same in every thread)
      if (total > cap && hl_total <= cap && t > 0) {
        uint16_t *row = plane + (uint64_t)q * stride + v.g_base;
        if (((uintptr_t)row & 3u) == 0) {
          for (uint32_t i = tid; i < v.n_genomes / 2; i += BLOCK) ((uint32_t *)row)[i] = 0u;
          if ((v.n_genomes & 1u) && tid == 0) row[v.n_genomes - 1] = 0;
        } else {
          for (uint32_t i = tid; i < v.n_genomes; i += BLOCK) row[i] = 0;
        }
        __syncthreads();   // (a barrier that waits for the zeros: the counts below are stored over them)
        for (uint32_t i = tid; i < hl_total; i += BLOCK) {
          const unsigned long long e = list[i];
          row[(uint32_t)e - v.g_base] = (uint16_t)(e >> 32);
        }
      }
      if (t + 1 == v.n_tiles) {
        if (total <= cap) {
          // (entries are read two at a time; the list was zeroed before the first tile, and key 0 -- the places
          // behind the last entry -- is larger than no key: a real key 0 is count 0 of genome 0, the smallest there is)
          const uint32_t t2 = (total + 1u) & ~1u;
          unsigned long long *out = co.hl + (uint64_t)q * cap;
          for (uint32_t i = tid; i < total; i += BLOCK) {
            const unsigned long long key = list[i];
            uint32_t rank = 0;
            for (uint32_t j = 0; j < t2; j += 2) {   // (all lanes read the same two entries: a broadcast)
              const ulonglong2 o = *(const ulonglong2 *)(list + j);
              rank += (o.x > key) + (o.y > key);
            }
            out[rank] = key;
          }
        }
        if (tid == 0) co.hl_n[q] = total;
      }
      hl_total = total;
      if (total <= cap) {
        lds_barrier();   // (everyone has read lds_n before the next walk takes its words back)
        NQ_GCLK(4 + 4 * (t & 1));
        continue;
      }
    }
    uint16_t *row = plane + (uint64_t)q * stride + v.g_base;
    if (v.stripe > 1 && v.n_tiles > 1 && ((uintptr_t)row & 3u) == 0) {
      // tiles striped in blocks of an even number of genomes: local ids 2w, 2w + 1 are neighbours in
      // the row, a wave writes whole blocks (64-byte blocks are what HBM takes without a
      // read-modify-write, tools/ubench_partial_write.hip)
      // blocks of >= 8 genomes on 16-byte aligned rows: 8 counters (4 words) per lane and store
      const uint32_t quads = (v.stripe % 8u == 0 && ((uintptr_t)row & 15u) == 0 && !v.accumulate) ? n_t / 8 : 0u;
      for (uint32_t k = tid; k < quads; k += BLOCK) {
        const uint32_t col = tile_gid(v, t, 8 * k);
        const uint4 c = *(const uint4 *)(cnt + 4 * k);
        *(uint4 *)(row + col) = c;
        if (want_cand) emit_quad(c, k, n_t);
      }
      for (uint32_t w = 4 * quads + tid; w < n_words; w += BLOCK) {
        const uint32_t col = tile_gid(v, t, 2 * w), c = cnt[w];
        uint32_t *dst = (uint32_t *)(row + col);
        if (2 * w + 1 < n_t) *dst = v.accumulate ? *dst + c : c;
        else { uint16_t *d = (uint16_t *)dst; *d = v.accumulate ? (uint16_t)(*d + c) : (uint16_t)c; }
        if (want_cand) {
          emit(c & 0xFFFFu, col);
          if (2 * w + 1 < n_t) emit(c >> 16, col + 1);
        }
      }
    } else if (v.stripe && v.n_tiles > 1) {
      // striped tiles: the tile's i-th counter belongs to genome tile_gid(t, i)
      for (uint32_t i = tid; i < n_t; i += BLOCK) {
        const uint16_t c = (uint16_t)(cnt[i >> 1] >> ((i & 1u) * 16u));
        uint16_t *dst = row + tile_gid(v, t, i);
        *dst = v.accumulate ? (uint16_t)(*dst + c) : c;
        if (want_cand) emit(c, tile_gid(v, t, i));
      }
    } else {
      // dense counter row of this tile: u16 counts[q*stride + g0 + i], written as the packed words
      const uint32_t g0 = t * v.tile;
      // (packed words need an even first column: odd g_base or g0 -> element-wise)
      const bool packed = ((v.g_base + g0) & 1u) == 0;
      uint32_t *out = (uint32_t *)(row + g0);
      const uint32_t full = packed ? n_t / 2 : 0;
      if (!packed)
        for (uint32_t i = tid; i < n_t; i += BLOCK) {
          const uint16_t c = (uint16_t)(cnt[i >> 1] >> ((i & 1u) * 16u));
          row[g0 + i] = v.accumulate ? (uint16_t)(row[g0 + i] + c) : c;
          if (want_cand) emit(c, g0 + i);
        }
      // (accumulating: sums stay <= F <= 2^15 per half, so the packed add cannot carry)
      for (uint32_t i = tid; i < full; i += BLOCK) {
        const uint32_t c = cnt[i];
        out[i] = v.accumulate ? out[i] + c : c;
        if (want_cand) { emit(c & 0xFFFFu, g0 + 2 * i); emit(c >> 16, g0 + 2 * i + 1); }
      }
      if (packed && (n_t & 1u) && tid == 0) {
        const uint16_t c = (uint16_t)(cnt[full] & 0xFFFFu);
        row[g0 + n_t - 1] = v.accumulate ? (uint16_t)(row[g0 + n_t - 1] + c) : c;
        if (want_cand) emit(c, g0 + n_t - 1);
      }
    }
    lds_barrier();
    if (want_cand && tid == 0) { n_surv = lds_n[0]; n_cand = lds_n[1]; }
    NQ_GCLK(4 + 4 * (t & 1));
  }
  }
  if (want_cand && tid == 0) {
    co.n[q] = (int32_t)n_cand;
    if (want_surv) co.surv_n[q] = (int32_t)n_surv;
  }
}

hipError_t launch_order(const IndexView &v, const int32_t *sketches, uint32_t nq, uint32_t *keys,
                        uint32_t *order, hipStream_t stream) {
  if (nq == 0 || nq > kOrderMax || v.n_genomes >= (1u << 20) - 1) return hipErrorInvalidValue;
  const size_t lds = (size_t)((v.n_genomes + kProbeBlock - 1) / kProbeBlock) * 4;   // <= 64 KB (n_genomes < 2^20)
  hipError_t e = hipFuncSetAttribute((const void *)probe_kernel<256>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(probe_kernel<256>, dim3(nq), dim3(256), lds, stream, v, sketches, keys);
  hipLaunchKernelGGL(order_kernel, dim3(1), dim3(1024), 0, stream, keys, nq, order);
  return hipGetLastError();
}

bool gather_variant_valid(int variant) {
  return variant >= 0 && variant <= 5;
}

GatherShape gather_shape(const IndexView &v, int variant, bool pre) {
  // The padded walk (PAD = true) takes a counter's LDS address from the genome id alone: the kernel's dynamic
  // LDS must start at LDS address 0, i.e. the instantiation must have no static LDS in front of it.  Asked of
  // the runtime once per process; if a toolchain ever puts something there, the form with explicit lengths
  // (any LDS base, any index layout) is launched instead.
  static const bool pad_at_zero = [] {
    hipFuncAttributes fa{};
    return hipFuncGetAttributes(&fa, (const void *)gather_kernel<1024, 32, -1, true>) == hipSuccess && fa.sharedSizeBytes == 0 &&
           hipFuncGetAttributes(&fa, (const void *)gather_kernel<1024, 16, 2, true>) == hipSuccess && fa.sharedSizeBytes == 0;
  }();
  const bool padded = v.padded && pad_at_zero;
  // look-ups from the pre-pass: one form for any tile count; else the stash forms for 2..4 tiles
  const int nt = pre ? -1 : (v.n_tiles >= 2 && v.n_tiles <= 4 ? (int)v.n_tiles : 1);
  switch (variant) {
    case 1: return GatherShape{1024, 8, nt, padded};
    case 2: return GatherShape{1024, 32, nt, padded};
    case 3: return GatherShape{512, 16, nt, false};
    case 4: return GatherShape{256, 16, nt, false};
    case 5: return GatherShape{128, 16, nt, false};
    default: break;
  }
  // small tiles (short-read indexes): counters of <= 24 KB leave room for several
  // workgroups per CU, and 4 waves per query then beat 16 (tools/bench_reads.py)
  if (v.tile <= 12288) return GatherShape{256, 16, nt, false};
  if (padded && pre) return GatherShape{1024, 32, nt, true};   // without look-ups of its own the walk gains from 32 lines per round trip (8.42 against 8.6 ms)
  return GatherShape{1024, 16, nt, padded};   // padded index: mask-free bucket walk
}

hipError_t launch_gather(const IndexView &v, const int32_t *sketches, uint32_t nq, uint16_t *counts, uint16_t *counts2,
                         uint64_t stride, Entry *stash, const uint32_t *order, int variant, bool pre,
                         hipStream_t stream, const CandOut &co) {
  if (nq == 0 || v.n_tiles == 0) return hipSuccess;
  if (v.f_local > kPassSlots && (!counts2 || v.accumulate)) return hipErrorInvalidValue;
  if (co.cand && (v.accumulate || v.f_local > kPassSlots || !co.n)) return hipErrorInvalidValue;
  if (co.surv && (!co.cand || !co.surv_n || co.surv_thr > co.thr || !co.surv_cap)) return hipErrorInvalidValue;
  if (!counts && !co.surv) return hipErrorInvalidValue;
  if (co.hl && (co.cand || !co.hl_n || !counts || !co.hl_cap || (co.hl_cap & 3u) || co.hl_cap > kHitListMaxCap || v.accumulate ||
                v.f_local > kPassSlots || hit_list_lds(v.tile, co.hl_cap) > kGatherMaxLds))
    return hipErrorInvalidValue;
#define NQ_GATHER_LDS(B) ((size_t)((v.tile + 1) / 2 + (v.padded ? kPadWords : 0u)) * 4 + (size_t)(B / 64) * kQueue * sizeof(Item) + (size_t)co.hl_cap * (co.hl ? 8 : 0))
  // with a locality order the grid is padded to whole groups on every XCD
  const uint32_t per_round = kXcds * kOrderGroup;
  dim3 grid(order ? (nq + per_round - 1) / per_round * per_round : nq);
  hipError_t e;
#define NQ_LAUNCH_GATHER(B, U, NT, ...)                                                          \
  do {                                                                                           \
    auto k = gather_kernel<B, U, NT, ##__VA_ARGS__>;                                             \
    const size_t lds = NQ_GATHER_LDS(B);                                                         \
    e = hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
    if (e != hipSuccess) return e;                                                               \
    hipLaunchKernelGGL(k, grid, dim3(B), lds, stream, v, sketches, counts, counts2, stride, stash, order, nq, co); \
  } while (0)
  const GatherShape sh = gather_shape(v, variant, pre);
#define NQ_BY_TILES(B, U, ...)                                                                   \
  do {                                                                                           \
    if (sh.nt < 0) NQ_LAUNCH_GATHER(B, U, -1, ##__VA_ARGS__);                                     \
    else if (sh.nt == 2) NQ_LAUNCH_GATHER(B, U, 2, ##__VA_ARGS__);                               \
    else if (sh.nt == 3) NQ_LAUNCH_GATHER(B, U, 3, ##__VA_ARGS__);                               \
    else if (sh.nt == 4) NQ_LAUNCH_GATHER(B, U, 4, ##__VA_ARGS__);                               \
    else NQ_LAUNCH_GATHER(B, U, 1, ##__VA_ARGS__);                                               \
  } while (0)
#define NQ_BY_PAD(B, U)                                                                          \
  do {                                                                                           \
    if (sh.pad) NQ_BY_TILES(B, U, true); else NQ_BY_TILES(B, U);                                 \
  } while (0)
  if (sh.block == 1024 && sh.unroll == 8) NQ_BY_PAD(1024, 8);
  else if (sh.block == 1024 && sh.unroll == 16) NQ_BY_PAD(1024, 16);
  else if (sh.block == 1024 && sh.unroll == 32) NQ_BY_PAD(1024, 32);
  else if (sh.block == 512 && sh.unroll == 16 && !sh.pad) NQ_BY_TILES(512, 16);
  else if (sh.block == 256 && sh.unroll == 16 && !sh.pad) NQ_BY_TILES(256, 16);
  else if (sh.block == 128 && sh.unroll == 16 && !sh.pad) NQ_BY_TILES(128, 16);
  else return hipErrorInvalidValue;   // (gather_shape names an instantiation this file does not have)
#undef NQ_BY_PAD
#undef NQ_BY_TILES
#undef NQ_GATHER_LDS
#undef NQ_LAUNCH_GATHER
  return hipGetLastError();
}

// Sum of touched bucket lengths per query (T of the roofline formula).
__global__ __launch_bounds__(256) void gathered_kernel(IndexView v, const int32_t *sketches,
                                                      unsigned long long *per_query) {
  const uint32_t q = blockIdx.x;
  const uint32_t R = v.d.R;
  const int32_t *sk = sketches + (uint64_t)q * v.q_stride + v.q_off;
  unsigned long long sum = 0;
  for (uint32_t s = threadIdx.x; s < v.f_local; s += blockDim.x) {
    int32_t fp = sk[s];
    if (fp >= 0 && (uint32_t)fp < R) {
      const Entry *p = v.entries + ((uint64_t)s * R + (uint32_t)fp) * v.n_tiles;
      for (uint32_t t = 0; t < v.n_tiles; ++t) sum += p[t].len;
    }
  }
  atomicAdd(&per_query[q], sum);
}

hipError_t launch_gathered(const IndexView &v, const int32_t *sketches, uint32_t nq,
                           unsigned long long *per_query, hipStream_t stream) {
  if (nq == 0) return hipSuccess;
  hipLaunchKernelGGL(gathered_kernel, dim3(nq), dim3(256), 0, stream, v, sketches, per_query);
  return hipGetLastError();
}

}  // namespace nq
