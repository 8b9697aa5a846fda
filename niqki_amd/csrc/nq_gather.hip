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
// order_kernel: nq_order.hip): similar queries then run on the same XCD at the same time and
// share their table and bucket lines through its L2.  For real batches the table
// look-ups are taken out of the kernel altogether by a pre-pass (lookup_rows_kernel
// / lookup_kernel: nq_lookup.hip) that walks the table slot block by slot block for all queries of
// the launch; the gather kernel then reads one packed word per (tile, slot).
// Which of these a launch takes, and which gather_kernel instantiation: nq_gather_plan.h; launch_gather carries it out.
#include "nq_gather_ops.h"

namespace nq {

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
static_assert(sizeof(Item) == kItemBytes, "gather_lds_bytes (nq_gather_plan.h) counts the queues of kQueue such items");

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
//   PRE      : entries come from the slot-major look-up pre-pass (nq_lookup.hip): one
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

// Hit lists (launch_gather: one plane, one segment, nothing to add to): the query's hits are picked while a tile's
// counters are in LDS -- count >= min_score, src/niqki_index.cpp:662-666 -- into one LDS list for all tiles, and
// ordered after the last tile, by rank: the keys count << 32 | gid are distinct, so an entry's place under
// greater<pair<count, gid>> (:685) is the number of entries with a larger key.  The key holds the global gid (the
// genomes of striped tiles interleave).  A query with a few dozen hits writes no 2N-byte counter row and reads
// none again.  A query with more than hl_cap hits (min_score 0: every genome) leaves through its counter row as
// before, and launch_hitlist_emit orders it.  Its total may pass hl_cap only at a later tile: that tile first
// writes the row's other tiles -- zeros, then the hits of the tiles before, which the list holds in full -- and it
// and every tile after it write their counters there as the counter-row form does (below).
// list: hl_cap keys in LDS; lds_n[0]: its length so far, the hits of the tiles before, hl_total of them.  Returns the
// list's length with this tile; where that is above hl_cap the caller writes the tile's counters to the row.
template <int BLOCK>
__device__ __forceinline__ uint32_t pick_hits(const IndexView &v, const CandOut &co, uint32_t q, uint32_t t, uint32_t n_t, const uint32_t *cnt,
                                              uint32_t *lds_n, unsigned long long *list, uint16_t *plane, uint64_t stride, uint32_t hl_total) {
  const uint32_t tid = threadIdx.x, n_words = (n_t + 1) / 2;
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
  return total;
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
    // Locality order (nq_order.hip): block b runs on XCD b % 8 as the (b / 8)-th
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
  // (PAD: the padded walk addresses the counters from LDS address 0 -- gather_pad_at_zero checks that this
  // instantiation has no static LDS in front of its dynamic block; gather_shape otherwise names the form without PAD)
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
      // hit lists (pick_hits above); a query over hl_cap goes on to the counter-row forms below
      unsigned long long *list = (unsigned long long *)(queue + (BLOCK / 64) * kQueue);   // hl_cap keys
      const uint32_t cap = co.hl_cap;
      const uint32_t total = pick_hits<BLOCK>(v, co, q, t, n_t, cnt, lds_n, list, plane, stride, hl_total);
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

bool gather_pad_at_zero() {
  static const bool pad_at_zero = [] {
    hipFuncAttributes fa{};
    return hipFuncGetAttributes(&fa, (const void *)gather_kernel<1024, 32, -1, true>) == hipSuccess && fa.sharedSizeBytes == 0 &&
           hipFuncGetAttributes(&fa, (const void *)gather_kernel<1024, 16, 2, true>) == hipSuccess && fa.sharedSizeBytes == 0;
  }();
  return pad_at_zero;
}

namespace {
struct GatherArgs {
  const IndexView &v;
  const int32_t *sketches;
  uint32_t nq;
  uint16_t *counts, *counts2;
  uint64_t stride;
  Entry *stash;
  const uint32_t *order;
  size_t lds;
  hipStream_t stream;
  const CandOut &co;
};
template <int B, int U, int NT, bool PAD>
hipError_t launch_one(const GatherArgs &a) {
  static_assert(gather_shape_exists(GatherShape{B, U, NT, PAD}), "nq_gather_plan.h lists the instantiations");
  auto k = gather_kernel<B, U, NT, PAD>;
  const hipError_t e = hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)a.lds);
  if (e != hipSuccess) return e;
  // with a locality order the grid is padded to whole groups on every XCD
  const uint32_t per_round = kXcds * kOrderGroup;
  const dim3 grid(a.order ? (a.nq + per_round - 1) / per_round * per_round : a.nq);
  hipLaunchKernelGGL(k, grid, dim3(B), a.lds, a.stream, a.v, a.sketches, a.counts, a.counts2, a.stride, a.stash, a.order, a.nq, a.co);
  return hipGetLastError();
}
template <int B, int U, bool PAD>
hipError_t launch_by_tiles(int nt, const GatherArgs &a) {
  switch (nt) {
    case -1: return launch_one<B, U, -1, PAD>(a);
    case 2: return launch_one<B, U, 2, PAD>(a);
    case 3: return launch_one<B, U, 3, PAD>(a);
    case 4: return launch_one<B, U, 4, PAD>(a);
    default: return launch_one<B, U, 1, PAD>(a);
  }
}
template <int U>
hipError_t launch_wide(const GatherShape &sh, const GatherArgs &a) {   // 1024 threads: with and without the padded walk
  return sh.pad ? launch_by_tiles<1024, U, true>(sh.nt, a) : launch_by_tiles<1024, U, false>(sh.nt, a);
}
}  // namespace

hipError_t launch_gather(const IndexView &v, const int32_t *sketches, uint32_t nq, uint16_t *counts, uint16_t *counts2,
                         uint64_t stride, Entry *stash, const uint32_t *order, const GatherShape &sh, size_t lds_bytes,
                         hipStream_t stream, const CandOut &co) {
  if (nq == 0 || v.n_tiles == 0) return hipSuccess;
  if (v.f_local > kPassSlots && (!counts2 || v.accumulate)) return hipErrorInvalidValue;
  if (co.cand && (v.accumulate || v.f_local > kPassSlots || !co.n)) return hipErrorInvalidValue;
  if (co.surv && (!co.cand || !co.surv_n || co.surv_thr > co.thr || !co.surv_cap)) return hipErrorInvalidValue;
  if (!counts && !co.surv) return hipErrorInvalidValue;
  if (co.hl && (co.cand || !co.hl_n || !counts || !co.hl_cap || (co.hl_cap & 3u) || co.hl_cap > kHitListMaxCap || v.accumulate ||
                v.f_local > kPassSlots || hit_list_lds(v.tile, co.hl_cap) > kGatherMaxLds))
    return hipErrorInvalidValue;
  if (!gather_shape_exists(sh)) return hipErrorInvalidValue;
  const GatherArgs a{v, sketches, nq, counts, counts2, stride, stash, order, lds_bytes, stream, co};
  if (sh.block == 1024) return sh.unroll == 8 ? launch_wide<8>(sh, a) : sh.unroll == 16 ? launch_wide<16>(sh, a) : launch_wide<32>(sh, a);
  if (sh.block == 512) return launch_by_tiles<512, 16, false>(sh.nt, a);
  if (sh.block == 256) return launch_by_tiles<256, 16, false>(sh.nt, a);
  return launch_by_tiles<128, 16, false>(sh.nt, a);
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
