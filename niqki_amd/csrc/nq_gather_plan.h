// nq_gather_plan.h -- which kernels a query launch takes, as a value (counts_segment, nq_api_query.hip).
//
// A counter call over one index segment is planned once, from facts of the segment's view, the handle's options and
// the call: whether the look-up pre-pass runs and from which copy of the table, whether each launch gets a locality
// order, how many queries a launch takes, the scratch it needs and the gather_kernel instantiation.  counts_segment
// computes the plan, prepares what it names and loops over the launches; per launch it asks lookup_form and order_form
// and hands their answers to launch_lookup (nq_lookup.hip), launch_order (nq_order.hip) and launch_gather
// (nq_gather.hip), which only carry them out.
//
// Host only, plain C++17: the kernels include this file for the constants they share with the rule,
// tests/test_gather_plan_cpu.py compiles it with g++ and pins the rule row by row.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "nq_common.h"

namespace nq {

// ---- constants that the rule and the kernels share ----
// gather_kernel (nq_gather.hip)
constexpr uint32_t kPassSlots = 32768;    // slots per pass over a view: more (S = 16 on a whole-range handle) take two counter planes
constexpr uint32_t kPadWords = 64;        // dummy counter words of a padded tile
constexpr uint32_t kPadMaxTile = 65408;   // tile + 2 * 63 must fit 16 bits
constexpr uint32_t kQueue = 256;          // items per wave-private LDS work queue
constexpr uint32_t kItemBytes = 8;        // ... of {pos, len}
constexpr uint32_t kEntryBytes = 8;       // a table entry {start, len}: what the stash keeps per (query, extra tile, slot)
// the 256-thread launch shape's largest tile (counters + queues + list within a CU's LDS several times over): an index
// of at most this many genomes takes the hit-list form as one tile
constexpr uint32_t kHitListMaxTile = 12288;
constexpr uint32_t kHitListMaxCap = 2048;
constexpr size_t kGatherMaxLds = 163840;
// look-up pre-pass (nq_lookup.hip)
constexpr uint32_t kXcds = 8;
constexpr uint32_t kPreBlock = 256;                   // lookup_kernel: queries per workgroup, one per thread
constexpr uint32_t kRowSlots = 32, kRowBlock = 1024;  // lookup_rows_kernel: slots x queries per workgroup
constexpr uint32_t kRowMaxBytes = 32768;              // ... and the packed row of a tile group that its LDS buffers hold
// locality order (nq_order.hip)
constexpr uint32_t kOrderGroup = 8;
constexpr uint32_t kOrderMax = 4096;   // queries per launch (12 index bits next to a 20-bit key)
constexpr uint32_t kOrderMaxGenomes = (1u << 20) - 1;   // ... and the key: a block of genomes below this, the value itself "unrelated"

// ---- the numbers at which the rule changes ----
constexpr uint32_t kPreMinQueries = 256;        // default pre-pass on more than kStashTiles tiles: from this many queries ("real batches")
constexpr uint32_t kPreRowsMinQueries = 1024;   // default pre-pass in its streamed-rows form (<= kRowGroupTiles tiles): from this many
constexpr uint32_t kStashTiles = 4;             // tiles whose entries one look-up inside the gather kernel can park; also the tiles
                                                // of one lookup_kernel launch
constexpr uint32_t kRowGroupTiles = 2;          // tiles of one lookup_rows_kernel launch (a group of the packed table)
constexpr uint32_t kRowsMinQueries = kRowBlock / 2;   // a launch takes the streamed rows from half a workgroup of queries on
constexpr uint32_t kOrderMinQueries = 64;       // a launch is ordered from this many queries on
constexpr uint32_t kOrderMinGenomes = 16384;    // query_order 1: "large indexes" ...
constexpr uint32_t kOrderMinSlots = 8192;       // ... and no slot shard below this (+4 % at 8192, nothing at 4096)
constexpr uint32_t kChunk = 4096;               // queries per launch wherever a launch has per-query scratch, an order or a pre-pass
constexpr size_t kChunkScratch = (size_t)128 << 20;   // per-query scratch of a launch that may take more than kChunk queries
constexpr size_t kPreMaxBytes = (size_t)8 << 30;      // the pre-pass words of a launch
constexpr uint32_t kPreChunkStep = 256;         // ... a launch cut down to fit them: a multiple of this, and no less
constexpr uint32_t kSmallTile = 12288;          // gather_variant 0: tiles up to here take the 256-thread shape

// ---- inputs ----
// what the rule reads of a segment's IndexView (nq_kernels.h: gather_facts)
struct GatherFacts {
  uint32_t R;           // fingerprint range
  uint32_t f_local, n_tiles, tile, align_log2;
  bool padded;
  uint32_t n_genomes;   // of the segment
};
// ... and of the handle
struct GatherOptions {
  int lookup_prepass;   // -1 = where it wins, 0 = never, 1 = wherever it is usable
  int query_order;      // 0 = never, 1 = large indexes and real batches, 2 = wherever it is possible
  int gather_variant;   // 0 = choose, 1..5 = a launch shape by name
  bool paged;           // resident_bytes != 0: the index is rebuilt page by page
};

// The gather_kernel<BLOCK, UNROLL, NT, PAD> instantiation of a launch.  pad is the form actually launched (the padded
// walk needs its dynamic LDS at address 0).
struct GatherShape {
  int block, unroll, nt;
  bool pad;
};
// stat "last_gather_kernel": BLOCK | UNROLL << 12 | (NT + 1) << 20 | PAD << 24
constexpr uint32_t gather_shape_code(const GatherShape &s) {
  return (uint32_t)s.block | (uint32_t)s.unroll << 12 | (uint32_t)(s.nt + 1) << 20 | (s.pad ? 1u : 0u) << 24;
}
// The instantiations there are: launch_gather (nq_gather.hip) has exactly these and refuses any other shape.
constexpr bool gather_shape_exists(const GatherShape &s) {
  const bool tiles = s.nt == -1 || (s.nt >= 1 && s.nt <= (int)kStashTiles);
  const bool wide = s.block == 1024 && (s.unroll == 8 || s.unroll == 16 || s.unroll == 32);   // with and without PAD
  const bool narrow = (s.block == 512 || s.block == 256 || s.block == 128) && s.unroll == 16 && !s.pad;
  return tiles && (wide || narrow);
}

struct GatherPlan {
  bool pre;            // the look-up pre-pass runs before every launch; the gather kernel reads its packed words
  bool packed_table;   // ... and the packed copy of the table must exist (stat "last_gather_form", bit 1)
  bool ordered;        // launches of at least kOrderMinQueries queries get a locality order
  uint32_t chunk;      // queries per launch
  size_t stash_bytes, pre_bytes, order_bytes;   // scratch to have before the first launch (0: none)
  GatherShape shape;
  size_t lds_bytes;    // dynamic LDS of the shape's kernel
  uint32_t lookup_slots;   // slots per lookup_kernel workgroup (what lookup_form needs of the facts)
};

// ---- look-up pre-pass ----
// slots per lookup_kernel workgroup
inline uint32_t lookup_slots(const GatherFacts &f) { return f.n_tiles <= kRowGroupTiles ? 32u : 16u; }

// Can the pre-pass serve this index?  Whole slot blocks, and both halves of the packed word
// within 16 bits (bucket lengths <= tile, starts relative to the slot <= tile / unit + R units).
inline bool launch_lookup_usable(const GatherFacts &f) {
  if (f.n_tiles < 1 || f.f_local % lookup_slots(f)) return false;
  if (f.tile > 65535u) return false;
  return (uint64_t)(f.tile >> f.align_log2) + f.R + 1 <= 65535u;
}

// The pre-pass reads a packed copy of the table (4 bytes per entry) where its row-staging kernel applies.
// Packed rows that the LDS buffers hold, dealt to 1024 threads in whole 16-byte loads: tiles are taken two at a
// time (rows of 2 R words = 32 KB at W = 12), a last odd tile alone.
inline bool lookup_wants_packed(const GatherFacts &f) {
  if (!launch_lookup_usable(f) || f.f_local % kRowSlots) return false;
  auto row_ok = [&](uint32_t nt) {   // a group's packed row: within 32 KB, whole 16-byte pieces per thread, 1 or 2 of them
    const uint32_t rw = f.R * nt;
    if (rw * 4u > kRowMaxBytes || rw % (4u * kRowBlock)) return false;
    const uint32_t per = rw / (4u * kRowBlock);
    return per == 1 || per == 2;
  };
  if (f.n_tiles >= 2 && !row_ok(2)) return false;
  if ((f.n_tiles & 1u) && !row_ok(1)) return false;
  return true;
}

// the pre-pass words pre[q][tile][slot] of nq queries
inline size_t lookup_pre_bytes(const GatherFacts &f, uint32_t nq) { return (size_t)f.f_local * nq * f.n_tiles * 4; }

// ---- gather kernel ----
// The one formula for gather_kernel's dynamic LDS: the tile's counters (packed u16 pairs; a padded index: its dummy
// words behind them), one queue per wave and, with hit lists, hl_cap 8-byte keys (0: none).
constexpr size_t gather_lds_bytes(uint32_t block, uint32_t tile, bool padded, uint32_t hl_cap) {
  return (size_t)((tile + 1) / 2 + (padded ? kPadWords : 0u)) * 4 + (size_t)(block / 64) * kQueue * kItemBytes + (size_t)hl_cap * 8;
}
// LDS of a gather launch with hit lists at its largest workgroup (1024 threads, a padded tile); the form takes tiles
// where that fits a workgroup's 160 KB
constexpr size_t hit_list_lds(uint32_t tile, uint32_t cap) { return gather_lds_bytes(1024, tile, true, cap); }

// launch shapes selectable through the "gather_variant" option (0 = choose)
inline bool gather_variant_valid(int variant) { return variant >= 0 && variant <= 5; }

// The one place where the shape is chosen.  pad_at_zero: the padded walk (PAD = true) takes a counter's LDS address
// from the genome id alone, so the kernel's dynamic LDS must start at LDS address 0, i.e. the instantiation must have
// no static LDS in front of it.  Asked of the runtime once per process (gather_pad_at_zero, nq_gather.hip); if a
// toolchain ever puts something there, the form with explicit lengths (any LDS base, any index layout) is launched
// instead.
inline GatherShape gather_shape(const GatherFacts &f, int variant, bool pre, bool pad_at_zero) {
  const bool padded = f.padded && pad_at_zero;
  // look-ups from the pre-pass: one form for any tile count; else the stash forms for 2..4 tiles
  const int nt = pre ? -1 : (f.n_tiles >= 2 && f.n_tiles <= kStashTiles ? (int)f.n_tiles : 1);
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
  if (f.tile <= kSmallTile) return GatherShape{256, 16, nt, false};
  if (padded && pre) return GatherShape{1024, 32, nt, true};   // without look-ups of its own the walk gains from 32 lines per round trip (8.42 against 8.6 ms)
  return GatherShape{1024, 16, nt, padded};   // padded index: mask-free bucket walk
}

// ---- the rule ----
// sketches_aligned: the query sketches are 16-byte aligned with a stride that is a multiple of 4 (the pre-pass reads
// them as int4); nq: queries of the call; hl_cap: capacity of the hit lists the launches fill, 0 without them.
inline GatherPlan gather_plan(const GatherFacts &f, const GatherOptions &o, bool sketches_aligned, bool pad_at_zero, uint32_t nq,
                              uint32_t hl_cap) {
  GatherPlan p{};
  p.lookup_slots = lookup_slots(f);
  // Table look-ups: inside the gather kernel (one random table line per query and slot), or
  // by the slot-major pre-pass, which walks the table once per launch for all its queries.
  p.pre = o.lookup_prepass != 0 && launch_lookup_usable(f) && sketches_aligned;
  // Measured at the north-star shape (profiles/r02_*): with random 16-byte look-ups (lookup_kernel) the
  // pre-pass takes 16 % of the HBM traffic off a launch but not its time -- both forms are bound by the
  // number of random line requests a CU keeps in flight, and inside the gather kernel the look-ups
  // overlap with the bucket walk.  The default (-1) therefore takes the pre-pass only where it wins:
  // An index of more than 4 tiles (> 261 632 genomes) is different: inside the kernel only 4 tiles'
  // entries can be parked per look-up, so every further tile would cost its own random table line
  // per query and slot; there the pre-pass is the default for real batches.
  // Up to 2 tiles of W <= 12 the pre-pass has a form that streams whole table rows through LDS from a
  // packed copy of the table (lookup_rows_kernel): 0.75 ms per 4096 queries, the launch 8 % faster than
  // with the look-ups inside the gather kernel -- the default for batches of >= 1024 queries.
  // (not on a paged index: the packed copy would be made again for every page, outside its memory budget)
  if (o.lookup_prepass < 0)
    p.pre = p.pre && ((f.n_tiles > kStashTiles && nq >= kPreMinQueries) ||
                      (lookup_wants_packed(f) && nq >= kPreRowsMinQueries && !o.paged && f.n_tiles <= kRowGroupTiles));
  p.packed_table = p.pre && lookup_wants_packed(f);
  // locality order of each launch: worth its probe on large indexes and real batches.  It takes ~8 % off
  // the gather kernel and costs 0.1 ms per 4096 queries at 100 000 genomes whatever the slot count:
  // measured even on a slot shard of 4096 slots (1.56 against 1.57 ms per 4096 queries), +4 % at 8192.
  p.ordered = o.query_order && nq >= kOrderMinQueries && f.n_genomes < kOrderMaxGenomes &&
              (o.query_order >= 2 || (f.n_genomes >= kOrderMinGenomes && f.f_local >= kOrderMinSlots));
  // launches of at most `chunk` queries: the order kernel sorts <= 4096, and the per-query scratch
  // (stash or pre-pass words) stays <= 128 MiB whatever the caller's batch size is (bigger launches are
  // no faster: 32 768 query shards in one launch take 8 x the time of 4096)
  const size_t per_query = p.pre ? lookup_pre_bytes(f, 1) : (size_t)(f.n_tiles - 1) * f.f_local * kEntryBytes;
  p.chunk = nq;
  if (per_query) p.chunk = (uint32_t)(kChunkScratch / per_query > kChunk ? kChunkScratch / per_query : kChunk);
  if (p.ordered || p.pre) p.chunk = kChunk;
  // (the pre-pass words of a launch: at most 8 GiB -- a launch of 4096 queries on up to 16 tiles at S = 15; the streamed
  // form reads the table once per launch, so fewer, larger launches halve its traffic on a 500 000-genome index)
  if (p.pre && per_query * p.chunk > kPreMaxBytes) {
    const uint32_t fit = (uint32_t)((kPreMaxBytes / per_query) & ~(size_t)(kPreChunkStep - 1));
    p.chunk = fit > kPreChunkStep ? fit : kPreChunkStep;
  }
  const uint32_t first = nq < p.chunk ? nq : p.chunk;   // queries of the largest launch
  if (p.pre) p.pre_bytes = lookup_pre_bytes(f, first);
  else if (f.n_tiles > 1) p.stash_bytes = (size_t)first * (f.n_tiles - 1) * f.f_local * kEntryBytes;
  if (p.ordered) p.order_bytes = (size_t)p.chunk * 8;   // keys and order: chunk words each
  p.shape = gather_shape(f, o.gather_variant, p.pre, pad_at_zero);
  p.lds_bytes = gather_lds_bytes((uint32_t)p.shape.block, f.tile, f.padded, hl_cap);
  return p;
}

// ---- per launch ----
// The pre-pass kernel of a launch of n queries: streamed rows from the packed table, tile groups of two
// (lookup_rows_kernel<NT, PER>), or random look-ups, up to four tiles per launch (lookup_kernel<NT, PS>).
struct LookupForm {
  bool rows;
  uint32_t slots;   // per workgroup: kRowSlots, or PS
  uint32_t step;    // tiles per kernel launch
};
inline LookupForm lookup_form(const GatherPlan &p, uint32_t n) {
  const bool rows = p.packed_table && n >= kRowsMinQueries;
  return LookupForm{rows, rows ? kRowSlots : p.lookup_slots, rows ? kRowGroupTiles : kStashTiles};
}
// ... and its kernel launch that starts at tile t0 (t0 = 0, step, 2 * step, ... below n_tiles) of a table of range R
struct LookupLaunch {
  uint32_t nt;    // tiles it serves
  uint32_t per;   // rows: 16-byte pieces of a packed row per thread (R * NT / 4096); else 0
};
inline LookupLaunch lookup_launch(const LookupForm &f, uint32_t n_tiles, uint32_t R, uint32_t t0) {
  const uint32_t nt = n_tiles - t0 < f.step ? n_tiles - t0 : f.step;
  return LookupLaunch{nt, f.rows ? R * nt / (4u * kRowBlock) : 0u};
}
// The instantiations there are (launch_lookup, nq_lookup.hip): 32 slots serve up to 2 tiles, 16 slots up to 4;
// a packed row is 1 or 2 pieces per thread.
constexpr bool lookup_launch_exists(bool rows, uint32_t slots, uint32_t nt, uint32_t per) {
  return rows ? slots == kRowSlots && (nt == 1 || nt == 2) && (per == 1 || per == 2)
              : (slots == 32 && (nt == 1 || nt == 2)) || (slots == 16 && nt >= 1 && nt <= 4);
}

// Is a launch of n queries ordered, and do probe + order run on a stream of their own beside the pre-pass (both only
// read the sketches)?
struct OrderForm {
  bool ordered, fork;
};
inline OrderForm order_form(const GatherPlan &p, uint32_t n) {
  const bool ordered = p.ordered && n >= kOrderMinQueries;
  return OrderForm{ordered, ordered && p.pre};
}

}  // namespace nq
