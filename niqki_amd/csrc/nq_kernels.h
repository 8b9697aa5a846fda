// nq_kernels.h -- launch interface between the C ABI (nq_api.hip) and the
// gfx950 kernels.  All pointers are device pointers unless noted.
#pragma once
#include "nq_common.h"
#include "nq_gather_plan.h"
#include "nq_retain_blocks.h"
#include "nq_sketch_plan.h"
#include "nq_unite_blocks.h"

namespace nq {

// ---- sketch (nq_sketch.hip, nq_sketch_reads.hip, nq_densify.hip) ------------
// What the sketch kernels receive.  A caller fills its own fields; the four marked "plan" are written by launch_sketch
// from the SketchPlan it carries out.
struct SketchArgs {
  Derived d;
  const uint8_t *seqs;        // record bytes; nullptr = densify-only launch
  const uint64_t *rec_off;    // n_rec+1
  const uint32_t *entry_rec;  // n_entry+1 or nullptr (one record per sketch)
  int32_t *sketches;          // n_entry x F
  uint32_t splits;            // workgroups per sketch (>1: partial mins merged in global memory)
  uint32_t halves;            // plan: 2 when the F cells do not fit LDS (S = 16): every workgroup
                              // keeps one half of the slots and sees all k-mers; results merge in global memory
  uint32_t accumulate;        // start from the sketches already in `sketches`
  uint32_t densify;           // run densification before the store (splits == 1 only)
  uint32_t distinct;          // plan: densify over distinct values (short-read path)
  uint32_t filter;            // plan: candidate filter for long inputs
  uint32_t read_entries;      // plan: capacity of the short-read kernel's entry list (192 or 384)
  uint32_t *redo;             // short records: one flag per sketch, or nullptr (then a sketch with more occupied cells than the
                              // one-wavefront kernel's entry list takes the plain pass over all cells)
  uint32_t redo_only;         // != 0: this launch works only on the sketches whose flag has this value
  uint32_t redo_mark;         // != 0 (one-wavefront kernel): a sketch that exceeds the entry list gets this flag and is left
                              // to a later launch -- nothing of it is stored
};
// Carries out a plan (nq_sketch_plan.h) on n_entry sketches: writes the plan's fields of SketchArgs and launches the
// plan's kernel, and densify_distinct_kernel behind it where the plan says so.  A refused plan: hipErrorInvalidValue.
hipError_t launch_sketch(const SketchArgs &a, uint32_t n_entry, const SketchPlan &plan, hipStream_t stream);
// NIQKI_SKETCH_WAVE and NIQKI_SKETCH_FILTER as they are now (read per call: tests change them between engines of one process)
SketchSwitches sketch_switches();
hipError_t launch_fill_u32(uint32_t *p, uint64_t n, uint32_t v, hipStream_t stream);
// the kernels of the other units, launched by launch_sketch with the arguments it has completed
hipError_t launch_sketch_reads(const SketchArgs &a, uint32_t n_entry, size_t lds, hipStream_t stream);        // nq_sketch_reads.hip
hipError_t launch_densify_distinct(const SketchArgs &a, uint32_t n_entry, size_t lds, hipStream_t stream);   // nq_densify.hip
hipError_t launch_densify_global(const SketchArgs &a, uint32_t n_entry, hipStream_t stream);

// ---- sketch store + inverted index (nq_index.hip) ---------------------------
// Sketch store: u16 [F_local][cap], slot major; 0xFFFF = empty/invalid cell.
// Inverted index over genome tiles (tile t = genomes [t*T, min((t+1)*T, N)), or, striped,
// the genomes g with g % n_tiles == t in ascending order):
//   entries  Entry [F_local][R][n_tiles]   bucket (slot, fp) of every tile side by
//                                          side, so ONE lookup serves all tiles
//   gids     u16, tile t at gids + tile_base[t]; a bucket starts at
//            (entry.start << align_log2) inside its tile and holds entry.len
//            tile-local genome ids, ascending.  With align_log2 = 6 every bucket
//            starts on a 128-byte line.
struct Entry {
  uint32_t start;  // in units of (1 << align_log2) ids
  uint32_t len;
};
static_assert(sizeof(Entry) == kEntryBytes, "the stash bytes of a GatherPlan (nq_gather_plan.h) count these");
struct IndexView {
  Derived d;
  uint32_t n_genomes;   // genomes of this segment
  uint32_t g_base;      // ... which are genomes [g_base, g_base + n_genomes) of the store / of the counter rows
                        // (0 for the main index; the delta segment of genomes inserted after the last full build)
  uint32_t tile;     // T, genomes per tile (multiple of 64, <= 65536)
  uint32_t n_tiles;
  uint32_t f_local;  // slot_end - slot_begin
  uint32_t align_log2;
  uint32_t padded;   // 128-byte aligned buckets whose unused tail positions hold padding ids: position p of
                     // a line holds id tile + 2p, which the gather kernel counts into 64 dummy words behind
                     // the tile's counters -- its bucket walk then needs no per-lane length test.  Every
                     // tile's id array ends with one line of padding only (the walk's "no chunk").
  uint32_t stripe;   // 0: tiles are ranges.  B = 1, 2, 4 .. 64: blocks of B consecutive genomes are dealt to the
                     // tiles round-robin (tile = (gid / B) % n_tiles): a run of related genomes is spread over
                     // all tiles, which keeps their buckets short in every tile
  uint64_t cap;      // row stride of the sketch store (genomes)
  const uint16_t *store;
  // query sketches handed to the query kernels: row q starts at sketches + q * q_stride, this
  // shard's first slot at + q_off (whole sketches: F and slot_begin; slot slices: f_local and 0)
  uint32_t q_stride, q_off;
  uint32_t accumulate;   // gather: add to the counter rows instead of overwriting them (slot pages after the first)
  const Entry *entries;
  const uint16_t *gids;
  const uint64_t *tile_base;   // n_tiles+1 (in ids), device
  const uint32_t *slot_units;  // n_tiles x (f_local+1): units before slot s of tile t
  const uint32_t *ptab = nullptr;   // [F_local][R][n_tiles] (start - first unit of the slot) << 16 | len, or nullptr
  // Single-tile indexes: bit c of hmask[s] = some bucket (s, fp) with fp >> hmask_shift == c is not empty
  // (hmask_shift = max(W - 4, 0): sixteen classes of the fingerprint range; with the regular H = 4 form a class
  // is a HyperLogLog part).  The gather kernel's own look-up tests it before it touches the table: a short
  // read's fingerprints (few leading zeros) fall into classes no indexed genome's minimum ever has, so a read
  // against a genome index skips ~99 % of its 2^S random table lines.  nullptr = no mask (look everything up).
  const uint16_t *hmask = nullptr;
  uint32_t hmask_shift = 0;
};
hipError_t launch_hmask(const IndexView &v, uint16_t *hmask, hipStream_t stream);

// genomes of tile t / global id of its i-th genome
NQ_HD uint32_t tile_count(const IndexView &v, uint32_t t) {
  if (v.stripe) {  // blocks of `stripe` genomes dealt round-robin
    const uint32_t nb = v.n_genomes / v.stripe, r = v.n_genomes % v.stripe;
    return (nb / v.n_tiles) * v.stripe + (t < nb % v.n_tiles ? v.stripe : 0u) + (t == nb % v.n_tiles ? r : 0u);
  }
  const uint32_t g0 = t * v.tile;
  return (v.n_genomes - g0) < v.tile ? (v.n_genomes - g0) : v.tile;
}
NQ_HD uint32_t tile_gid(const IndexView &v, uint32_t t, uint32_t i) {
  if (!v.stripe) return t * v.tile + i;
  const uint32_t sh = (uint32_t)__builtin_ctz(v.stripe);   // a power of two
  return (((i >> sh) * v.n_tiles + t) << sh) + (i & (v.stripe - 1u));
}

// sk_stride / sk_off: as q_stride / q_off of IndexView
hipError_t launch_store_insert(const Derived &d, const int32_t *sketches, uint32_t sk_stride, uint32_t sk_off,
                               uint32_t n, uint16_t *store, uint64_t cap, uint32_t first_gid,
                               hipStream_t stream);
hipError_t launch_store_read(const Derived &d, const uint16_t *store, uint64_t cap,
                             uint32_t begin, uint32_t n, int32_t *sketches, hipStream_t stream);
// niqki_retain (nq_retain_blocks.h: blocks of kRetainBlock source columns).  Rank pass: keep[n] flags (nonzero = stays)
// -> words (kRetainWords per block: its keep bits), blk_dst (n_blocks + 1: each block's first destination column, then
// the kept total) and, where new_ids is not null, every genome's new id (0xFFFFFFFF: dropped).
hipError_t launch_retain_ranks(const uint8_t *keep, uint32_t n, unsigned long long *words, uint32_t *blk_dst, uint32_t *new_ids,
                               hipStream_t stream);
// ... then the kept columns of the n_src columns of every row, in order, to the front of ANOTHER store (dst_cap >= the
// kept total; both capacities multiples of 8 columns, both stores 16-byte aligned)
hipError_t launch_store_compact(const uint16_t *src, uint64_t src_cap, uint32_t n_src, uint16_t *dst, uint64_t dst_cap,
                                uint32_t f_local, const unsigned long long *words, const uint32_t *blk_dst, hipStream_t stream);
// niqki_unite (nq_unite.hip; launch shape in nq_unite_blocks.h): dst(s, l) = the minimum of row s of src over the columns
// members[off[l] .. off[l + 1]) for the n_labels labels, empty in the columns [n_labels, dst_cap) (off: n_labels + 1
// entries; every member below src_cap; ANOTHER store than src)
hipError_t launch_store_unite(const uint16_t *src, uint64_t src_cap, uint16_t *dst, uint64_t dst_cap, uint32_t f_local, uint32_t n_labels,
                              const uint32_t *off, const uint32_t *members, hipStream_t stream);
// niqki_registers / niqki_sketch_registers (nq_registers.hip): ADD to hist, u32 [n][2^H + 1] preset by the caller, the
// register histograms (cell >> M; the last bin: cells outside [0, 2^W)) of store columns [begin, end) over f_local rows,
// or of n sketch rows of F cells.  d must be regular (mask_m, max_rem as the constructor derives them from H), H <= 6.
hipError_t launch_store_registers(const Derived &d, const uint16_t *store, uint64_t cap, uint32_t f_local, uint32_t begin, uint32_t end,
                                  uint32_t *hist, hipStream_t stream);
hipError_t launch_row_registers(const Derived &d, const int32_t *sketches, uint32_t n, uint32_t *hist, hipStream_t stream);
// Build, phase 1: units per (tile, slot) -> exclusive prefix per tile in
// slot_units, tile totals as a prefix (in ids) in tile_base.
hipError_t launch_build_sizes(const IndexView &v, uint32_t *slot_units, uint64_t *tile_base,
                              hipStream_t stream);
// Build, phase 2: entries + gids (gids sized from tile_base[n_tiles]).
hipError_t launch_build_fill(const IndexView &v, Entry *entries, uint16_t *gids, hipStream_t stream);
// padded layout: the padding pattern over the whole id array (n_ids a multiple of 64), before the fill
hipError_t launch_pad_fill(uint16_t *gids, uint64_t n_ids, uint32_t tile, hipStream_t stream);
// (kPadWords, kPadMaxTile: nq_gather_plan.h)
// dump stream (src/niqki_index.cpp:42-55) of a whole-range index.
// layout: slot_word[s] (F+1 entries) = word position of bucket (s, 0) in the stream
// (header excluded); export: the words of slots [s0, s1) into `out` (word 0 = first
// word of slot s0).
hipError_t launch_export_layout(const IndexView &v, unsigned long long *slot_word, hipStream_t stream);
hipError_t launch_export(const IndexView &v, const unsigned long long *slot_word, uint32_t *out,
                         uint32_t s0, uint32_t s1, hipStream_t stream);
// inverse: walk the dump words of slots [s0, s0+n_slots) and write the sketch
// store.  slot_word: n_slots+1 word positions of the slots inside `words`.  Ids are valid below n_genomes (others
// are counted in *bad and not stored); id g is written to column col_base + g (0: an import; an append: the
// handle's genome count).
hipError_t launch_import(const Derived &d, const uint32_t *words, const uint64_t *slot_word,
                         uint16_t *store, uint64_t cap, uint32_t n_genomes, uint32_t col_base, uint32_t *bad,
                         uint32_t s0, uint32_t n_slots, hipStream_t stream);

// ---- query: counters (nq_gather.hip, nq_lookup.hip, nq_order.hip) ---------------
// Which of these kernels a launch takes, its scratch and its LDS: nq_gather_plan.h.  The launchers here carry a plan out.
// what the plan reads of a view
inline GatherFacts gather_facts(const IndexView &v) {
  return GatherFacts{v.d.R, v.f_local, v.n_tiles, v.tile, v.align_log2, v.padded != 0, v.n_genomes};
}
// gather-histogram: counts[q*stride + g] for all genomes (u16), one workgroup
// per (query, tile).
// stash: nq x (n_tiles-1) x f_local Entry scratch (unused for n_tiles == 1); shape.nt < 0: the packed words of
//        launch_lookup for ALL tiles (sketches are then unused)
// order: nullptr, or the locality order of the batch from launch_order (nq <= 4096)
// shape, lds_bytes: GatherPlan::shape and ::lds_bytes
// counts2: second counter plane, needed (and used) when the view has more than kPassSlots slots
// (S = 16 on a whole-range handle): a count can then reach 2^16, so the slots are walked in two
// passes of <= 2^15 and plane p holds pass p's counters; the true count is the 32-bit sum.
// Candidate output of a gather launch (multi-GPU path): while a query's counters leave LDS, the genomes
// with a count >= thr are appended to cand[q*cap ..] (unordered, at most cap kept) and n[q] grows by how
// many qualified.  The caller presets n to 0 and cand to -1; launches over further segments of the same
// index append.  Not with accumulate (slot pages) or a second plane.
struct CandOut {
  int32_t *cand = nullptr;
  int32_t *n = nullptr;
  uint32_t thr = 0, cap = 0;
  // Survivors (the sparse exchange without counter rows): every genome whose count reaches surv_thr
  // (<= thr) is appended as {genome id, count} to surv[q*surv_cap ..] (unordered, at most surv_cap kept)
  // and surv_n[q] grows by how many qualified.  With survivors the launch may run WITHOUT a counter row
  // (counts = nullptr): what another rank may ask about a genome that is not among them is answered from
  // the sketch store instead (nq_group.hip).
  int2 *surv = nullptr;
  int32_t *surv_n = nullptr;
  uint32_t surv_thr = 0, surv_cap = 0;
  // Hit lists (single-segment, single-plane indexes, any number of tiles): the thresholded hits of a query --
  // Index::query_sketch's result, src/niqki_index.cpp:662-666,:685 -- are picked while each tile's counters are still
  // in LDS and leave the kernel after the last tile, ordered by descending (count, gid): hl[q*hl_cap + i] =
  // count << 32 | gid (the keys order like the pairs) and hl_n[q] = how many there are.  Only a query with more than
  // hl_cap hits writes its 2N-byte counter row (to `counts`, which must be given) and leaves hl_n[q] > hl_cap:
  // launch_hitlist_emit thresholds and orders that row.
  // Not together with cand / surv.  hl_cap: a multiple of 4.
  unsigned long long *hl = nullptr;
  uint32_t *hl_n = nullptr;
  uint32_t *hl_over = nullptr;   // nq + 1 words: [0] is zeroed by the launch (launch_hitlist_scan lists the overflowing queries there)
  uint32_t hl_cap = 0, hl_min = 0;
};
hipError_t launch_gather(const IndexView &v, const int32_t *sketches, uint32_t nq,
                         uint16_t *counts, uint16_t *counts2, uint64_t stride, Entry *stash, const uint32_t *order,
                         const GatherShape &shape, size_t lds_bytes, hipStream_t stream, const CandOut &co = CandOut());
// true: no gather_kernel instantiation with the padded walk has static LDS in front of its dynamic block (asked of the
// runtime once per process): an input of the plan
bool gather_pad_at_zero();
// out[i] = a[i] + b[i]: as u16 with wrap-around (the reference's uint16 matrix counters, src/niqki_index.cpp:572)
// or as u32 (the two planes of a launch_gather above; the kernels are in nq_hits.hip)
hipError_t launch_plane_add16(uint16_t *a, const uint16_t *b, uint64_t n, hipStream_t stream);
hipError_t launch_plane_sum32(const uint16_t *a, const uint16_t *b, uint32_t *out, uint64_t n, hipStream_t stream);
// Slot-major look-up pre-pass for the queries of a launch (nq_lookup.hip): fills pre[q][tile][slot] (lookup_pre_bytes
// of scratch) with the kernel that `form` names (lookup_form of the plan and nq); its streamed-rows kernel reads v.ptab,
// the packed copy of the table that launch_pack_entries makes.
hipError_t launch_pack_entries(const IndexView &v, uint32_t *ptab, hipStream_t stream);
hipError_t launch_lookup(const IndexView &v, const int32_t *sketches, uint32_t nq, uint32_t *pre, const LookupForm &form,
                         hipStream_t stream);
// Locality order of a launch (nq_order.hip).  keys / order: nq words of scratch each
hipError_t launch_order(const IndexView &v, const int32_t *sketches, uint32_t nq, uint32_t *keys,
                        uint32_t *order, hipStream_t stream);
hipError_t launch_gathered(const IndexView &v, const int32_t *sketches, uint32_t nq,
                           unsigned long long *per_query, hipStream_t stream);

// ---- query: hits (nq_hits.hip) -------------------------------------------------
// threshold + compaction + order.  blk_counts: nq x n_blk scratch;
// hit_off nq+1 (u64); tmp_*: capacity-sized scratch for the sort.
struct HitsArgs {
  const uint16_t *counts;
  const uint16_t *counts2;   // second counter plane (S = 16) or nullptr: the count is the 32-bit sum
  uint64_t stride;
  uint32_t nq;
  uint32_t gid_begin, n_gids;
  uint32_t min_score;
  uint32_t *blk_counts;   // nq * n_blk
  uint32_t n_blk;
  unsigned long long *hit_off;  // nq+1
  uint32_t *hit_counts, *hit_gids;
  uint32_t *tmp_counts, *tmp_gids;
  uint64_t capacity;
  // top-k (k > 0): launch_hits_count takes hits_select_kernel, which finds each query's boundary -- the count T and
  // how many of the genomes with count T are kept, the largest gids -- and writes per block the entries kept
  // (blk_counts) and the ties at T dropped at the block's low-gid end (blk_skip: 0 = none, kSkipAllTies = all);
  // hits_compact_kernel keeps c > T plus the ties blk_skip leaves.  thr == nullptr: c >= min_score, as without top-k.
  uint32_t top_k = 0;
  uint32_t *thr = nullptr;        // nq: T of each query
  uint32_t *blk_skip = nullptr;   // nq * n_blk
  uint32_t *blk_tmp = nullptr;    // nq * n_blk * kSelBlkWords scratch of the select
};
constexpr uint32_t kHitsBlk = 4096;  // genomes per compaction block
constexpr uint32_t kSkipAllTies = 0xFFFFFFFFu;
constexpr uint32_t kSelBins = 4352;     // count >> 4 (<= 4096 for counts <= 2^16), padded to 17 per thread of 256
constexpr uint32_t kSelBlkWords = 17;   // per block: genomes above the boundary bin, then one per count of that bin
hipError_t launch_candidates(const uint16_t *counts, uint64_t stride, uint32_t nq, uint32_t n_gids, uint32_t thr,
                             uint32_t cap, int32_t *cand, int32_t *n, hipStream_t stream);
hipError_t launch_hits_count(const HitsArgs &a, hipStream_t stream);
// After a gather launch with hit lists (CandOut::hl): launch_hitlist_scan turns the queries' hit counts n[0..nq) into
// the offsets a.hit_off (hit_off[nq] = total); launch_hitlist_emit copies every query's ordered list to its place in
// hit_counts / hit_gids, and thresholds + orders the counter row (a.counts) of a query whose list overflowed.
// over: nq + 1 words of scratch (the queries whose lists overflowed, made by the scan, taken by the emit launch)
hipError_t launch_hitlist_scan(const uint32_t *n, const HitsArgs &a, uint32_t hl_cap, uint32_t *over, hipStream_t stream);
// n: the lists' sizes (hl_n of the gather launch); with a.top_k a query's segment holds the first min(n, k) entries
hipError_t launch_hitlist_emit(const HitsArgs &a, const uint32_t *n, const unsigned long long *hl, uint32_t hl_cap, const uint32_t *over,
                               hipStream_t stream);
hipError_t launch_hits_emit(const HitsArgs &a, hipStream_t stream);

// ---- single-linkage clusters (nq_cluster.hip) ------------------------------------
// parent[g] = g for g < n
hipError_t launch_cluster_init(uint32_t *parent, uint32_t n, hipStream_t stream);
// Unites, for every query t < nq and every hit g = hit_gids[i], hit_off[t] <= i < hit_off[t + 1], with g < t0 + t, the
// components of t0 + t and g on parent[]: the larger root goes under the smaller one.  One wavefront per query.
hipError_t launch_cluster_link(uint32_t *parent, uint32_t n, const unsigned long long *hit_off, const uint32_t *hit_gids,
                               uint32_t t0, uint32_t nq, hipStream_t stream);
// labels[g] = root of g; *n_roots (zeroed here) = number of roots.  labels may not alias parent.
hipError_t launch_cluster_flatten(const uint32_t *parent, uint32_t n, uint32_t *labels, uint32_t *n_roots, hipStream_t stream);

// ---- greedy representatives (nq_cluster.hip) -------------------------------------
enum : uint8_t { kUndecided = 0, kRep = 1, kCovered = 2 };   // state[g]; the caller presets it
// Decides the queries t0 + q, q < nq, of a batch whose hit lists
// are (hit_off, hit_gids) and whose earlier genomes are all decided: two launches over the batch, then one workgroup
// that runs the remaining rounds.  info: 4 words, zeroed once per call; info[0] = the most rounds a batch needed.
hipError_t launch_derep_decide(uint8_t *state, uint32_t n, const unsigned long long *hit_off, const uint32_t *hit_gids, uint32_t t0,
                               uint32_t nq, uint32_t *info, hipStream_t stream);
// every representative of the batch: best[g] = max(best[g], count << 32 | ~t) over its hits g != t
hipError_t launch_derep_assign(const uint8_t *state, unsigned long long *best, uint32_t n, const unsigned long long *hit_off,
                               const uint32_t *hit_counts, const uint32_t *hit_gids, uint32_t t0, uint32_t nq, hipStream_t stream);
// niqki_dereplicate_from: every query t0 + q of the batch: best[t] = max(best[t], count << 32 | ~g) over its own hits
// g < first, the given representatives (nothing is launched for first == 0)
hipError_t launch_derep_given(unsigned long long *best, uint32_t n, uint32_t first, const unsigned long long *hit_off,
                              const uint32_t *hit_counts, const uint32_t *hit_gids, uint32_t t0, uint32_t nq, hipStream_t stream);
// labels[g] = g or the representative in best[g]; label_counts (may be null) = 0 or the count in best[g];
// *n_reps (zeroed here) = number of representatives
hipError_t launch_derep_finish(const uint8_t *state, const unsigned long long *best, uint32_t n, uint32_t *labels, uint32_t *label_counts,
                               uint32_t *n_reps, hipStream_t stream);

// ---- single-linkage forest (nq_cluster.hip; the edge key: nq_linkage_key.h) --------
// One batch of the self-join: forest_new = the maximum spanning forest of forest_old (info[0] keys) and the pairs
// (g, t0 + q), g < t0 + q, of the batch's hit lists; info[0] = its size.  comp[n], best[n] are scratch.  The caller
// swaps the forests for the next batch.  linkage_rounds(n) = ceil(log2 n) + 1 rounds are enqueued; those after a round
// without offers return at once.
// info: kLinkageInfoHead + linkage_rounds(n) words, zeroed once per call.  info[0] = edges of forest_old (kept by the
// launches themselves), info[2] = the most rounds in which a batch hooked, info[3] = nonzero: a bug;
// info[kLinkageInfoHead + r] = nonzero: round r of this batch had offers.
constexpr uint32_t kLinkageInfoHead = 4;
uint32_t linkage_rounds(uint32_t n);
hipError_t launch_linkage_batch(uint32_t *comp, unsigned long long *best, const unsigned long long *forest_old,
                                unsigned long long *forest_new, uint32_t *info, uint32_t n, const unsigned long long *hit_off,
                                const uint32_t *hit_counts, const uint32_t *hit_gids, uint32_t t0, uint32_t nq, hipStream_t stream);

// ---- greedy cover of a query (nq_cover.hip; the rounds: nq_api_cover.hip) -----------
// One entry of the pick log: a round writes one per active row, in row order.  pos = the pick's place in its query's
// list, kCoverNoPick for a query that had no hit in the round (it leaves the active set).
constexpr uint32_t kCoverNoPick = 0xFFFFFFFFu;
struct CoverPick {
  uint32_t q, pos, count, gid, total;
};
// info words of a batch (zeroed per batch, kCoverInfoActive and kCoverInfoPicks rewritten per round)
enum : uint32_t { kCoverInfoActive = 0, kCoverInfoPicks = 1, kCoverInfoStuck = 2, kCoverInfoMismatch = 3, kCoverInfoWords = 4 };
struct CoverPickArgs {
  const unsigned long long *hit_off;   // n_active + 1: the round's hits at top_k = 1, at most one a row
  const uint32_t *hit_counts, *hit_gids;
  const uint32_t *qidx;                // n_active: the batch's query each row belongs to
  const int32_t *orig;                 // the batch's sketches as given, F apart
  int32_t *masked;                     // n_active working rows, F apart
  const uint16_t *store;               // slot-major u16 store of a whole-range handle: store[s * cap + g]
  uint64_t cap;
  uint32_t n_genomes, F, R, max_picks;
  uint32_t *n_picks;                   // per query of the batch
  uint32_t *flag;                      // n_active: out, the row goes on
  CoverPick *log;                      // n_active entries of this round
  uint32_t *info;                      // kCoverInfoWords
};
hipError_t launch_cover_init(uint32_t *qidx, uint32_t *n_picks, uint32_t n, hipStream_t stream);   // qidx[i] = i, n_picks[i] = 0
// Every row with a hit: total = its winner's matches against the original row, the matching cells of the masked row
// become -1; info[kCoverInfoMismatch] += |cells masked - count|, info[kCoverInfoStuck] += 1 where none was masked or
// the winner lies outside the index, info[kCoverInfoPicks] += 1.  One workgroup per row; right for any F >= 1.
hipError_t launch_cover_pick(const CoverPickArgs &a, uint32_t n_active, hipStream_t stream);
// pos[i] = the number of flagged rows before row i, info[kCoverInfoActive] = the number of flagged rows (pos: n + 1 words)
hipError_t launch_cover_compact_scan(const uint32_t *flag, uint32_t n_active, uint32_t *pos, uint32_t *info, hipStream_t stream);
// the flagged rows of src / qidx_src, in order, to the front of dst / qidx_dst
hipError_t launch_cover_compact(const uint32_t *flag, const uint32_t *pos, const int32_t *src, const uint32_t *qidx_src, int32_t *dst,
                                uint32_t *qidx_dst, uint32_t F, uint32_t n_active, hipStream_t stream);
// hit_off[0 .. n] = exclusive scan of n_picks
hipError_t launch_cover_finish(const uint32_t *n_picks, uint32_t n, unsigned long long *hit_off, hipStream_t stream);
// every pick of the log to place hit_off[q] + pos of the output arrays (hit_totals may be null)
hipError_t launch_cover_scatter(const CoverPick *log, uint64_t n_log, const unsigned long long *hit_off, uint32_t *hit_counts,
                                uint32_t *hit_gids, uint32_t *hit_totals, uint64_t capacity, hipStream_t stream);

// ---- collapsed hits: the best hit per label (nq_collapse.hip; the batches: nq_api_collapse.hip) -----------
// One entry of a collapsed list on its way out: the label's best member and how many members the full list holds.
struct CollapsedHit {
  uint32_t count, gid, members;
};
// info words of a batch: queries that took the global-table route; entries no table could take (a bug: the host ends the call)
enum : uint32_t { kCollapseInfoLong = 0, kCollapseInfoBad = 1, kCollapseInfoWords = 2 };
constexpr uint32_t kCollapseMaxLdsCap = 4096;
struct CollapseArgs {
  const unsigned long long *hit_off;   // nq + 1: the full ordered lists (top_k = 0) of the batch
  const uint32_t *hit_gids;
  const uint32_t *dense;               // per genome: its label as a dense id below n_labels
  uint32_t n_genomes, n_labels, nq;
  uint32_t lds_cap;                    // the longest list the LDS table takes
  uint32_t lds_slots;                  // collapse_lds_slots(lds_cap)
  uint32_t top_k;                      // 0 = no cut
  unsigned long long *tables;          // one cleared table of n_labels entries per workgroup of the launch, or null (no list is long)
  uint32_t *kept;                      // out, per hit: the label's members where the hit is its label's first, else 0
  uint32_t *n_kept;                    // out, per query: its kept hits, at most top_k
  uint32_t *info;                      // kCollapseInfoWords, zeroed by the caller
};
uint32_t collapse_lds_slots(uint32_t lds_cap);   // slots of the LDS table: a power of two >= 2 x lds_cap (12 bytes a slot)
// n_blocks workgroups share the nq queries; with tables, n_blocks of them.  Leaves every table cleared.
hipError_t launch_collapse_first(const CollapseArgs &a, uint32_t n_blocks, hipStream_t stream);
hipError_t launch_collapse_table_init(unsigned long long *tables, uint64_t n_entries, hipStream_t stream);   // every entry cleared
// off[0 .. n] = exclusive scan of n_kept
hipError_t launch_collapse_scan(const uint32_t *n_kept, uint32_t n, unsigned long long *off, hipStream_t stream);
// query q's first n_kept[q] kept hits, in list order, to out[off[q] ...)
hipError_t launch_collapse_emit(const unsigned long long *hit_off, const uint32_t *hit_counts, const uint32_t *hit_gids, const uint32_t *kept,
                                const uint32_t *n_kept, const unsigned long long *off, uint32_t n, CollapsedHit *out, hipStream_t stream);
hipError_t launch_collapse_unpack(const CollapsedHit *in, uint64_t n, uint32_t *hit_counts, uint32_t *hit_gids, uint32_t *hit_members,
                                  hipStream_t stream);   // (hit_members may be null)

// ---- hits chosen by share (nq_contain.hip; the batches: nq_api_contain.hip; the share: nq_contain_share.h) ----------
// One entry of a contained list on its way out.
struct ContainedHit {
  uint32_t share, count, gid;
};
// info words of a batch: lists ordered by radix passes (more than kContainNetworkMax survivors); gids or lists out of
// range (a bug: the host ends the call); query sizes of 2^40 or more (the host refuses the call)
enum : uint32_t { kContainInfoLong = 0, kContainInfoBad = 1, kContainInfoBadSize = 2, kContainInfoWords = 3 };
constexpr uint32_t kContainNetworkMax = 2048;   // survivors the bitonic network of contain_order_kernel takes
struct ContainArgs {
  const unsigned long long *hit_off;   // nq + 1: the full ordered lists (top_k = 0) of the batch
  const uint32_t *hit_counts, *hit_gids;
  const unsigned long long *sizes;     // per genome (0: none)
  const unsigned long long *qsizes;    // per query of the batch (0: none)
  uint32_t n_genomes, nq, F, mode, min_share, top_k;
  // per hit place, a query's at [hit_off[q], ...): its survivors' shares and 0xFFFFFFFF - position, in list order after
  // contain_share, in the contained list's order after contain_order; b_*: where the radix passes turn round
  uint32_t *a_share, *a_npos, *b_share, *b_npos;
  uint32_t *n_surv;                    // per query: its sized hits with share >= min_share
  uint32_t *n_kept;                    // per query: min(n_surv, top_k)
  uint32_t *n_unsized;                 // per query: its hits without a size
  uint32_t *info;                      // kContainInfoWords, zeroed by the caller
};
// a workgroup per query: the shares, the survivors compacted in list order, n_surv, n_unsized
hipError_t launch_contain_share(const ContainArgs &a, hipStream_t stream);
// a workgroup per query: its survivors into the contained list's order (in a_*), n_kept
hipError_t launch_contain_order(const ContainArgs &a, hipStream_t stream);
// query q's first n_kept[q] entries to out[off[q] ...), count and gid fetched by position
hipError_t launch_contain_emit(const ContainArgs &a, const unsigned long long *off, ContainedHit *out, hipStream_t stream);
hipError_t launch_contain_unpack(const ContainedHit *in, uint64_t n, uint32_t *hit_shares, uint32_t *hit_counts, uint32_t *hit_gids,
                                 hipStream_t stream);

// ---- taxon of a query: the LCA of its near-best hits (nq_lca.hip; the batches: nq_api_lca.hip) ------------
// One taxon of the device taxonomy: a step up the tree is one 8-byte load.  A root is its own parent at depth 0.
struct TaxNode {
  uint32_t parent, depth;
};
constexpr uint32_t kTaxonNone = 0xFFFFFFFFu;   // NIQKI_TAXON_NONE: absorbing in the fold
// info words of a call: queries folded by the whole workgroup; gids or nodes out of range (a bug: the host ends the
// call); queries with two or more considered hits and no common taxon
enum : uint32_t { kLcaInfoLong = 0, kLcaInfoBad = 1, kLcaInfoNoCommon = 2, kLcaInfoWords = 3 };
constexpr uint32_t kLcaMinWaveCap = 64, kLcaMaxWaveCap = 65536;
struct LcaArgs {
  const unsigned long long *hit_off;   // nq + 1: the full ordered lists (top_k = 0) of the leaf
  const uint32_t *hit_counts, *hit_gids;
  const TaxNode *nodes;                // n_taxa
  const uint32_t *genome_taxon;        // n_genomes, each below n_taxa
  uint32_t n_genomes, n_taxa, max_depth, nq;
  uint32_t top_permille;               // 0 .. 1000
  uint32_t wave_cap;                   // the longest considered prefix one wavefront folds
  uint32_t *taxon;                     // out, nq rows each; the three below may be null
  uint32_t *best_count, *best_gid, *considered;
  uint32_t *info;                      // kLcaInfoWords, zeroed by the caller; the launch adds to them
};
hipError_t launch_lca(const LcaArgs &a, hipStream_t stream);

// ---- label audit: a genome's neighbours against its label (nq_audit.hip; the self-join: nq_api_audit.hip) ----
// info words of a call: gids outside the index or lists longer than it (a bug: the host ends the call)
enum : uint32_t { kAuditInfoBad = 0, kAuditInfoWords = 1 };
constexpr uint32_t kAuditMaxK = 63;   // the first k + 1 entries of a list are one wavefront's load
struct AuditArgs {
  const unsigned long long *hit_off;   // nq + 1: the full ordered lists (top_k = 0) of genomes t0 .. t0 + nq
  const uint32_t *hit_counts, *hit_gids;
  const uint32_t *labels;              // n_genomes: any label values (the kernel only compares them)
  uint32_t n_genomes, t0, nq;
  uint32_t k;                          // 1 .. kAuditMaxK: the entries that vote
  // out, n_genomes rows each, written at t0 .. t0 + nq; each may be null
  uint32_t *verdict, *own_count, *own_gid, *other_count, *other_gid, *vote_gid, *vote_n;
  uint32_t *info;                      // kAuditInfoWords, zeroed by the caller; the launch adds to them
};
hipError_t launch_audit(const AuditArgs &a, hipStream_t stream);

// ---- taxon tally: the LCA rows counted per taxon and clade (nq_tally.hip; the calls: nq_api_tally.hip) ----
// A workgroup of tally_rows_kernel combines a pass of kTallyPassRows rows in an LDS table of kTallySlots slots
// {key u32, count u32, best sum u64} (32 KiB) before anything reaches global memory.
constexpr uint32_t kTallyPassRows = 1024, kTallySlots = 2048;
// the 64-bit words beside the accumulators: rows with a taxon, rows without a hit, rows without a common taxon, bad rows
enum : uint32_t { kTallyClassified = 0, kTallyNoHit = 1, kTallyNoCommon = 2, kTallyBad = 3, kTallyWords = 4 };
struct TallyArgs {
  const uint32_t *taxon;               // n rows
  const uint32_t *best_count;          // n, or null: all zeros
  const uint32_t *considered;          // n, or null: a row without a taxon has no hit
  uint32_t n, n_taxa;
  unsigned long long *direct, *direct_best;   // n_taxa each; the launch adds to them
  unsigned long long *words;           // kTallyWords; the launch adds to them
};
hipError_t launch_tally_rows(const TallyArgs &a, hipStream_t stream);
struct TallyCladeArgs {
  const TaxNode *nodes;                // n_taxa
  uint32_t n_taxa, max_depth;
  const unsigned long long *direct, *direct_best;
  unsigned long long *clade, *clade_best;   // n_taxa each, zeroed by the caller
};
hipError_t launch_tally_clade(const TallyCladeArgs &a, hipStream_t stream);

// ---- FASTA / FASTQ framing (nq_ingest.hip) --------------------------------------
constexpr uint32_t kIngestBlock = 256;
constexpr uint32_t kIngestChunk = 8192;  // bytes per workgroup; chunks never span two files
struct IngestArgs {
  const uint8_t *raw;           // bytes of all files (16-byte aligned, >= 64 readable bytes after the end)
  const uint64_t *file_off;     // n_files+1 offsets into raw
  const uint8_t *file_type;     // n_files: 'A' (FASTA) or 'Q' (FASTQ)
  const uint32_t *chunk_first;  // n_files+1: first chunk of each file
  uint32_t n_files, n_chunks;
  uint32_t *summ;               // n_chunks x 5, pass 1 -> 2
  uint32_t *chunk_out;          // n_chunks x 4, pass 2 -> 3
  uint64_t *file_kept;          // n_files+1: sequence bytes before each file (after launch_ingest_scan)
  uint32_t *file_nrec;          // n_files+1: records before each file   (  "  )
  uint64_t *totals;             // {records, sequence bytes}
  uint8_t *seqs;                // out: record sequences back to back
  uint64_t *rec_off;            // out: n_rec+1 (entry n_rec is written by the caller)
  uint64_t *hdr_pos;            // out: raw offset of each record's header line
};
// passes 1+2 (census, per-file chaining, bases); then the caller sizes rec_off/hdr_pos
// from totals[0] and runs pass 3
hipError_t launch_ingest_scan(const IngestArgs &a, hipStream_t stream);
hipError_t launch_ingest_emit(const IngestArgs &a, hipStream_t stream);
// lines mode: records [0, n_use) longer than K -> entries (<= max_entries);
// result = {n_entry, first record not consumed}; entry_rec gets n_entry+1 values
hipError_t launch_ingest_entries(const uint64_t *rec_off, const uint64_t *hdr_pos, uint32_t n_use, uint32_t K,
                                 uint32_t max_entries, uint32_t *entry_rec, uint64_t *entry_hdr,
                                 uint32_t *result, hipStream_t stream);

// Packed FASTA (nq_pack.h) back to the files' bytes: segment k writes raw[dst ..) from wire[src ..); count / width as
// nqp::PackSeg (width 0: `count` bytes copied; else `count` lines of `width` bases + '\n' from 2-bit codes);
// first_block: exclusive prefix of ceil(raw length / kUnpackChunk) over the segments (n_blocks = its total).
constexpr uint32_t kUnpackChunk = 16384;
struct UnpackSeg {
  uint64_t dst, src;
  uint32_t count, width;
  uint32_t first_block, pad_;
};
hipError_t launch_unpack(const UnpackSeg *segs, uint32_t n_seg, uint32_t n_blocks, const uint8_t *wire, uint8_t *raw, hipStream_t stream);

// ---- gzip members inflated on the device (nq_inflate.hip) ------------------------------------------
// One job per gzip file: its bytes wire[src, src + src_len) become raw[dst, dst + cap), cap = the size the file's
// trailer announces.  status 0: every member decoded, CRC-32 and sizes agree, exactly cap bytes were written.  Any
// other status (1 header, 2 block type, 3 stored length, 4 code lengths, 5 symbol, 6 distance too far back, 7 more
// than cap bytes, 8 input ends early, 9 CRC, 10 member size, 11 bytes behind the last member, 12 fewer than cap
// bytes): the file is to be read some other way -- nothing was written outside [dst, dst + cap).
struct InflateJob {
  uint64_t src, src_len, dst, cap;
};
struct InflateOut {
  uint32_t status, members;
  uint64_t produced, consumed;
  uint32_t rounds, round_bytes, serial_tokens, blocks;   // how the file was decoded (nq_inflate.hip)
#ifdef NQ_INFLATE_CLOCK
  uint64_t clk[8];   // shader cycles by phase (diagnosis build only)
#endif
};
constexpr uint32_t kInflateXtabWords = 130;
uint32_t inflate_resident_files(bool small_ring);   // workgroups of a form of the kernel the current device keeps resident
void inflate_xtab(uint32_t *t);   // host: the CRC folding constants the kernel reads (kInflateXtabWords words)
// wire_bytes: readable bytes of `wire` (the kernel loads whole dwords up to there); raw: 16-byte aligned
// small_ring: -1 = choose by the number of files (the whole 32 KB window in LDS, four files per CU at a time, or its
// last 8 KB with far matches read back from the output, ten per CU), 0 / 1 = force (tests)
hipError_t launch_inflate(const InflateJob *jobs, uint32_t n_jobs, const uint8_t *wire, uint64_t wire_bytes, uint8_t *raw,
                          const uint32_t *xtab, InflateOut *outs, hipStream_t stream, int small_ring = -1);

// ---- synthetic genomes (nq_synth.hip) ----------------------------------------
hipError_t launch_synth(uint64_t seed, const uint32_t *family, const uint32_t *member,
                        const uint32_t *rate14, uint32_t n, uint64_t len, uint64_t stride,
                        uint8_t *out, hipStream_t stream);

hipError_t launch_synth_reads(uint64_t seed, const uint32_t *family, const uint32_t *member, const uint32_t *rate14,
                              const uint64_t *offset, const uint32_t *read_id, uint32_t read_rate14, uint32_t n,
                              uint32_t len, uint64_t stride, uint8_t *out, hipStream_t stream);

// ---- integer-ALU ceiling probes (nq_probe.hip; measurement support) -----------------------------
// what = 0: independent 32-bit adds; 1: 32-bit multiplies (v_mul_lo_u32); 2: the sketch kernel's
// per-k-mer arithmetic alone (roll, canonical choice, high word of the filter hash, K = 31) with no
// LDS, memory or compaction; 3: v_lshl_add_u32 (the issue class of most vector opcodes).
// *units = adds / multiplies / k-mers / instructions executed; timed by the caller.
hipError_t launch_alu_probe(int what, uint32_t iters, uint32_t *sink, uint64_t *units, hipStream_t stream);
// dst[0, bytes) = src[0, bytes) by a plain grid-stride kernel (bytes a multiple of 16)
hipError_t launch_copy_probe(const void *src, void *dst, uint64_t bytes, hipStream_t stream);

}  // namespace nq
