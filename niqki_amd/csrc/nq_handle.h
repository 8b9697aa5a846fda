// nq_handle.h -- the handle behind the C ABI (niqki_index) and the library-internal helpers
// shared by nq_api.hip (single-GPU entry points) and nq_group.hip (slot-sharded groups).
// Private to libniqki_hip.so.
//
// Full hit lists: what the calls that consume a query's full hit lists on the device share -- niqki_cluster,
// niqki_dereplicate and niqki_linkage (nq_api_selfjoin.hip), niqki_audit (nq_api_audit.hip), niqki_query_collapsed (nq_api_collapse.hip),
// niqki_query_lca (nq_api_lca.hip), niqki_query_contained (nq_api_contain.hip) and, without the halving, niqki_cover
// (nq_api_cover.hip).  Bodies: nq_api_lists.hip.
//   CallParams    the call's min_score / top_k on the handle, the handle's own back on every exit
//   PhaseTimer    HIP events around the phases of a call while the handle is profiling
//   hit_room      how many hits the fixed hit buffers take (option "cluster_ws_mib")
//   HitLists      the batch loop over a SketchSource and the leaf that halves a batch whose lists exceed the room
//   ensure_keep   ensure() that keeps what a batch has already written to the buffer
#pragma once
#include "../../include/niqki_hip.h"
#include "../../include/niqki_hip_bench.h"
#include "nq_kernels.h"

#include <functional>
#include <string>
#include <vector>

namespace nqi {

struct Buf {
  void *p = nullptr;
  size_t n = 0;
};

struct ProfSpan {
  int kc;
  hipEvent_t a, b;
};

// what niqki_get_stat reports of a self-join call (nq_api_selfjoin.hip)
struct SelfJoinStats {
  uint64_t splits = 0;   // batches the call had to halve
  uint64_t pairs = 0;    // the hits its kernels went through (while profiling is on)
  uint64_t rounds = 0;   // niqki_dereplicate: most decide rounds of a batch; niqki_linkage: most hooking rounds of a batch
  double ms[4] = {0, 0, 0, 0};
};

// what niqki_get_stat reports of the last niqki_cover / niqki_staged_cover call (nq_api_cover.hip)
struct CoverStats {
  uint64_t rounds = 0;       // the most rounds a batch ran
  uint64_t picks = 0;
  uint64_t mismatches = 0;   // cells masked against counts reported, summed: 0 unless there is a bug
  double ms[4] = {0, 0, 0, 0};   // while profiling is on: hits, pick, compact, finish
};

// what niqki_get_stat reports of the last niqki_query_collapsed / niqki_staged_query_collapsed call (nq_api_collapse.hip)
struct CollapseStats {
  uint64_t splits = 0;       // batches the call had to halve
  uint64_t long_lists = 0;   // queries whose list took the global-table route
  double ms[3] = {0, 0, 0};  // while profiling is on: hits, first, emit
};

// what niqki_get_stat reports of the last niqki_query_contained / niqki_staged_query_contained call (nq_api_contain.hip)
struct ContainStats {
  uint64_t splits = 0;       // batches the call had to halve
  uint64_t long_lists = 0;   // queries whose survivors the radix passes ordered
  double ms[3] = {0, 0, 0};  // while profiling is on: hits, share, order (with the scan and the emit)
};

// what niqki_get_stat reports of the last niqki_query_lca / niqki_staged_query_lca call (nq_api_lca.hip)
struct LcaStats {
  uint64_t splits = 0;       // batches the call had to halve
  uint64_t long_lists = 0;   // queries whose considered prefix the whole workgroup folded
  uint64_t no_common = 0;    // queries with two or more considered hits and no common taxon
  double ms[3] = {0, 0, 0};  // while profiling is on: hits, fold, the rows into an open tally
};

void shared_free(struct ::niqki_index *ix);   // nq_shared.hip

}  // namespace nqi

struct niqki_index {
  niqki_params p{};
  nq::Derived d{};
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  bool stream_prio_set = false;   // option "stream_priority": the own stream (and the side stream) were made with stream_prio
  int stream_prio = 0;
  std::string err;

  // sketch store, u16 [f_local][cap]
  uint16_t *store = nullptr;
  uint64_t cap = 0;
  uint32_t n_genomes = 0;

  // Paged index (option "resident_bytes"): the sketch store lives in page-locked host memory and
  // the inverted index exists for one page of slots at a time; a query batch walks the pages and
  // the gather kernel accumulates the counters (hit counts are sums over slots).  While a page is
  // resident, d.slot_begin/slot_end, store and cap describe THAT page, so every kernel and launch
  // sequence of the resident case is reused unchanged.
  uint64_t resident_bytes = 0;          // 0 = everything resident (default)
  uint16_t *host_store = nullptr;       // u16 [full_end - full_begin][host_cap], page-locked
  uint64_t host_cap = 0;
  uint32_t full_begin = 0, full_end = 0;   // the handle's real slot range
  uint32_t page_begin = 0, page_end = 0;   // slots (relative to full_begin) of the resident page; equal = none
  uint32_t page_n = 0;                     // genomes the resident page was built for
  nqi::Buf pg_store, pg_stage;
  std::vector<uint64_t> pg_layout;      // dump word positions of all slots (export of a paged index), for pg_layout_n genomes
  uint32_t pg_layout_n = 0xFFFFFFFFu;

  // Inverted index: two segments of the same layout.  `main` is what niqki_build makes, over store columns [0, main.n).
  // Delta segment: genomes inserted after that build get an index of their own over the columns behind the main
  // segment's, [delta.g_base, delta.g_base + delta.n), instead of a rebuild of everything (build_if_needed); a query
  // walks the delta, then the main segment, and their counter columns are disjoint.  delta.n == 0: there is none.
  // What a segment owns is named in three places: here, view() and free_segment() (nq_api_build.hip).
  struct Seg {
    nq::Entry *entries = nullptr;
    uint16_t *gids = nullptr;
    uint64_t *tile_base = nullptr;   // n_tiles+1, device
    uint32_t *slot_units = nullptr;  // n_tiles x (f_local+1), device
    uint32_t *ptab = nullptr;        // packed copy of `entries` for the look-up pre-pass (made at its first launch)
    uint16_t *hmask = nullptr;       // per slot: which sixteenths of the fingerprint range hold a bucket (IndexView::hmask)
    size_t entries_bytes = 0, gids_bytes = 0, tile_base_bytes = 0, slot_units_bytes = 0, ptab_bytes = 0, hmask_bytes = 0;
    uint32_t tile = 0, n_tiles = 0, align_log2 = 0, padded = 0;
    uint32_t n = 0, g_base = 0;      // the genomes it covers: how many, and the first
    uint32_t stripe = 0;             // tiles are dealt round-robin
    bool ptab_ok = false, hmask_ok = false;
  } main, delta;
  uint32_t built_n = 0;
  bool built = false;
  int stripe_opt = 32;             // option: block size of the stripes when there are several tiles (0 = ranges)
  int bucket_align = -1;           // option: log2 ids per bucket alignment unit, -1 = choose
  int incremental = 1;             // option "incremental_build"

  // niqki_append_begin .. the last niqki_append_slots: the dump's n_new genomes are being written into the store columns
  // [n_genomes, n_genomes + n_new), which no reader looks at; the commit adds n_new to n_genomes (nq_api_dump.hip)
  struct {
    bool active = false;
    uint32_t n_new = 0, next_slot = 0;
  } append;

  void *shared_state = nullptr;   // nq_shared.hip: the combiner of the *_shared (many host threads) entry points

  int gather_variant = 0;
  uint32_t last_densify_form = 0;   // stat "last_densify_form": nq::DensifyForm of the last sketch / densify call
  uint32_t last_form = 0;        // stat "last_gather_form": 1 = look-up pre-pass, 2 = packed table prepared (streamed rows from 512 queries per launch), 4 = locality order
  uint32_t last_kernel = 0;      // stat "last_gather_kernel": nq::gather_shape_code of the last gather launch
  uint64_t record_len_hint = 0;  // avg bytes per sketch for device-side batches (0 = read it back)
  uint32_t query_batch = 1024;
  int query_order = 1;           // option: order the queries of a launch for cache locality (1 = where it pays, 2 = wherever possible)
  int lookup_prepass = -1;       // option: slot-major table look-up pre-pass: -1 = when it pays, 0 = never, 1 = whenever usable
  int hit_lists = 1;             // option: queries of a single small tile leave the gather kernel as ordered hit lists (no counter rows)
  uint32_t hit_list_cap = 256;   // option: hits per query such a list holds; a query with more goes through its counter row
  uint32_t last_hits_form = 0;   // stat "last_hits_form": 1 = the last query call took the hit-list form
  uint32_t cluster_ws_mib = 1024;   // option "cluster_ws_mib": device hit buffers of a niqki_cluster batch (nq_api_selfjoin.hip)
  // the last niqki_cluster / niqki_dereplicate call (stats "cluster_*", "derep_*").  ms, while profiling is on: store
  // read, gather + hits, then link and flatten (cluster) or decide and assign (derep)
  // niqki_linkage (stats "linkage_*"): store read, gather + hits, forest rounds, then sort + hierarchy + copies
  // niqki_audit (stats "audit_*"): store read, gather + hits, the scan of the lists
  nqi::SelfJoinStats cluster_stats, derep_stats, linkage_stats, audit_stats;
  // niqki_audit: the info words of a call, then a host call's seven result arrays of n_genomes words each
  nqi::Buf ws_audit;
  nqi::CoverStats cover_stats;
  // niqki_cover: two buffers of masked rows with their query numbers, the per-row and per-query words, the pick log, a
  // batch's picks on their way to the host
  nqi::Buf ws_cv_sk[2], ws_cv_idx, ws_cv_log, ws_cv_out;
  // niqki_set_labels: the genomes' labels as dense ids (device, n_genomes words) and how many there are; every call that
  // changes the genome set drops them (drop_labels)
  nqi::Buf lab_dense;
  uint32_t n_labels = 0;
  bool labels_set = false;
  uint32_t collapse_lds_cap = 1024;   // option "collapse_lds_cap": the longest list the LDS table of collapse_first_kernel takes
  nqi::CollapseStats collapse_stats;
  // niqki_query_collapsed: a flag word per hit, the kept counts per query, a leaf's offsets and info words, the global
  // tables, a batch's collapsed entries, its offsets on their way to the host
  nqi::Buf ws_cl_keep, ws_cl_nk, ws_cl_off, ws_cl_tab, ws_cl_stage;
  bool cl_tab_clean = false;   // every entry of ws_cl_tab is cleared (false after growth and while a call is under way)
  // niqki_set_sizes: a size per genome (device, n_genomes 64-bit words, each below 2^40; 0 = none); every call that
  // changes the genome set drops them (drop_sizes).  Independent of labels and taxonomy.
  nqi::Buf sizes_dev;
  bool sizes_set = false;
  nqi::ContainStats contain_stats;
  // niqki_query_contained: a host batch's query sizes; where the radix passes turn round (8 bytes a hit); per query of a
  // batch the kept and unsized counts, then a leaf's survivors; a leaf's offsets and info words; a batch's entries
  nqi::Buf ws_ct_qs, ws_ct_tmp, ws_ct_n, ws_ct_off, ws_ct_stage;
  // niqki_set_taxonomy: a node {parent, depth} per taxon and every genome's taxon (device), how many taxa there are and
  // the largest depth; every call that changes the genome set drops them (drop_taxonomy).  Independent of the labels.
  nqi::Buf tax_nodes, tax_genome;
  uint32_t n_taxa = 0, tax_depth = 0;
  bool tax_set = false;
  uint32_t lca_wave_cap = 1024;   // option "lca_wave_cap": the longest considered prefix one wavefront of lca_kernel folds
  nqi::LcaStats lca_stats;
  // niqki_query_lca: a host call's result rows of a batch, the info words of a call
  nqi::Buf ws_lca_out, ws_lca_info;
  // niqki_tally_*: kTallyWords 64-bit words, then direct, direct_best, clade and clade_best of tally_taxa entries each
  // (device); the rows a caller left out of an LCA call or a host call's staged rows.  The tally belongs to the
  // taxonomy: whatever sets, removes or drops that ends it (end_tally).
  nqi::Buf tally_acc, ws_tally_rows;
  int tally_state = 0;            // stat "tally": 0 none, 1 open, 2 broken (tally_why says how)
  uint32_t tally_taxa = 0;
  std::string tally_why;
  uint64_t tally_queries = 0;     // stat "tally_queries": rows added as of the last read
  double tally_ms[2] = {0, 0};    // while profiling is on: the row kernel of the last LCA or add call, the clade kernel of the last read
  // the last niqki_retain call while profiling was on (stats "retain_us_rank", "retain_us_compact"): rank pass, compaction
  double retain_ms[2] = {0, 0};
  // the last niqki_unite call while profiling was on (stats "unite_us_prepare", "unite_us_min"): the host's numbering and
  // member lists with their copies, the minimum pass
  double unite_ms[2] = {0, 0};
  // niqki_registers / niqki_sketch_registers / niqki_staged_registers: a host call's histograms on the device; the last
  // call of each kernel while profiling was on (stats "registers_us_store", "registers_us_rows")
  nqi::Buf ws_reg;
  double registers_ms[2] = {0, 0};

  nqi::Buf ws_seq, ws_recoff, ws_entry, ws_sk, ws_counts, ws_blk, ws_hitoff, ws_hc, ws_hg, ws_tc, ws_tg,
      ws_misc, ws_stash, ws_hl, ws_parent;
  // staged batch (niqki_stage_raw): framing results live in ws_seq / ws_recoff / ws_entry
  nqi::Buf ws_raw, ws_fmeta, ws_summ, ws_chunk, ws_fkept, ws_fnrec, ws_hdrpos, ws_ehdr, ws_stsk, ws_order, ws_pre, ws_useg, ws_ijob, ws_xtab;
  uint64_t inflate_stats[4] = {0, 0, 0, 0};   // niqki_gunzip_stats
  int inflate_window = -1;   // option "inflate_window": which form of the inflate kernel a launch takes
  bool xtab_ok = false;   // ws_xtab holds the CRC folding constants of the inflate kernel
  struct {
    bool valid = false, sketched = false;
    uint32_t n_entry = 0, n_rec = 0;
    uint64_t seq_bytes = 0;
    uint64_t entry_bytes = 0;   // sequence bytes of the records the entries cover (lines mode may stop before the last framed record)
    const uint32_t *entry_rec = nullptr;  // device, n_entry+1
  } staged;
  // niqki_stage_raw_prefetch: file bytes of coming batches on their way into ws_wire[slot] on copy_stream.  Two
  // slots, taken in turn: the bytes of batch i + 1 may cross while batch i -- whose own (prefetched) bytes are still
  // being inflated / unpacked out of the other slot -- is staged.
  nqi::Buf ws_wire[2];
  nqi::Buf ws_redo[2];   // sketch_dev: flags of short-record sketches left to the second launch ([1]: calls on the sketch lane)
  hipStream_t copy_stream = nullptr;
  struct {
    bool valid = false;
    std::vector<const uint8_t *> ptr;
    std::vector<uint64_t> off;
    hipEvent_t ev = nullptr;
  } pre[2];
  uint32_t pre_next = 0;   // the slot the next prefetch takes

  // niqki_sketch_ahead / niqki_query_ahead: the sketches of up to two coming query batches, made on the sketch lane (a
  // side stream of the handle) beside whatever the handle's stream runs -- the gather and hit kernels of the batch before
  hipStream_t sk_stream = nullptr;
  uint32_t sk_lane_cus = 0;      // option "sketch_lane_cus": the sketch lane's compute units (0 = all)
  struct Ahead {
    nqi::Buf sk;                 // n_entry x F cells
    uint32_t n_entry = 0;
    hipEvent_t done = nullptr;   // its sketch kernel has finished (recorded on sk_stream)
    hipEvent_t used = nullptr;   // the query that took it has read it (recorded on the handle's stream)
    bool used_set = false;
  } ahead[2];
  uint32_t ahead_head = 0, ahead_n = 0;   // the oldest slot in flight, how many are

  bool prof = false;
  double prof_ms[NIQKI_KC_COUNT] = {0};
  uint64_t prof_n[NIQKI_KC_COUNT] = {0};
  std::vector<nqi::ProfSpan> spans;
  std::vector<hipEvent_t> ev_pool;
  // side stream: the locality probe + order of a launch run beside its look-up pre-pass
  hipStream_t aux_stream = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
};


namespace nqi {

// ---- nq_api.hip: the handle ----
void *host_alloc(size_t bytes);   // page-locked host memory (niqki_host_alloc): slabs on transparent huge pages
void host_free(void *p);
int fail(niqki_index *ix, int code, const std::string &msg);
int ensure(niqki_index *ix, Buf &b, size_t bytes);   // device scratch of at least `bytes`
// ... whose first `keep` bytes stay what they are (nq_api_lists.hip; grows to twice the need, synchronises when it grows)
int ensure_keep(niqki_index *ix, Buf &b, size_t keep, size_t bytes);
nq::IndexView view(const niqki_index *ix, const niqki_index::Seg &seg);
inline nq::IndexView view(const niqki_index *ix) { return view(ix, ix->main); }   // the main segment
std::string &create_error();   // thread-local: why the last niqki_create / niqki_import_* of the calling thread failed
int derive(const niqki_params &p, nq::Derived &d, std::string &why);
int collect_spans(niqki_index *ix);
// more than 2^15 slots on the handle (whole-range S = 16): counts reach 2^16, two counter planes (nq_kernels.h, kPassSlots)
bool two_planes(const niqki_index *ix);
// first slot of the handle in a whole sketch row (while a page is resident d.slot_begin is the page's)
uint32_t first_slot(const niqki_index *ix);
// ---- nq_api_build.hip: sketch store, sketching, index segments ----
int reserve_store(niqki_index *ix, uint64_t want);
int sketch_dev(niqki_index *ix, const uint8_t *seqs, const uint64_t *rec_off, uint32_t n_rec, const uint32_t *entry_rec,
               uint32_t n_entry, int32_t *sketches, uint64_t total_bytes);
// the store the device has just filled replaces the handle's, for n genomes; a paged handle's host store was rewritten in place
int adopt_store(niqki_index *ix, uint16_t *ns, uint64_t cap, uint32_t n);
void host_store_rewritten(niqki_index *ix, uint32_t n);
int build_range(niqki_index *ix, niqki_index::Seg &seg, uint32_t g_base, uint32_t N);   // store columns [g_base, g_base + N) into seg
void free_segment(niqki_index::Seg &seg);              // its device buffers back to the device, seg = Seg()
uint64_t segment_bytes(const niqki_index::Seg &seg);   // what the stat "index_bytes" counts of it
// both segments freed: the genome set has changed, the next use builds one main segment
void release_segments(niqki_index *ix);
int build_if_needed(niqki_index *ix);
int build_single(niqki_index *ix);    // ONE index over all genomes (dump export, per-bucket statistics)
// the stored sketches of genomes [t0, t0 + n) as device query rows (resident store, or zero-copy from the paged host store)
int stored_sketch_rows(niqki_index *ix, uint32_t t0, uint32_t n, int32_t *dst);
// ---- nq_api_query.hip: counters and hits ----
uint32_t page_slots(const niqki_index *ix);
int load_page(niqki_index *ix, uint32_t s0, uint32_t s1);
int counts_resident(niqki_index *ix, const int32_t *sketches, uint32_t q_stride, uint32_t q_off, uint32_t nq, uint16_t *counts,
                    uint64_t stride, bool accumulate, uint16_t *counts2 = nullptr, const nq::CandOut *co = nullptr);
// hit counters of nq device-resident sketches (rows q_stride apart, this shard's slots at q_off)
// counts2: the second counter plane of a whole-range S = 16 handle (nq_kernels.h, kPassSlots), else nullptr
// co: also the candidate lists of the rows (nq_kernels.h CandOut; presets them itself), not on paged or S = 16 handles
int counts_dev(niqki_index *ix, const int32_t *sketches, uint32_t q_stride, uint32_t q_off, uint32_t nq,
               uint16_t *counts, uint64_t stride, uint16_t *counts2 = nullptr, const nq::CandOut *co = nullptr);
// The counter planes of n query rows in ws_counts: one, or two on a two-plane handle (c2 is null otherwise).
struct Planes {
  uint16_t *c1 = nullptr, *c2 = nullptr;
};
int counter_planes(niqki_index *ix, uint32_t n, uint64_t stride, Planes &pl, bool zeroed = false);
// Where the hits of a step go, in device memory: off (n + 1 offsets, off[n] = the total), then `capacity` places for
// counts and gids.  check: read the total back (a synchronise) into `total` and return NIQKI_E_CAPACITY, with nothing
// written to counts / gids, where it exceeds the capacity; without it more hits than `capacity` are the caller's error.
struct HitOut {
  unsigned long long *off = nullptr;
  uint32_t *counts = nullptr, *gids = nullptr;
  uint64_t capacity = 0;
  bool check = false;
  uint64_t total = 0;   // out, with check
};
// ... in the handle's own buffers (ws_hitoff, ws_hc, ws_hg) for n queries and `capacity` hits, checked
int hit_out_ws(niqki_index *ix, uint32_t n, uint64_t capacity, HitOut &out);
// off[0..n] of a checked step (rc: what it returned) and, where it fitted, its hits to host memory; synchronises.
// Returns rc.
int hits_to_host(niqki_index *ix, int rc, const HitOut &out, uint32_t n, void *hit_off, uint32_t *hit_counts, uint32_t *hit_gids);
// threshold + order of nq counter rows (counts2: the second plane or null) over genomes [gid_begin, gid_begin + n_gids)
int hits_dev(niqki_index *ix, const uint16_t *counts, const uint16_t *counts2, uint32_t nq, uint64_t stride, uint32_t gid_begin,
             uint32_t n_gids, HitOut &out);
int query_hits_dev(niqki_index *ix, const int32_t *sketches, uint32_t nq, const Planes &pl, uint64_t stride, HitOut &out);
// Hits of nq queries into HOST arrays, batches of qb queries, hits appended in query order.  src makes the sketches of
// queries [q0, q0 + n) device-resident whole rows and names them in *d_sk.
using SketchSource = std::function<int(uint32_t q0, uint32_t n, const int32_t **d_sk)>;
SketchSource host_rows(niqki_index *ix, const int32_t *sketches);      // through ws_sk
SketchSource device_rows(niqki_index *ix, const int32_t *sketches);
SketchSource stored_rows(niqki_index *ix, uint32_t begin);             // genomes from `begin` on, through ws_misc
uint32_t query_rows_per_batch(const niqki_index *ix);   // option "query_batch", or more where no counter rows are written
int query_to_host(niqki_index *ix, const SketchSource &src, uint32_t nq, uint32_t qb, uint64_t *hit_off, uint32_t *hit_counts,
                  uint32_t *hit_gids, uint64_t capacity);
// ---- nq_api_lists.hip: full hit lists (the head of this file) ----
// The query path with a call's own threshold and top_k; the handle's own values come back whatever happens.
struct CallParams {
  niqki_index *ix;
  const uint32_t ms, pms, k;   // the handle's own d.min_score, p.min_score, p.top_k
  CallParams(niqki_index *ix_, uint32_t min_score, uint32_t top_k);
  ~CallParams();
};
// Events 0 .. n_events - 1 on the handle's stream.  Unless the handle is profiling (ix->prof) there are none, and
// mark and add do nothing.  add: the span a .. b, finished (it synchronises on b), onto ms[to].
struct PhaseTimer {
  niqki_index *ix;
  double *ms;
  std::vector<hipEvent_t> ev;
  PhaseTimer(niqki_index *ix_, int n_events, double *ms_) : ix(ix_), ms(ms_), ev((size_t)n_events, nullptr) {}
  ~PhaseTimer();
  int create();
  int mark(int k);
  int add(int a, int b, int to);
};
// hits the fixed hit buffers (hit_out_ws) take within option "cluster_ws_mib"; never below the genome count
uint64_t hit_room(const niqki_index *ix);
// One call that consumes full hit lists where the query path leaves them.  run: queries [0, nq) of src in batches of qb,
// in order; per batch src, leaf, then `after` where there is one.  leaf: n whole sketch rows at d_sk, the queries
// q_at .. q_at + n of the batch: counter_planes, hit_out_ws(hit_room), ev.mark(ev_hits), query_hits_dev.  Lists that
// exceed the room: one query is refused ("<who>: one query's hits exceed the genome count"), more are halved -- one more
// on `splits`, then the first n / 2 rows to the end, consumer included, before the others.  Lists that fit go to
// `consume`, which enqueues the consumer's kernels and marks its own phases.  q0 is the running batch's first query.
struct HitLists {
  niqki_index *ix;
  const char *who;
  PhaseTimer &ev;
  int ev_hits;
  uint64_t &splits;
  bool shrink;   // the batches after a halved one take the size of its smallest part (the self-join: no gather twice)
  std::function<int(const HitOut &out, const int32_t *d_sk, uint32_t q_at, uint32_t n)> consume;
  std::function<int(uint32_t q0, uint32_t n)> after;
  uint32_t q0 = 0;
  int run(const SketchSource &src, uint32_t nq, uint32_t qb);
  int leaf(const int32_t *d_sk, uint32_t q_at, uint32_t n, uint32_t *fitted);
};
// ---- nq_api_collapse.hip ----
void drop_labels(niqki_index *ix);   // the genome set changes: the labelling of niqki_set_labels goes
// ---- nq_api_contain.hip ----
void drop_sizes(niqki_index *ix);    // the genome set changes: the sizes of niqki_set_sizes go
// ---- nq_api_lca.hip ----
void drop_taxonomy(niqki_index *ix);   // the genome set changes: the taxonomy of niqki_set_taxonomy goes
// ---- nq_api_tally.hip ----
void end_tally(niqki_index *ix);       // the taxonomy is replaced or goes: so does the tally (the buffers stay the handle's)
void break_tally(niqki_index *ix, const std::string &why);   // an open tally holds part of a call's rows
// rows [0, n) in device memory into the open tally, in stream order (best_count, considered: may be null)
int tally_rows_dev(niqki_index *ix, const uint32_t *taxon, const uint32_t *best_count, const uint32_t *considered, uint32_t n);
// ---- nq_api_selfjoin.hip ----
// the handle counts whole sketches (no slot-range shard): what the self-join calls need
bool whole_range(const niqki_index *ix);
// One self-join with a consumer of the hit buffers: niqki_cluster (the link kernel), niqki_dereplicate (decide +
// assign), niqki_linkage (the forest kernels) or niqki_audit (nq_api_audit.hip: the audit kernel).  The batches go in
// index order and a halved batch finishes its first half before its second (HitLists): the dereplication relies on
// that (a batch's earlier genomes are all decided), the others do not care.
struct SelfJoin {
  niqki_index *ix;
  const char *who;
  SelfJoinStats &stats;
  // phases of a batch the stats time (stats.ms): store read, gather + hits, then the consumer's: 3 or 4 in all
  const int phases;
  // events: 0-1 the store read of a batch; of a leaf 2-3 gather + hits, then phase k = 2 .. phases - 1 between k + 1
  // and k + 2
  PhaseTimer ev;
  // Enqueues the consumer's kernels on the hits (off, hit_counts, hit_gids) of genomes [t0, t0 + n) and ends each of
  // its phases k = 2 .. phases - 1 with ev.mark(k + 2).
  std::function<int(const unsigned long long *, const uint32_t *, const uint32_t *, uint32_t, uint32_t)> consume;
  bool count_pairs = false;   // stats.pairs also without profiling (the total is read back per batch anyway)

  SelfJoin(niqki_index *ix_, const char *who_, SelfJoinStats &stats_, int phases_)
      : ix(ix_), who(who_), stats(stats_), phases(phases_), ev(ix_, phases_ + 2, stats_.ms) {}
};
// the self-join of genomes [begin, n_run) at the handle's min_score (the caller's CallParams) and top_k 0
int self_join_batches(SelfJoin &r, uint32_t n_run, uint32_t begin = 0);
// sketches of the handle's staged batch (niqki_stage_raw) into ix->ws_stsk, once per batch
int staged_sketch_ws(niqki_index *ix);
// appends n device-resident sketches (same addressing as counts_dev) to the sketch store
int insert_dev(niqki_index *ix, const int32_t *sketches, uint32_t sk_stride, uint32_t sk_off, uint32_t n);

// HIP events around a kernel class while profiling is on (niqki_profile_*)
struct Span {
  niqki_index *ix;
  int kc;
  hipEvent_t a = nullptr, b = nullptr;
  Span(niqki_index *ix_, int kc_);
  ~Span();
};

}  // namespace nqi

#define NQ_HIP(ix, call)                                                                    \
  do {                                                                                      \
    hipError_t e_ = (call);                                                                 \
    if (e_ != hipSuccess)                                                                   \
      return nqi::fail(ix, e_ == hipErrorOutOfMemory ? NIQKI_E_NOMEM : NIQKI_E_HIP,         \
                       std::string(#call) + ": " + hipGetErrorString(e_));                  \
  } while (0)
