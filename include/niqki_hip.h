/*
 * niqki_hip.h -- C ABI of the MI355X-native NIQKI sketch/query engine
 * (libniqki_hip.so).
 *
 * This is the drop-in boundary for the reference's hot path.  The reference
 * has no FFI layer: its boundary is the C++ class Index
 * (/root/reference/src/niqki_index.h:35-213) whose inner operators
 *
 *     void         compute_sketch(const string&, vector<int32_t>&) const;   niqki_index.h:103
 *     void         insert_sketch(const vector<int32_t>&, uint32_t gid);      niqki_index.h:108
 *     query_output query_sketch(const vector<int32_t>&) const;               niqki_index.h:142
 *
 * are what the file drivers call per record.  Each entry point below names the
 * reference interface (file:line under /root/reference) it replaces.  All
 * signatures are plain C: opaque handle, pointers and sizes, int status.
 * No exceptions cross the boundary.  Calls on one handle must be serialised by
 * the caller (one handle per GPU; the reference's const query methods map to
 * batched calls here, not to concurrent ones) -- except the niqki_*_shared entry
 * points, which any number of host threads may call on one handle at the same time
 * (the reference's `omp parallel` record loops, kept as they are).
 *
 * Memory spaces: every array argument of a call lives in the space named by
 * the call's `mem` argument -- NIQKI_MEM_HOST (pageable or pinned host memory;
 * the library stages it) or NIQKI_MEM_DEVICE (device memory of the handle's
 * GPU; nothing is copied, work is enqueued on the handle's stream and the call
 * returns without synchronising unless stated otherwise).
 *
 * Sketch layout: F = 2^S int32 per sketch, row major, -1 = empty cell, exactly
 * the reference's vector<int32_t>. *
 * Not here: measurement, diagnosis and test support (synthetic inputs, per-kernel timers, the steps of the sparse
 * multi-GPU exchange one by one ...) -- include/niqki_hip_bench.h.
 *
 * Environment variables the LIBRARY reads (none changes a result; options of niqki_set_option are the way to set
 * anything per handle):
 *   NIQKI_GROUP_TRANSPORT   rccl | ipc | local: transport of niqki_group_create / niqki_group_new_id (see "one index
 *                           over several GPUs" below); default: RCCL, device copies for shards that share a device
 *   NIQKI_IPC_WORDS         host | coarse: where an ipc rank keeps its sequence words (default: fine-grained device
 *                           memory, the shared host block where that cannot be exported); NIQKI_IPC_ARENA=coarse:
 *                           plain device memory for its exchange buffers.  Test switches.
 *   NIQKI_LOOKUP_PREPASS    -1 | 0 | 1: initial value of option "lookup_prepass" of every handle (the test suite runs
 *                           under both look-up paths this way)
 *   NIQKI_TILE_STRIPE       overrides option "tile_stripe" at every index build (tests of the tile dealing)
 *   NIQKI_HMASK=0           builds single-tile indexes without their per-slot class mask (stat "class_mask")
 *   NIQKI_SKETCH_WAVE=0     short records take the workgroup sketch kernel instead of the one-wavefront one;
 *   NIQKI_SKETCH_FILTER     0 = long records are sketched without the candidate filter, n >= 2 = with a fixed filter
 *                           strength (default: chosen per sketch).  Test switches of the sketch launch rule (nq_sketch_plan.h).
 * The `niqki` host program reads NIQKI_HOST_THREADS (reader threads; default: the CPUs the process may use),
 * NIQKI_HOST_TIMING (phase times on stderr), NIQKI_HOST_NO_PACK (plain FASTA files travel as their bytes),
 * NIQKI_HOST_NO_GPU_INFLATE (gzip files are always inflated by the reader threads), NIQKI_HOST_GPU_INFLATE_MIN (how many
 * gzip files a list must hold for the device to inflate them; default 32 per reader thread),
 * NIQKI_HOST_ZLIB_ONLY (no libdeflate), NIQKI_SHARDS_ON_ONE_DEVICE (--gpus N on one device: tests).
 */
#ifndef NIQKI_HIP_H
#define NIQKI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NIQKI_ABI_VERSION 2   /* 2: niqki_raw_batch.file_status, NIQKI_E_GZIP, niqki_sketch_ahead / niqki_query_ahead */

/* Bytes the caller must keep readable after the last sequence byte of a
 * NIQKI_MEM_DEVICE sequence buffer (the sketch kernel reads whole dwords). */
#define NIQKI_SEQ_PAD 64

enum niqki_status {
  NIQKI_OK = 0,
  NIQKI_E_INVALID = 1,     /* bad argument / unsupported parameter combination */
  NIQKI_E_NOMEM = 2,       /* host or device allocation failed */
  NIQKI_E_HIP = 3,         /* a HIP runtime call failed; see niqki_last_error */
  NIQKI_E_CAPACITY = 4,    /* caller buffer too small; sizes were still reported */
  NIQKI_E_STATE = 5,       /* call not valid in the handle's current state */
  NIQKI_E_NODEVICE = 6,    /* no usable gfx950 device */
  NIQKI_E_GZIP = 7         /* niqki_stage_raw: a file flagged NIQKI_FILE_GZIP is not a plain intact gzip file of the
                              size its trailer states (see niqki_raw_batch.file_status); nothing was staged */
};

enum niqki_mem { NIQKI_MEM_HOST = 0, NIQKI_MEM_DEVICE = 1 };

typedef struct niqki_index niqki_index; /* opaque */

/* Constructor arguments: Index(lF,K,W,H,filename,min_fract),
 * src/niqki_index.cpp:13-38 (output-file handling stays in the host program).
 * Supported: 1<=K<=31 (K=32 is UB in the reference, :28-29), 1<=S<=16,
 * H<=W<=15, S+W<=30.  S = 16 is the reference's lF>15 branch (uint32 counters, :668-682): a
 * count can reach 2^16, so the u16 counter calls (niqki_query_counts, niqki_hits_from_counts)
 * refuse it on a whole-range handle; niqki_query* / niqki_staged_query / niqki_query_counts32 are
 * exact (also on a paged handle, whose pages add up per half of the slots), and so are groups of
 * two or more shards (a shard counts at most 2^15 slots, the cross-shard sums travel as u32)
 * and niqki_matrix_range wraps like the reference's uint16 matrix counters (:572). */
typedef struct niqki_params {
  uint32_t K;          /* k-mer length */
  uint32_t S;          /* lF: log2 of the number of sketch slots */
  uint32_t W;          /* fingerprint bits */
  uint32_t H;          /* HyperLogLog bits inside the fingerprint */
  uint32_t min_score;  /* hits need count >= min_score (niqki_min_score) */
  uint32_t slot_begin; /* this shard owns sketch slots [slot_begin, slot_end); */
  uint32_t slot_end;   /*   0,0 means the whole range [0, 2^S)                 */
  int32_t device;      /* HIP device ordinal; -1 = current device */
  uint32_t tile_genomes; /* genomes per counter tile (0 = choose); see DESIGN.md */
  uint32_t resident_mib; /* > 0: paged index, as option "resident_bytes" (in MiB) from the start --
                            the way to load a dump into a paged handle */
  uint32_t top_k;      /* > 0: a query's hits are the first min(k, n) of its full list (option "top_k") */
  uint32_t reserved[1];
} niqki_params;

int niqki_abi_version(void);
const char *niqki_status_string(int status);

/* min_score = (uint32)(min_fract * 2^S): src/niqki_index.cpp:21-22 */
uint32_t niqki_min_score(double min_fract, uint32_t S);

/* Index::Index / Index::~Index: src/niqki_index.cpp:13-38, :106-109.
 * Fails with NIQKI_E_NODEVICE when there is no GPU: there is no CPU path. */
int niqki_create(const niqki_params *params, niqki_index **out);
void niqki_destroy(niqki_index *ix);
/* Index::select_best_H(genome_size) (the CLI's -G): src/niqki_index.cpp:126-164.
 * Picks H in 2..6 from the expected genome size and replaces H and M = W-H on
 * the handle.  As in the reference, the fingerprint's low-part mask and
 * saturation constant keep the values the constructor derived from the
 * ORIGINAL H (:24-25 are not recomputed), so the parts of a fingerprint may
 * overlap or exceed W bits; cells outside [0, 2^W) are sketched but never
 * indexed or queried (:364, :654).  May be called at any time, like the
 * reference's member; *H_out (may be NULL) receives the chosen H.
 * NIQKI_E_INVALID when the chosen H exceeds W (the reference's unsigned M
 * wraps there). */
int niqki_select_best_H(niqki_index *ix, double genome_size, uint32_t *H_out);
/* Text of the last error on the handle; with ix == NULL, why the last
 * niqki_create / niqki_import_dump of the calling thread failed. */
const char *niqki_last_error(const niqki_index *ix);
int niqki_get_params(const niqki_index *ix, niqki_params *out);

/* Work is enqueued on this hipStream_t (default: a stream the handle owns). */
int niqki_set_stream(niqki_index *ix, void *hip_stream);
void *niqki_get_stream(const niqki_index *ix);
int niqki_synchronize(niqki_index *ix);

/* Tuning knobs (no reference counterpart; none of them changes a result, except "min_score" and "top_k", the two
 * options that set what a query returns):
 * "gather_variant" (launch shape of the gather kernel, 0 = choose .. 5), "query_batch",
 * "tile_genomes" (multiple of 64, <= 65536; takes effect at the next build),
 * "bucket_align_log2" (-1 = choose, 0..6: buckets start on multiples of 2^a ids),
 * "tile_stripe" (B = 1, 2, 4 .. 64, default 32: with several tiles, blocks of B consecutive
 * genomes are dealt to the tiles round-robin, so a run of related genomes is spread over all
 * tiles; blocks of 32 are 64 bytes of a counter row, the smallest piece HBM writes without
 * a read-modify-write; 0 = tiles are ranges of genome ids),
 * "min_score", "top_k" (0 = default: every hit; k > 0: per query the first min(k, n) entries of the full list of
 * its n hits, in the same order -- count descending, among equal counts the larger gid first, so equal counts that
 * straddle the cut keep their largest gids; selected on the device from the counter rows, see "top-k" below),
 * "record_len_hint" (average bytes per sketch of NIQKI_MEM_DEVICE
 * batches, so that niqki_sketch need not read rec_off back to pick a launch
 * shape; 0 = read it back), "query_order" (1 = default: the queries of a launch
 * are processed in an order that puts similar ones on the same XCD where that pays --
 * >= 16384 genomes and >= 8192 slots on the handle; 2 = on every index; results are
 * unaffected; 0 = input order), "lookup_prepass" (1 = the index table is walked
 * once per launch, slot block by slot block, for all its queries instead of one random
 * table line per query and slot inside the gather kernel, wherever the index shape
 * allows: 16 % less HBM traffic.  The default (-1) uses it where it is also faster: batches of
 * >= 1024 queries on indexes of 1 or 2 counter tiles with W <= 12 (whole table rows are then
 * streamed through LDS from a packed copy of the table, +4 bytes per table entry: 8 % faster), and
 * indexes of more than 4 tiles, > 261 632 genomes (25 % faster); 0 = never),
 * "incremental_build" (1 = default: genomes inserted after a build get a delta index of their own
 * -- a query walks both -- until they pass an eighth of the main index, then everything is rebuilt;
 * 0 = every insert after a query rebuilds the whole index at the next query),
 * "resident_bytes" (indexes beyond the memory one wants to give them -- or beyond HBM: with a
 * value > 0, set before the first insert, the sketch store (2 bytes per genome and slot) lives
 * in page-locked host memory and the inverted index is built for one PAGE of slots at a time,
 * sized so that the page's store rows + index stay within the value; a query batch walks the
 * pages and the gather kernel accumulates the hit counters, which are sums over slots.  Same
 * answers as a resident index.  Insert, the dump import (niqki_params.resident_mib), every query
 * call, niqki_get_sketches, niqki_matrix_range (the stored sketches are read from the host store)
 * and the dump export (page after page) work on a paged handle; niqki_query_gathered, the
 * candidate / survivor calls and groups do not (NIQKI_E_STATE / NIQKI_E_INVALID)),
 * "stream_priority" (1 / 0 / -1: the handle gets a stream of its own, made at the top / default / bottom of
 * the device's stream priority range -- also after niqki_set_stream, whose stream stays the caller's --, so
 * that e.g. a query handle's short kernels are dispatched ahead of another handle's long sketch kernel;
 * niqki_get_stream returns it),
 * "sketch_lane_cus" (0 = default: all; n: the lane of niqki_sketch_ahead is made anew on the TOP n compute units of the
 * device's numbering (hipExtStreamCreateWithCUMask) -- for a caller that fences the two lanes, with its own stream
 * limited to the other units; on one MI355X the split is no faster than the hardware's own dispatch),
 * "hit_lists" (1 = default: on a resident single-segment index with counts below 2^16 -- one counter tile of at most
 * 12 288 genomes, the short-read shape of src/niqki_index.cpp:412-430, or a larger index of any number of tiles whose
 * counters leave room for the list in a workgroup's LDS -- niqki_query* / niqki_staged_query take a query's thresholded
 * hits out of the gather kernel while its counters are in LDS, already ordered, instead of writing a 2N-byte counter
 * row per query and reading it again; 0 = always through counter rows), "hit_list_cap" (1..2048, default 256: hits per query such a list holds; a
 * query with more -- min_score 0: every genome -- leaves through its counter row and is ordered from there),
 * "inflate_window" (-1 = default: a launch of the device inflate, NIQKI_FILE_GZIP below, keeps each file's whole 32 KB
 * window in LDS -- four files per CU at a time -- unless it holds more files than that runs at once; then only the
 * window's last 8 KB, ten files per CU, and matches that reach further back read the file's own flushed output;
 * 0 / 1 = always the first / second form.  Same bytes either way). */
int niqki_set_option(niqki_index *ix, const char *key, int64_t value);

/* Pre-sizes the sketch store for n_genomes (optional; the store grows). */
int niqki_reserve(niqki_index *ix, uint32_t n_genomes);

/* Index::compute_sketch (src/niqki_index.cpp:335-358) including
 * sketch_densification (:313-331), batched.
 *   seqs        concatenated record bytes (ASCII, no newlines)
 *   rec_off     n_rec+1 byte offsets into seqs
 *   entry_rec   n_entry+1 record indices: sketch e accumulates records
 *               [entry_rec[e], entry_rec[e+1]) (whole-file mode,
 *               src/niqki_index.cpp:442-456); NULL = one record per sketch
 *               (lines mode, :383-408) and then n_entry must equal n_rec
 *   sketches    n_entry x F int32 out
 * Records with length <= K contribute nothing (:395,:450).  Densification
 * runs once per sketch after all its records (the reference's per-record
 * densification hangs on multi-record files).  Where
 * the reference would never terminate (B.2) the remaining cells stay -1. */
int niqki_sketch(niqki_index *ix, const uint8_t *seqs, const uint64_t *rec_off,
                 uint32_t n_rec, const uint32_t *entry_rec, uint32_t n_entry,
                 int32_t *sketches, int mem);

/* Index::sketch_densification alone (src/niqki_index.cpp:313-331), in place. */
int niqki_densify(niqki_index *ix, int32_t *sketches, uint32_t n, int mem);

/* Index::insert_sketch (src/niqki_index.cpp:362-370) for n sketches; they get
 * genome ids genome_count .. genome_count+n-1 in order, like the id counter of
 * :396-401 / :479-490 does single-threaded. */
int niqki_insert(niqki_index *ix, const int32_t *sketches, uint32_t n, int mem);

/* Number of inserted genomes: Index::getNbGenomes, src/niqki_index.h:138-140 */
uint32_t niqki_genome_count(const niqki_index *ix);

/* Builds the device-resident inverted index (CSR per genome tile) from
 * everything inserted so far.  Replaces the reference's incremental
 * vector<gid> Buckets[] appends (src/niqki_index.h:55, :365-367).  Idempotent;
 * the query calls run it when inserts are pending. */
int niqki_build(niqki_index *ix);

/* Counting half of Index::query_sketch (src/niqki_index.cpp:652-661): for
 * query q, counts[q*stride + g] = number of this shard's slots whose bucket
 * holds genome g.  uint16 counters like the reference's lF<=15 branch.
 * stride >= genome_count (in elements), even; a NIQKI_MEM_DEVICE `counts` must be
 * 4-byte aligned (rows are written as packed u16 pairs).  Fastest when every row
 * starts on a 128-byte line: NIQKI_ROW_STRIDE(genome_count) and a 128-byte aligned
 * buffer (a partial 64-byte block costs HBM a read-modify-write).  This is the
 * per-genome hit vector the multi-GPU path sums across slot shards. */
#define NIQKI_ROW_STRIDE(n) ((((uint64_t)(n)) + 63u) & ~(uint64_t)63u)
int niqki_query_counts(niqki_index *ix, const int32_t *sketches, uint32_t nq,
                       uint16_t *counts, uint64_t stride, int mem);

/* The same with uint32 counters, exact for every S (the reference's lF>15 branch,
 * src/niqki_index.cpp:668-677). */
int niqki_query_counts32(niqki_index *ix, const int32_t *sketches, uint32_t nq,
                         uint32_t *counts, uint64_t stride, int mem);

/* Threshold + order half of Index::query_sketch (src/niqki_index.cpp:662-666,
 * :685): from (possibly cross-shard summed) counters of genomes
 * [gid_begin, gid_begin+n_gids) produce, per query, the (count,gid) pairs with
 * count >= min_score sorted by descending (count, gid).
 *   hit_off     nq+1 exclusive prefix offsets (always exact, even on
 *               NIQKI_E_CAPACITY)
 *   hit_counts, hit_gids   capacity entries each
 * Synchronises the stream when mem == NIQKI_MEM_HOST. */
int niqki_hits_from_counts(niqki_index *ix, const uint16_t *counts, uint32_t nq,
                           uint64_t stride, uint32_t gid_begin, uint32_t n_gids,
                           uint64_t *hit_off, uint32_t *hit_counts,
                           uint32_t *hit_gids, uint64_t capacity, int mem);

/* ---- many host threads on one handle ------------------------------------------------------
 * A handle is single-caller (see the top of this file).  The reference's drivers, however, call
 * compute_sketch / insert_sketch / query_sketch from every thread of an `omp parallel` region on
 * one Index (src/niqki_index.cpp:391-401, :415-428, :479-490, :525-538).  These four entry points
 * keep that contract: any number of host threads may call them on one handle at the same time
 * (and ONLY them, while such calls are in flight).  Concurrent callers are combined into batches --
 * the first thread to arrive leads a batch, threads that arrive while it is on the GPU form the
 * next one -- and each batch runs through niqki_sketch / niqki_insert / niqki_query
 * (NIQKI_MEM_HOST): same results, about one launch per `threads` records instead of one per record.
 *   niqki_sketch_shared           Index::compute_sketch of one record (len bytes) -> sketch[2^S]
 *   niqki_insert_shared           Index::insert_sketch; *genome_id (may be NULL) = the id it got:
 *                                 ids are handed out in arrival order, as the reference's critical
 *                                 section does with several threads (:396-401, :486-490)
 *   niqki_query_shared            Index::query_sketch: *n_hits = number of hits, the first
 *                                 min(*n_hits, capacity) written in the reference's order
 *   niqki_query_sequence_shared   Index::query_sequence (:691-695)
 * (niqki_shared_stats, niqki_hip_bench.h: batches run so far, requests served, the largest batch.) */
int niqki_sketch_shared(niqki_index *ix, const uint8_t *seq, uint64_t len, int32_t *sketch);
int niqki_insert_shared(niqki_index *ix, const int32_t *sketch, uint32_t *genome_id);
int niqki_query_shared(niqki_index *ix, const int32_t *sketch, uint64_t *n_hits, uint32_t *hit_counts,
                       uint32_t *hit_gids, uint64_t capacity);
int niqki_query_sequence_shared(niqki_index *ix, const uint8_t *seq, uint64_t len, uint64_t *n_hits,
                                uint32_t *hit_counts, uint32_t *hit_gids, uint64_t capacity);

/* ---- top-k (niqki_params.top_k, option "top_k") ---------------------------------------------
 * With k > 0, niqki_query, niqki_query_sequences, niqki_staged_query, niqki_query_ahead, niqki_query_shared,
 * niqki_query_sequence_shared, niqki_hits_from_counts (over its [gid_begin, gid_begin + n_gids) range) and the group
 * query calls return per query the first min(k, n) entries of the list they return with k = 0 (n = hits at or above
 * min_score; min_score 0: count-0 genomes are hits).  k >= the genome count is the same as k = 0.  The hits of a batch
 * of nq queries then never exceed nq x k: capacity = nq x k never returns NIQKI_E_CAPACITY.
 * niqki_matrix_range, niqki_query_counts / niqki_query_counts32 and the dump do not look at it. */

/* Index::query_sketch (src/niqki_index.cpp:633-687), batched: both halves. */
int niqki_query(niqki_index *ix, const int32_t *sketches, uint32_t nq,
                uint64_t *hit_off, uint32_t *hit_counts, uint32_t *hit_gids,
                uint64_t capacity, int mem);

/* Index::query_sequence (src/niqki_index.cpp:691-695), batched: sketch +
 * query.  Arguments as niqki_sketch / niqki_query. */
int niqki_query_sequences(niqki_index *ix, const uint8_t *seqs,
                          const uint64_t *rec_off, uint32_t n_rec,
                          const uint32_t *entry_rec, uint32_t n_entry,
                          uint64_t *hit_off, uint32_t *hit_counts,
                          uint32_t *hit_gids, uint64_t capacity, int mem);

/* The same in two halves, so that consecutive batches overlap on the device: niqki_sketch_ahead starts the sketch
 * kernel of a batch on a lane of the handle's own (a side stream) and returns; niqki_query_ahead runs the query of the
 * OLDEST batch sketched ahead on the handle's stream, behind that batch's sketch kernel.  A caller that keeps one batch
 * ahead --
 *     niqki_sketch_ahead(batch 0);
 *     for i: niqki_sketch_ahead(batch i + 1); niqki_query_ahead(hits of batch i);
 * -- has batch i + 1's sketch kernel (bound by vector instruction issue) running beside batch i's gather and hit
 * kernels (bound by HBM): 164 k against 158 k query genomes/s at the 100 000-genome shape.  At most two
 * batches are ahead at a time (NIQKI_E_STATE beyond).  Device memory only, and the one call whose device inputs are NOT
 * taken in the order of the handle's stream: `seqs`, `rec_off` and `entry_rec` are read on the sketch lane, so they must
 * be complete when niqki_sketch_ahead is called and stay untouched until the niqki_query_ahead that takes the batch
 * has been called.  The results of niqki_query_ahead are those of niqki_query_sequences on the same records
 * and, as there, in the handle's stream order for NIQKI_MEM_DEVICE outputs.  `n_entry` (may be NULL) receives the batch's
 * entry count, `sketches` (may be NULL; n_entry x 2^S cells in `mem`) a copy of its sketches.  NIQKI_E_CAPACITY (host
 * outputs) leaves the batch the oldest one: the same call again with larger arrays.  niqki_synchronize waits for the
 * sketch lane too. */
int niqki_sketch_ahead(niqki_index *ix, const uint8_t *seqs, const uint64_t *rec_off, uint32_t n_rec,
                       const uint32_t *entry_rec, uint32_t n_entry, int mem);
int niqki_query_ahead(niqki_index *ix, uint32_t *n_entry, uint64_t *hit_off, uint32_t *hit_counts,
                      uint32_t *hit_gids, uint64_t capacity, int32_t *sketches, int mem);

/* ---- raw file bytes in: FASTA / FASTQ framing on the GPU -------------------
 * Index::Biogetline (src/niqki_index.cpp:890-941) and the read loops of
 * insert_file_whole / query_file_whole (:442-456, :505-519) and
 * insert_file_lines / query_file_lines (:383-430): the caller hands over the
 * bytes of its files (gzip files as they are, see NIQKI_FILE_GZIP below, or inflated), the records are framed on the device and stay
 * there as the "staged batch" of the handle; niqki_staged_* then sketch, insert
 * or query it.  Framing is the reference's: FASTA = the first line of a file and
 * every line starting with '>' is a header, all other lines are concatenated
 * (nothing trimmed or upper-cased); FASTQ = 4-line records.  A record of at most
 * K bases is skipped (:395,:423,:450,:512).  The staged batch stays usable until the
 * next niqki_stage_raw or the next HOST-memory niqki_sketch / niqki_query_sequences
 * on the handle (they share its staging buffers; niqki_staged_* then report
 * NIQKI_E_STATE); every other call leaves it alone. */
typedef struct niqki_raw_batch {
  const uint8_t *raw;        /* bytes of n_files files back to back, in the memory space of the
                                call (device: 4-byte aligned, NIQKI_SEQ_PAD readable bytes after) */
  const uint8_t *const *file_ptr; /* optional (host memory space only): HOST array of n_files host
                                pointers, file f's bytes start at file_ptr[f]; raw is then ignored */
  const uint64_t *file_off;  /* HOST array, n_files+1 offsets into raw (their differences are the
                                file sizes when file_ptr is used) */
  const uint8_t *file_type;  /* HOST array, n_files: 'A' FASTA / 'Q' FASTQ (get_data_type, :944-952); 'a' = a FASTA
                                file handed over as the container niqki_pack_fasta made of it (host memory space, the
                                file_ptr form, whole mode): 2 bits per base across PCIe, the device writes the file's
                                own bytes back before it frames them -- same results as 'A' on the file itself;
                                'A' | NIQKI_FILE_GZIP, 'Q' | NIQKI_FILE_GZIP = the file as it lies on disk, gzip'd (host
                                memory space, the file_ptr form, whole mode): inflated on the device, see below */
  uint32_t n_files;
  uint32_t lines;            /* 0: one sketch per file (whole mode); 1: one sketch per record longer
                                than K (lines mode, n_files must be 1) */
  uint32_t final;            /* lines mode: raw reaches the end of the file; otherwise the last
                                (possibly incomplete) record is left for the next call */
  uint32_t max_entries;      /* lines mode: stop after this many sketches */
  uint8_t *file_status;      /* optional HOST array, n_files, written when the call returns NIQKI_E_GZIP: 0, or why the
                                device would not inflate gzip file f (1..13, nq_kernels.h InflateJob) */
} niqki_raw_batch;

/* Gzip files inflated on the device.  The reference reads every input through zstr::ifstream (src/zstr.hpp:190-203,
 * :236-239: gzip by magic, zlib member after member); a file flagged NIQKI_FILE_GZIP crosses PCIe as it lies on disk
 * (a quarter of its FASTA bytes) and one wavefront per file writes its bytes where the framing expects them.  The
 * device takes what is plainly a gzip file: members that inflate without any irregularity, CRC-32 and ISIZE of every
 * member right, and either ONE member as long as the file's last four bytes say (the usual case), or a file whose
 * members all carry their size -- BGZF (bgzip / htslib: the 'B' 'C' extra subfield) or this project's 'N' 'Q' tag --,
 * which is cut into its members and inflated by one wavefront per member.  For anything else -- damaged or truncated
 * streams, plainly concatenated members, bytes behind the last member, sizes of 2 GiB and more -- niqki_stage_raw stages nothing,
 * returns NIQKI_E_GZIP and names the files in file_status; the caller inflates those itself (zlib decides what they
 * yield, as before) and hands them over as 'A' / 'Q'.  The kernel is at least as strict as zlib's inflate, so a file
 * it accepts has zlib's bytes. */
#define NIQKI_FILE_GZIP 0x80

typedef struct niqki_stage_info {
  uint32_t n_entry;    /* sketches the staged batch produces */
  uint32_t n_rec;      /* records framed, short ones included */
  uint64_t consumed;   /* raw bytes covered by the entries: a lines-mode stream resumes here
                          (always the first byte of a header line, or the end) */
  uint64_t seq_bytes;  /* sequence bytes staged */
} niqki_stage_info;

/* entry_hdr (HOST array of max_entries, lines mode, may be NULL): raw offset of the
 * header line of each entry (names are the header lines, :395-400). */
int niqki_stage_raw(niqki_index *ix, const niqki_raw_batch *batch, int mem_space,
                    niqki_stage_info *info, uint64_t *entry_hdr);
/* Starts the host-to-device copy of the NEXT batch's file bytes (file_ptr form, whole mode) on a
 * copy stream of the handle and returns without waiting: the copy runs beside the kernels of the
 * batch staged now (the read loops of :461-500 / :523-540 with the transfer of file i+1 under the
 * work on file i).  A niqki_stage_raw(NIQKI_MEM_HOST) whose batch names the same file_ptr[] and
 * file_off[] takes these bytes instead of copying.  Two prefetches may be on their way at a time (the
 * batch about to be staged and the one behind it: a third takes the older one's place); staging
 * one of them leaves the other alone, staging any other batch drops both.  The
 * caller keeps the host bytes valid until that call returns (page-locked memory, or the copy is
 * not asynchronous). */
int niqki_stage_raw_prefetch(niqki_index *ix, const niqki_raw_batch *batch);
/* compute_sketch of every staged entry (n_entry x 2^S int32). */
int niqki_staged_sketch(niqki_index *ix, int32_t *sketches, int mem_space);
/* ... + insert_sketch: ids follow the entries (:396-401, :479-490). */
int niqki_staged_insert(niqki_index *ix);
/* ... + query_sketch per entry; outputs as niqki_query. */
int niqki_staged_query(niqki_index *ix, uint64_t *hit_off, uint32_t *hit_counts,
                       uint32_t *hit_gids, uint64_t capacity, int mem_space);
/* Packed FASTA: what a host-to-device copy of whole genomes costs is 1 byte per base; a FASTA file is almost
 * entirely full lines of one width holding A, C, G, T only.  niqki_pack_fasta turns the bytes of a file into a
 * container in which every run of such lines travels as 2 bits per base and everything else -- header lines, lines
 * with any other byte, a last line without its newline -- verbatim; staged with file_type 'a', the device restores
 * the file's exact bytes (so Index::Biogetline's framing, src/niqki_index.cpp:890-941, sees what it would have seen).
 * Host code, no device needed.  niqki_pack_fasta returns the container's size, or 0 when the file is not worth
 * packing (reads, FASTQ, CRLF lines: hand it over raw); capacity >= niqki_pack_bound(n).  niqki_unpack_fasta is the
 * host restatement of the device pass (raw == NULL: only *raw_len). */
size_t niqki_pack_bound(size_t n);
size_t niqki_pack_fasta(const uint8_t *raw, size_t n, uint8_t *out, size_t capacity);
int niqki_unpack_fasta(const uint8_t *container, size_t len, uint8_t *raw, size_t capacity, size_t *raw_len);
/* Page-locked host memory for raw batches (plain malloc'ed memory works too, slower). */
void *niqki_host_alloc(size_t bytes);
void niqki_host_free(void *p);

/* Counting loop of Index::query_range (src/niqki_index.cpp:570-597): for
 * target genomes t in [begin,end), counts[(t-begin)*stride + a] = number of
 * buckets holding both a and t (the reference's counts[a*batch + t-begin];
 * the matrix is symmetric).  uint16 like :572. */
int niqki_matrix_range(niqki_index *ix, uint32_t begin, uint32_t end,
                       uint16_t *counts, uint64_t stride, int mem);

/* ---- self-join: the index asked about itself ------------------------------------------------
 * Whole-range single-GPU handles only (resident or paged, any tile count, hit lists or counter rows, S <= 16, with or
 * without a delta segment).  A slot-range shard (niqki_params.slot_begin / slot_end) sees partial counts: both calls
 * return NIQKI_E_STATE on it.  Groups have no self-join (out of scope: build a single-GPU index for it).
 *
 * Sparse form of Index::query_range (src/niqki_index.cpp:570-610): the hits of the STORED sketches of genomes
 * [begin, end).  Defined as: exactly what niqki_query returns for the output of
 * niqki_get_sketches(ix, begin, end - begin, ...) -- same threshold (the handle's min_score), same order and tie
 * rule, top_k honoured, the genome itself included where its own count passes the threshold -- without the
 * sketches leaving the device.  Capacity protocol and mem as niqki_query (NIQKI_MEM_DEVICE: one launch round for the
 * whole range, no capacity check; NIQKI_MEM_HOST: batches of option "query_batch", NIQKI_E_CAPACITY with the true
 * total in hit_off[end - begin]).  begin > end or end > genome count: NIQKI_E_INVALID. */
int niqki_neighbors_range(niqki_index *ix, uint32_t begin, uint32_t end, uint64_t *hit_off,
                          uint32_t *hit_counts, uint32_t *hit_gids, uint64_t capacity, int mem);

/* Single-linkage clusters of the indexed genomes: a and b are linked when their co-occurrence count (the cell
 * niqki_matrix_range gives, before any u16 wrap) is >= threshold; a cluster is a connected component of that
 * graph.  labels[g] = the SMALLEST genome id of g's cluster, for every g in [0, n_genomes).  *n_clusters (may be
 * NULL, host memory whatever mem is) = number of g with labels[g] == g.  The result is a function of the index and the
 * threshold only: it does not depend on batch sizes, options, top_k (ignored here) or the order in which the device
 * links pairs.  threshold 0 links everything: all labels 0, nothing is launched.  The handle's min_score and top_k are
 * unchanged when the call returns, also when it fails.
 * The pair list never leaves the device: per batch of option "query_batch" stored sketches the hits at the threshold
 * stay in device buffers of a fixed budget (option "cluster_ws_mib", default 1024; a batch whose hits exceed it is
 * split in halves, down to one query, whose hits always fit; stat "cluster_splits" counts the splits of the last
 * call) and a link kernel unites the components on a device-resident parent array.
 * While profiling is on (niqki_profile_enable, niqki_hip_bench.h) the call also times its phases with events, one
 * synchronisation per batch; niqki_get_stat then gives, for the last call: "cluster_us_read" (stored sketches back
 * into query form), "cluster_us_hits" (gather + threshold + order), "cluster_us_link", "cluster_us_flatten"
 * (microseconds) and "cluster_pairs" (hits the link kernel went through; tools/bench_selfjoin.py). */
int niqki_cluster(niqki_index *ix, uint32_t threshold, uint32_t *labels, uint32_t *n_clusters, int mem);

/* Dereplication: greedy representatives of the indexed genomes, in INDEX ORDER.  count(a, b) is the co-occurrence count
 * of the stored sketches (the cell niqki_matrix_range gives, before any u16 wrap); a and b are linked when
 * count(a, b) >= threshold.
 *   1. genome t is a representative iff no representative g < t is linked to t;
 *   2. labels[t] = t for a representative; for any other genome the linked representative r (of any index position,
 *      also r > t) with the largest count(t, r), among equal counts the smallest r.  One exists by rule 1.
 * So no two representatives are linked, every other genome is linked to its label, and every label is a
 * representative (single linkage, niqki_cluster, promises none of that: its clusters chain).  labels[g] for every g
 * in [0, n_genomes); label_counts (may be NULL) [g] = count(g, labels[g]), 0 for a representative;
 * *n_representatives (may be NULL, host memory whatever mem is) = number of g with labels[g] == g.  mem as in
 * niqki_cluster: NIQKI_MEM_DEVICE takes labels / label_counts as device arrays and copies nothing.
 * The result is a function of the index and the threshold only: it does not depend on batch sizes, options, top_k
 * (ignored here) or the order in which the device decides.  threshold 0 links everything: genome 0 is the only
 * representative (only genome 0's list is made, for label_counts).  No genomes: 0 representatives.  The handle's
 * min_score and top_k are unchanged when the call returns, also when it fails.  Handles as niqki_cluster
 * (NIQKI_E_STATE on a slot-range shard).
 * The pair list never leaves the device: the batches, the hit buffers, their budget (option "cluster_ws_mib") and the
 * halving rule are niqki_cluster's (stat "derep_splits": the splits of the last call).  Per batch, in index order,
 * decide rounds settle who is a representative -- a genome waits while a linked genome below it is undecided, so a
 * batch may need several rounds (a path in index order: as many as it has genomes); stat "derep_rounds" = the most
 * rounds one batch of the last call needed -- then every new representative offers itself to the genomes of its list
 * with one 64-bit atomic maximum each.  Device state: 13 bytes a genome.
 * While profiling is on the call times its phases with events, one synchronisation per batch: "derep_us_read",
 * "derep_us_hits", "derep_us_decide", "derep_us_assign" (microseconds) and "derep_pairs" (hits the batches held). */
int niqki_dereplicate(niqki_index *ix, uint32_t threshold, uint32_t *labels, uint32_t *label_counts,
                      uint32_t *n_representatives, int mem);

/* Dereplication that takes the genomes below `first` as given (a database update: which of the genomes added behind
 * `first` does the collection not represent yet?).  Arguments, mem, stats ("derep_*": the last call of either entry
 * point) and the restored min_score / top_k as niqki_dereplicate; rule 1 is replaced:
 *   0. every genome g < first is a representative, whatever it is linked to;
 *   1. a genome t >= first is a representative iff no representative g < t, given or new, is linked to t;
 *   2. labels / label_counts as above for t >= first (the linked representative with the largest count, ties to the
 *      smallest id, later ones count too); labels[g] = g and label_counts[g] = 0 for every g < first.
 * first = 0 is niqki_dereplicate, bit for bit.  first >= the genome count: everything is a representative and nothing
 * is launched.  Only the hit lists of the genomes [first, n) are made: the self-join batches start at `first`, and
 * since the given representatives have no lists of their own, each batch reads their offers off its own lists
 * (counts are symmetric). */
int niqki_dereplicate_from(niqki_index *ix, uint32_t first, uint32_t threshold, uint32_t *labels,
                           uint32_t *label_counts, uint32_t *n_representatives, int mem);

/* The complete single-linkage hierarchy of the indexed genomes, and the spanning forest it is, in ONE self-join: what
 * niqki_cluster answers at one threshold, for every threshold >= floor.
 * Definitions.  count(a, b) is the co-occurrence count of the stored sketches (the cell niqki_matrix_range gives,
 * before any u16 wrap; at S = 16 the exact sum of the two planes).  labels_t[g] is what niqki_cluster(ix, t) returns.
 * Edge order: undirected pairs lo < hi are strictly ordered by (1) the larger count first, (2) among equal counts the
 * smaller lo, (3) then the smaller hi.
 * Forest: the unique maximum spanning forest, under that order, of the graph whose edges are the pairs with
 * count >= max(floor, 1) -- what Kruskal keeps when it takes the edges in that order.  edge_lo / edge_hi /
 * edge_count[0 .. n_edges) hold it in that order, n_edges = N - *n_roots; the arrays have N places each, the places
 * from n_edges on are not written.
 * Hierarchy: for every genome g, merge_count[g] is the largest t >= max(floor, 1) with labels_t[g] != g and
 * merge_into[g] is labels_t[g] at that t.  If there is no such t (g is the smallest id of its component at the floor)
 * merge_into[g] = g and merge_count[g] = 0.  merge_into[g] < g whenever it differs from g, and a child's merge_count
 * is strictly larger than its parent's.  labels_t for every t >= max(floor, 1) is read off the two arrays: from g,
 * follow merge_into while merge_count >= t (and merge_into differs).
 * floor = 0: the result of floor = 1, and then every remaining root r > 0 joins genome 0 at count 0: edges (0, r, 0)
 * in ascending r at the end of the list, merge_into[r] = 0, merge_count[r] = 0, *n_roots = 1 (canonical under the
 * edge order: the count-0 pairs come last, and (0, r) is the first of them that joins r).
 * The result is a function of the index and floor only: it does not depend on batch sizes, options, top_k (ignored),
 * tile count, paging, a delta segment or the order in which the device links.  The handle's min_score and top_k are
 * unchanged when the call returns, also when it fails.  Handles as niqki_cluster: whole-range single-GPU handles,
 * resident or paged, any tile count, with or without a delta segment, S <= 16; NIQKI_E_STATE on a slot-range shard.
 * More than 2^23 genomes: NIQKI_E_INVALID (an edge is one 64-bit key with 23 bits an id; niqki_last_error says so).
 * No genomes: NIQKI_OK, *n_roots = 0.  merge_into and merge_count may both be NULL, the three edge arrays may all be
 * NULL, n_roots (host memory whatever mem is) may be NULL.  mem as in niqki_cluster: with NIQKI_MEM_DEVICE the five
 * arrays are device arrays, written in stream order; the call synchronises.
 * One self-join: the batches, the hit buffers, their budget (option "cluster_ws_mib") and the halving rule are
 * niqki_cluster's.  The device keeps a forest of fewer than N edges; per batch Boruvka rounds (offers with a 64-bit
 * atomic maximum per component, hooks, pointer jumping) make the forest of the old forest and the batch's pairs; after
 * the last batch the forest crosses to the host once, is sorted, and a union-find over its levels gives the hierarchy
 * (DESIGN.md 4.6g).  Device state: 28 bytes a genome.
 * niqki_get_stat, the last call: "linkage_rounds" (the most rounds in which a batch hooked components),
 * "linkage_splits", "linkage_pairs" (hits the batches held); while profiling is on, with one synchronisation per
 * batch: "linkage_us_read", "linkage_us_hits", "linkage_us_forest", "linkage_us_finish" (microseconds; the last one
 * by the host's clock: copy, sort, hierarchy, results). */
int niqki_linkage(niqki_index *ix, uint32_t floor, uint32_t *merge_into, uint32_t *merge_count,
                  uint32_t *edge_lo, uint32_t *edge_hi, uint32_t *edge_count, uint32_t *n_roots, int mem);

/* Label audit: every indexed genome's nearest neighbours read against the labelling of niqki_set_labels -- the
 * leave-one-out k-nearest-neighbour check of a curated collection, in ONE self-join.  A label file is trusted by
 * niqki_query_collapsed, niqki_unite and, as the leaves of a taxonomy, niqki_query_lca; this call says which genomes
 * the index itself would have labelled otherwise, before the file is acted on.
 * Definition.  label[g] is the labelling of niqki_set_labels.  t = max(threshold, 1).  H(g) is exactly what
 * niqki_neighbors_range(ix, g, g + 1, ...) returns at min_score = t and top_k = 0: ordered by count descending, then
 * gid descending.  H'(g) is H(g) without the entry whose gid is g; that entry is absent when g's own valid cells are
 * fewer than t, and it is not the first one when an exact duplicate with a larger id ties it.  For every g in
 * [0, n_genomes):
 *   own_count[g], own_gid[g]      the first entry of H'(g) whose label equals label[g]; none: 0, 0xFFFFFFFF.
 *   other_count[g], other_gid[g]  the first entry of H'(g) whose label differs from label[g]; none: 0, 0xFFFFFFFF.
 *   vote_gid[g], vote_n[g]        V is the first min(k, |H'(g)|) entries of H'(g).  The winning label is the one with
 *                                 the most entries in V, among equal numbers the one whose first entry in V comes
 *                                 first; vote_gid is that first entry's gid, vote_n the label's number of entries in
 *                                 V.  V empty: 0xFFFFFFFF, 0.  k = 1: simply the nearest neighbour.
 *   verdict[g]                    set by the two counts alone:
 *                                 NIQKI_AUDIT_ALONE      both counts 0
 *                                 NIQKI_AUDIT_AGREES     own_count > other_count
 *                                 NIQKI_AUDIT_TIED       own_count == other_count > 0
 *                                 NIQKI_AUDIT_MISPLACED  other_count > own_count > 0
 *                                 NIQKI_AUDIT_STRAY      other_count > 0 == own_count
 * Each of the seven arrays may be NULL.  k must be in 1..63, else NIQKI_E_INVALID (the first k + 1 entries of a list
 * are one wavefront's load).  Without a labelling the call returns NIQKI_E_STATE and niqki_last_error says to call
 * niqki_set_labels (again); no genomes: NIQKI_OK, also without a labelling.  The result is a function of the index, the
 * labels, t and k only: it does not depend on batch sizes, options, splits, top_k (ignored here) or the order in which
 * the device works.  The handle's min_score and top_k are unchanged when the call returns, also when it fails.
 * Handles as niqki_cluster: whole-range single-GPU handles, resident or paged, any tile count, hit lists or counter
 * rows, with or without a delta segment; NIQKI_E_STATE on a slot-range shard.  Groups have no audit.  mem as in
 * niqki_cluster: with NIQKI_MEM_DEVICE the arrays are device arrays of n_genomes words, written in place in stream
 * order; host results go through one device workspace of 7 x n_genomes words and cross once, at the end.  The call
 * synchronises.
 * One self-join: the batches, the hit buffers, their budget (option "cluster_ws_mib") and the halving rule are
 * niqki_cluster's.  Per batch the audit kernel takes a list per wavefront, 64 entries a step: it drops g's own entry
 * with a ballot and a prefix count of lanes, lets the first k lanes' labels be compared by all lanes (a popcount a
 * label) and finds the first own-label and the first foreign entry by ballots, until both are known or the list ends;
 * the verdict is computed there and nowhere else.  Nothing is sorted, nothing spins.
 * niqki_get_stat, the last call: "audit_splits", "audit_pairs" (hits the batches held); while profiling is on, with
 * one synchronisation per batch: "audit_us_read", "audit_us_hits", "audit_us_scan" (microseconds;
 * tools/bench_audit.py). */
#define NIQKI_AUDIT_ALONE 0
#define NIQKI_AUDIT_AGREES 1
#define NIQKI_AUDIT_TIED 2
#define NIQKI_AUDIT_MISPLACED 3
#define NIQKI_AUDIT_STRAY 4
int niqki_audit(niqki_index *ix, uint32_t threshold, uint32_t k, uint32_t *verdict, uint32_t *own_count,
                uint32_t *own_gid, uint32_t *other_count, uint32_t *other_gid, uint32_t *vote_gid, uint32_t *vote_n,
                int mem);

/* Greedy cover of a query: the non-redundant form of niqki_query's answer.  A sample that holds several genomes, or an
 * index with many close relatives of one genome, makes niqki_query list every relative; the cover lists, pick after
 * pick, the genome that explains the most query slots nothing picked before it explains.
 * Let Q be a query sketch and G_g the stored sketch of genome g, as niqki_get_sketches returns it.  A cell v is valid
 * when 0 <= v < 2^W (the rule of Index::query_sketch, src/niqki_index.cpp:639).
 *   R_0 = {s : Q[s] valid};  total(g) = |{s in R_0 : G_g[s] == Q[s]}|, the count niqki_query reports.
 *   Round r = 1, 2, ...:  c_r(g) = |{s in R_(r-1) : G_g[s] == Q[s]}|;  g_r = the genome with the largest c_r, among
 *   equal counts the LARGEST id -- by definition the first hit niqki_query returns for Q with every cell outside
 *   R_(r-1) set to -1.  The cover ends before round r when c_r(g_r) < max(min_score, 1) (the handle's min_score) or
 *   when r > max_picks (max_picks = 0: no limit).  Otherwise pick r is (count c_r(g_r), gid g_r, total(g_r)) and
 *   R_r = R_(r-1) minus the slots where G_(g_r) matches.
 * Consequences: counts never increase from pick to pick; no genome is picked twice; the counts of a query's picks sum
 * to at most |R_0|; a query has at most min(N, |R_0| / max(min_score, 1)) picks.  The result is a function of the
 * index, Q, min_score and max_picks only: batch sizes, options, tile count, a delta segment and the handle's top_k
 * (ignored here) do not change it.  min_score and top_k are the handle's own again when the call returns, also when
 * it fails.
 * Outputs as niqki_query's: hit_off holds nq + 1 offsets, a query's picks appear in pick order in hit_counts (the
 * slots the pick newly explains), hit_gids and hit_totals (total(g); may be NULL).  In BOTH memory spaces a total
 * above `capacity` returns NIQKI_E_CAPACITY with the true total in hit_off[nq] and nothing written to the other
 * arrays; capacity = nq x max_picks never fails when max_picks > 0.  NIQKI_MEM_HOST works in batches of option
 * "query_batch"; NIQKI_MEM_DEVICE takes the nq sketches as one batch and writes in stream order.
 * niqki_staged_cover works on the sketches of the staged batch (niqki_stage_raw) and leaves it usable: a
 * niqki_staged_query after it answers as if it had not run.
 * Handles: whole-range, single-GPU, resident handles; any tile count, hit lists or counter rows, with or without a
 * delta segment, S <= 16.  A slot-range shard gets NIQKI_E_STATE, and so does a paged handle (resident_bytes /
 * resident_mib; niqki_last_error says so): its store is host memory, and a column read per pick across the bus is not
 * a form worth having -- refused, never answered differently.  Groups have no cover.  No genomes, nq = 0 or a sketch
 * without a valid cell: NIQKI_OK and no picks.
 * How: per batch the device keeps the sketches as given, a working copy and the list of active queries.  A round runs
 * the query path itself (threshold max(min_score, 1), top_k = 1) on the active queries' working rows, so every count
 * and every tie is niqki_query's; then one workgroup per active query walks the winner's column of the sketch store,
 * counts total against the sketch as given, sets the matching cells of the working row to -1 and logs the pick; the
 * rows of the queries that go on are moved together, in query order, so later rounds cost less.  The host reads the
 * active count back once per round -- the round's only synchronisation -- and ends the call with NIQKI_E_STATE (never
 * a spin) if a pick masked no cell or the rounds pass min(N, F / max(min_score, 1), max_picks if nonzero) + 1.
 * niqki_get_stat, the last call: "cover_rounds" (the most rounds a batch ran), "cover_picks",
 * "cover_recount_mismatches" (the sum over picks of |cells masked - count reported|: 0 unless there is a bug); while
 * profiling is on: "cover_us_hits", "cover_us_pick", "cover_us_compact", "cover_us_finish" (microseconds).
 * DESIGN.md 4.5c. */
int niqki_cover(niqki_index *ix, const int32_t *sketches, uint32_t nq, uint32_t max_picks, uint64_t *hit_off,
                uint32_t *hit_counts, uint32_t *hit_gids, uint32_t *hit_totals, uint64_t capacity, int mem);
int niqki_staged_cover(niqki_index *ix, uint32_t max_picks, uint64_t *hit_off, uint32_t *hit_counts,
                       uint32_t *hit_gids, uint32_t *hit_totals, uint64_t capacity, int mem);

/* Collapsed hits: per query the best hit of every LABEL.  A collection with a species label per genome (from a
 * taxonomy table, or the labels niqki_cluster / niqki_dereplicate return) answers "which species, and how close is its
 * best member" without the full lists (nq x relatives entries) ever leaving the device.
 * niqki_set_labels gives every indexed genome g a label[g], any uint32_t: values are arbitrary and need not be dense, 0
 * and 0xFFFFFFFF are ordinary labels.  n must equal niqki_genome_count (else NIQKI_E_INVALID, the labelling the handle
 * had stays); labels == NULL or n == 0 removes the labelling.  mem as in niqki_cluster: a device array is taken in
 * stream order; the call may synchronise once.  The call prepares what the kernel needs -- dense label ids, a rank
 * among the distinct values -- and stat "labels" = the number of distinct labels (0 when none is set); this is one-off
 * work and runs on the host.  The labelling belongs to a genome set: every call that adds or drops genomes removes it
 * (niqki_insert, niqki_insert_shared, niqki_staged_insert of at least one genome; a committed niqki_append_*;
 * niqki_retain, whatever its flags).  Without a labelling the collapsed calls return NIQKI_E_STATE and
 * niqki_last_error says to set labels again.  Plain queries and every other call never look at the labelling.
 * Definition.  For a query sketch Q let H(Q) be the list niqki_query returns for Q with top_k = 0 at the handle's
 * min_score: ordered by count descending, then gid descending (min_score 0: every genome is a hit).  The collapsed
 * list of Q is the subsequence of H(Q) made of the entries that are the first of their label in H(Q), in H(Q)'s order.
 * Each carries count and gid of that entry (the label's best member, ties to the larger gid because that is H's order)
 * and members, the number of entries of H(Q) with that label; members never depends on top_k.  With the handle's
 * top_k = k > 0 the result is the first min(k, n) entries of the collapsed list: top_k bounds LABELS.
 * Consequences: every genome its own label gives H(Q) itself, with members 1; one label for all gives at most one
 * entry per query, with members = |H(Q)|; a query's members sum to |H(Q)| when top_k = 0.  The result is a function
 * of the index, the labels, Q, min_score and top_k only: batch size, options, tile count, paging, a delta segment and
 * the hit-list versus counter-row form do not change it.  The handle's min_score and top_k are its own again when the
 * call returns, also when it fails.
 * Outputs as niqki_cover's: hit_off holds nq + 1 offsets; hit_counts, hit_gids and hit_members (may be NULL) hold the
 * entries in list order.  In BOTH memory spaces a total above `capacity` returns NIQKI_E_CAPACITY with the true total
 * in hit_off[nq] and nothing written to the other arrays; capacity = nq x min(top_k or "labels", "labels") never
 * fails.  NIQKI_MEM_HOST works in batches of option "query_batch"; NIQKI_MEM_DEVICE takes the nq sketches in one call
 * and writes in stream order.  niqki_staged_query_collapsed works on the staged batch (niqki_stage_raw) and leaves it
 * usable: a niqki_staged_query after it answers as if it had not run.
 * Handles: whole-range single-GPU handles, resident or paged, any tile count, hit lists or counter rows, with or
 * without a delta segment, S <= 16 (at S = 16 counts reach 65 536; the outputs are u32).  A slot-range shard gets
 * NIQKI_E_STATE.  Out of scope: multi-GPU groups, the _shared calls and the _ahead calls have no collapsed form.  No
 * genomes, nq = 0 or a query without a hit: NIQKI_OK and empty lists (no genomes: also without a labelling, which an
 * empty index cannot have).
 * How: per batch the query path itself runs at top_k = 0 into the handle's device hit buffers, whose budget is option
 * "cluster_ws_mib" with the halving rule of niqki_cluster (a batch whose full lists do not fit is split in halves,
 * down to one query, whose list always fits; stat "collapse_splits").  collapse_first_kernel then takes a query per
 * workgroup: a list of at most L entries (option "collapse_lds_cap", 1..4096, default 1024: a 24 KiB table, six
 * workgroups a compute unit) goes through an open-addressing table in LDS keyed by the dense label id -- per entry an
 * atomic minimum on the label's first position and an atomic add on its member count, at least 2 L slots, linear
 * probing bounded by the table size -- and a longer list through a direct-indexed table in global memory, one per
 * resident workgroup (labels x 8 bytes each, as many as a quarter of the budget holds, 1 .. 1024), which is cleared by
 * walking the list again; stat "collapse_long_lists" counts the queries of the last call on that route.  An entry is
 * kept iff its position is its label's first; a scan of the kept counts, cut to top_k, and a scatter in list order
 * finish the batch.  Nothing is sorted, nothing spins, and the kept total is read back once per batch (4 more bytes a
 * hit than the hit buffers for the flags).  While profiling is on: "collapse_us_hits", "collapse_us_first",
 * "collapse_us_emit" (microseconds, the last call).  DESIGN.md 4.5d. */
int niqki_set_labels(niqki_index *ix, const uint32_t *labels, uint32_t n, int mem);
int niqki_query_collapsed(niqki_index *ix, const int32_t *sketches, uint32_t nq, uint64_t *hit_off,
                          uint32_t *hit_counts, uint32_t *hit_gids, uint32_t *hit_members, uint64_t capacity, int mem);
int niqki_staged_query_collapsed(niqki_index *ix, uint64_t *hit_off, uint32_t *hit_counts, uint32_t *hit_gids,
                                 uint32_t *hit_members, uint64_t capacity, int mem);

/* Containment search: per query the hits whose SHARE reaches a threshold, ordered by it.  A Jaccard index is the wrong
 * number for a part against a whole -- a 64 F-k-mer piece of a 256 F-k-mer genome has J near 0.25 with it although every
 * k-mer of the piece is in the genome -- and niqki_registers only annotates a list that min_score and the count have
 * already chosen and ordered.  These calls select by the share, order by it and cut to top_k on the device, so a
 * batch's output stays bounded by nq x top_k.
 * Sizes.  A size is a uint64_t number of distinct k-mers; 0 means "no usable size"; sizes are below 2^40, a larger one
 * is NIQKI_E_INVALID.  niqki_set_sizes gives every indexed genome g its size[g] and follows niqki_set_labels in every
 * respect: n must equal niqki_genome_count (else NIQKI_E_INVALID, the sizes the handle had stay; so they do when a size
 * does not fit); sizes == NULL or n == 0 removes them; a device array is taken in stream order and the call may
 * synchronise once; the sizes belong to a genome set, so every call that adds or drops genomes removes them (the calls
 * named under niqki_set_labels, and niqki_unite).  They are independent of labels and taxonomy.  Stat "sizes" = n, or
 * 0.  The caller supplies the numbers: the host program takes them from niqki_registers and its estimator, another
 * caller may know exact ones.
 * Share.  For a hit with count c (0 <= c <= F = 2^S, S <= 16), query size q, genome size g and a mode: d = q for
 * NIQKI_CONTAIN_QUERY (the share of the query's k-mers found in the genome), d = g for NIQKI_CONTAIN_GENOME, d = min(q, g)
 * for NIQKI_CONTAIN_MAX (the larger of the two shares).  Nn = c (q + g), Dd = (F + c) d -- that is |A n B| =
 * J (|A| + |B|) / (1 + J) with J = c / F, over d; both products are below 2^57.  share = 0xFFFFFFFF if Nn >= Dd, else
 * floor(Nn 2^32 / Dd).  NIQKI_CONTAIN_ONE = 0xFFFFFFFF stands for a share of 1.  Integers only, checked bit for bit:
 * 32 rounds of "double Nn; if Nn >= Dd, subtract and set the bit" in 64-bit arithmetic (nq_contain_share.h).  A hit is
 * UNSIZED when q == 0 or g == 0.
 * Result.  H(Q) is the list niqki_query returns for Q at the handle's min_score with top_k = 0: count descending, then
 * gid descending.  The contained list C(Q): drop the unsized entries of H(Q); keep those with share >= min_share;
 * order by share descending, ties in the order they have in H(Q) (a stable sort: with equal sizes C(Q) is a sub-list of
 * H(Q) in H's order).  The handle's top_k (0 = all) keeps the first top_k entries of C(Q).  n_unsized[Q] (may be NULL) is
 * the number of unsized entries of H(Q).  The result depends only on the index, the sizes, qsizes, mode, min_share,
 * min_score and top_k: batch sizes, splits, tile count, paging, a delta segment, hit lists against counter rows and the
 * order in which the device works do not change it.
 * min_score IS THE FLOOR: a genome whose count is below it is never seen, whatever its share.  Lower min_score to what
 * the smallest share of interest needs (a part of a tenth of a genome has J near 0.1 with it).
 * Outputs as niqki_query_collapsed's: hit_off holds nq + 1 offsets; hit_shares, hit_counts and hit_gids hold the entries
 * in C's order.  qsizes has nq entries (the staged form: one per staged entry) and lives in the same memory space as
 * the outputs.  In both spaces a total above `capacity` returns NIQKI_E_CAPACITY with the true total in hit_off[nq] and
 * nothing promised of the other arrays; capacity = nq x top_k never fails.  NIQKI_MEM_HOST works in batches of option
 * "query_batch"; NIQKI_MEM_DEVICE takes the nq sketches in one batch and writes in stream order (a device qsizes entry
 * of 2^40 or more ends the call with NIQKI_E_INVALID when the kernel meets it).  The staged form leaves the staged batch
 * usable.  The handle's min_score and top_k are its own again on every exit.
 * Handles as niqki_query_collapsed: whole-range single-GPU handles, resident or paged, any tile count, lists or rows,
 * with or without a delta segment, S <= 16; a slot-range shard gets NIQKI_E_STATE.  A mode above 2: NIQKI_E_INVALID.
 * Without sizes on a non-empty index: NIQKI_E_STATE, and niqki_last_error says to call niqki_set_sizes (again).  No
 * genomes or nq = 0: NIQKI_OK with zero offsets.  Groups, the _shared calls and the _ahead calls have no such form.
 * How: per batch the query path runs at top_k = 0 into the handle's hit buffers (option "cluster_ws_mib", halved like
 * niqki_cluster's batches; stat "contain_splits").  contain_share_kernel, a workgroup of 256 per query, gathers
 * size[gid], computes the shares and compacts the survivors in list order; contain_order_kernel orders up to 2048
 * survivors as keys share << 32 | (0xFFFFFFFF - position) under the bitonic network of the hit kernels, and more by four
 * stable 8-bit radix passes of one wave (stat "contain_long_lists": the queries of the last call on that route); a scan
 * of the kept counts and an emit that fetches count and gid by position finish the batch.  8 more bytes a hit than the
 * hit buffers.  While profiling is on: "contain_us_hits", "contain_us_share", "contain_us_order" (microseconds, the last
 * call).  DESIGN.md 4.5h. */
#define NIQKI_CONTAIN_QUERY 0u
#define NIQKI_CONTAIN_GENOME 1u
#define NIQKI_CONTAIN_MAX 2u
#define NIQKI_CONTAIN_ONE 0xFFFFFFFFu
int niqki_set_sizes(niqki_index *ix, const uint64_t *sizes, uint32_t n, int mem);
int niqki_query_contained(niqki_index *ix, const int32_t *sketches, const uint64_t *qsizes, uint32_t nq, uint32_t mode,
                          uint32_t min_share, uint64_t *hit_off, uint32_t *hit_shares, uint32_t *hit_counts,
                          uint32_t *hit_gids, uint32_t *n_unsized, uint64_t capacity, int mem);
int niqki_staged_query_contained(niqki_index *ix, const uint64_t *qsizes, uint32_t mode, uint32_t min_share,
                                 uint64_t *hit_off, uint32_t *hit_shares, uint32_t *hit_counts, uint32_t *hit_gids,
                                 uint32_t *n_unsized, uint64_t capacity, int mem);

/* Taxon of a query: the lowest common ancestor (LCA) of its near-best hits, the rule of Kraken and MEGAN.  Labels are
 * flat; a collection also says that species X lies in genus Y and Y in family Z, and what a read classifier asks of
 * the index is ONE taxon per query: the species when the best hits all lie in it, the genus when several of its
 * species are hit equally well.  The result is one fixed-size row per query; nothing per hit leaves the device.
 * niqki_set_taxonomy.  Taxa are the dense ids 0 .. n_taxa - 1.  parent[t] is t's parent; parent[t] == t makes t a root,
 * and several roots form a forest.  genome_taxon[g] is the taxon of indexed genome g; interior taxa may carry genomes,
 * and a taxon nothing refers to is fine.  n_genomes must equal niqki_genome_count; every genome_taxon[g] and parent[t]
 * must be below n_taxa; n_taxa < 0xFFFFFFFE; following parent from any taxon must reach a root (no cycle other than a
 * root's self-loop).  Any breach returns NIQKI_E_INVALID, niqki_last_error names the offending genome or taxon, and
 * the taxonomy the handle had stays.  genome_taxon == NULL, parent == NULL or n_taxa == 0 removes the taxonomy.  mem as
 * in niqki_set_labels: both arrays live in that space; the call may synchronise once.  Validation and the depth of
 * every taxon (a root has depth 0) are one-off work on the host; the device keeps one 8-byte node {parent, depth} per
 * taxon and genome_taxon.  Stat "taxa" = n_taxa (0 when no taxonomy is set), stat "taxonomy_depth" = the largest
 * depth.  The taxonomy is independent of niqki_set_labels -- neither call disturbs the other -- and belongs to a
 * genome set in the same way: every call that drops the labelling drops the taxonomy.  Without one the two query
 * calls return NIQKI_E_STATE and niqki_last_error says to set it again (no genomes: NIQKI_OK also without one).
 * Definition.  H(Q) is the list niqki_query returns for Q with top_k = 0 at the handle's min_score: count descending,
 * then gid descending (min_score 0: every genome is a hit).  H(Q) empty: taxon = NIQKI_TAXON_NONE, best_count = 0,
 * best_gid = 0xFFFFFFFF, considered = 0.  Otherwise best_count and best_gid are H(Q)'s first entry, and the CONSIDERED
 * hits are the entries with count * 1000 >= best_count * (1000 - top_permille), in 64-bit arithmetic, equality
 * included.  H is ordered, so they are a prefix of H(Q) and `considered` is its length.  top_permille = 0: only the
 * ties with the best hit; 1000: every hit; above 1000: NIQKI_E_INVALID.  taxon is the deepest taxon that is an
 * ancestor-or-self of genome_taxon[g] for every considered g, and NIQKI_TAXON_NONE when the considered hits lie in
 * more than one tree (told from "no hit" by considered >= 2).  The handle's top_k is ignored; min_score and top_k are
 * the handle's own again when the call returns, also when it fails.  The result is a function of the index, the
 * taxonomy, Q, min_score and top_permille only: batch size, options, tile count, paging, a delta segment and hit
 * lists versus counter rows do not change it.
 * Outputs: four arrays of nq entries in `mem`; taxon is required, each of the other three may be NULL.
 * NIQKI_MEM_HOST works in batches of option "query_batch"; NIQKI_MEM_DEVICE takes the nq sketches in one call and
 * writes in stream order.  There is no capacity argument and NIQKI_E_CAPACITY never occurs.
 * niqki_staged_query_lca works on the staged batch (niqki_stage_raw) and leaves it usable, as
 * niqki_staged_query_collapsed does.
 * Handles as niqki_query_collapsed: whole-range single-GPU handles, resident or paged, any tile count, with or without
 * a delta segment, S <= 16; a slot-range shard gets NIQKI_E_STATE.  Groups, the _shared calls and the _ahead calls
 * have no LCA form.
 * How: per batch the query path itself runs at top_k = 0 into the handle's device hit buffers (budget: option
 * "cluster_ws_mib"; a batch whose lists do not fit is halved down to one query, first half first; stat "lca_splits"),
 * then one launch of lca_kernel per leaf.  A 256-thread workgroup takes four queries at a time, a wavefront each.  The
 * wavefront finds the considered prefix by a 64-way search of the ordered counts (64 evenly spaced probes and a ballot
 * a step, at most 6 steps), each lane folds its strided share of the prefix with a pairwise LCA -- lift the deeper
 * node to the other's depth, then both until they meet or both are roots, at most "taxonomy_depth" steps each -- and
 * six __shfl_xor steps combine the lanes.  A prefix longer than option "lca_wave_cap" (64 .. 65536, default 1024) is
 * folded by the whole workgroup after the four waves' own queries; stat "lca_long_lists" counts those queries of the
 * last call, stat "lca_no_common" its queries with considered >= 2 and no common taxon.  Nothing spins and no loop is
 * unbounded.  While profiling is on: "lca_us_hits", "lca_us_fold" (microseconds, the last call).  DESIGN.md 4.5e. */
#define NIQKI_TAXON_NONE 0xFFFFFFFFu
int niqki_set_taxonomy(niqki_index *ix, const uint32_t *genome_taxon, uint32_t n_genomes, const uint32_t *parent,
                       uint32_t n_taxa, int mem);
int niqki_query_lca(niqki_index *ix, const int32_t *sketches, uint32_t nq, uint32_t top_permille, uint32_t *taxon,
                    uint32_t *best_count, uint32_t *best_gid, uint32_t *considered, int mem);
int niqki_staged_query_lca(niqki_index *ix, uint32_t top_permille, uint32_t *taxon, uint32_t *best_count,
                           uint32_t *best_gid, uint32_t *considered, int mem);

/* Taxon tally: the rows of the LCA calls counted per taxon and per clade on the device -- what a read classifier's
 * report holds.  The LCA calls answer per query; a read set asks how many reads landed ON each taxon and how many in
 * the clade BELOW it.  The rows are on the device already and so is the taxonomy; the tally is an accumulator beside
 * them, and a caller in NIQKI_MEM_DEVICE reads back 32 bytes per taxon instead of 16 bytes per read.  It counts nothing
 * new in the index and touches no gather or hit kernel: its answer is a pure function of rows the LCA calls return.
 * State.  A handle has at most one tally; it belongs to the handle's taxonomy.  niqki_tally_begin allocates and clears
 * the accumulators for n_taxa taxa and opens the tally; on an open or broken tally it clears and reopens it; without
 * a taxonomy it returns NIQKI_E_STATE and niqki_last_error says to set one; on a slot-range shard NIQKI_E_STATE, as the
 * LCA calls.  niqki_tally_end discards the tally (NIQKI_OK also when none is open).  Whatever replaces or drops the
 * taxonomy ends the tally: a successful niqki_set_taxonomy (set or remove) and every call that drops the taxonomy
 * (inserts, a committed niqki_append_*, niqki_retain, import); a refused niqki_set_taxonomy leaves it alone.
 * niqki_tally_add and niqki_tally_read without a tally return NIQKI_E_STATE.
 * Rows.  A row is (taxon, best_count, considered) as the LCA calls write them.  taxon < n_taxa: classified,
 * direct[taxon] += 1 and direct_best[taxon] += best_count.  taxon == NIQKI_TAXON_NONE and considered == 0: no_hit.
 * taxon == NIQKI_TAXON_NONE and considered >= 1: no_common.  Anything else is a bad row: it is never used as an index,
 * the call returns NIQKI_E_INVALID, niqki_last_error gives the number of bad rows, and the tally becomes BROKEN,
 * because the good rows of that call have already been added.  niqki_tally_add: best_count == NULL counts as all
 * zeros, considered == NULL counts every NONE row as no_hit, n == 0 adds nothing; mem names the space of the three
 * arrays.  Host arrays are staged by the library and the call synchronises.  Device arrays are read in stream order and
 * the call does not synchronise, so bad rows among them are reported by the next niqki_tally_read, which returns
 * NIQKI_E_INVALID and breaks the tally then.
 * While a tally is open every niqki_query_lca and niqki_staged_query_lca on the handle adds each row it returns,
 * exactly once: in both memory spaces, for every batch and every halved leaf, and whichever of the three optional
 * output arrays the caller left NULL (the library keeps those rows in a workspace of its own).  The rows the caller gets
 * are unchanged.  A call refused before its first batch (a bad top_permille, a missing taxonomy, an argument error)
 * adds nothing and leaves the tally usable; a call that fails later marks it broken.  On a broken tally
 * niqki_tally_read and niqki_tally_add return NIQKI_E_STATE and niqki_last_error says why; niqki_tally_begin starts
 * afresh.  Plain, collapsed, cover and self-join calls are never tallied; groups, the _shared calls and the _ahead
 * calls have no tally because they have no LCA form.
 * Read.  niqki_tally_read leaves the tally open: more rows may follow, and a second read without new rows returns the
 * same bytes.  With sub(t) = t and all its descendants under parent: clade[t] = the sum of direct[u] over u in sub(t),
 * clade_best[t] = the sum of direct_best[u] over u in sub(t).  Each of the four arrays has n_taxa entries in `mem` and
 * may be NULL; totals is host memory whatever mem is and may be NULL.  The call synchronises.
 * Always: queries = classified + no_hit + no_common; the sum of direct = classified; the sum of clade over the roots =
 * classified; clade[t] >= direct[t].  All sums are exact 64-bit integers.  The result is a function of the multiset of
 * rows and the taxonomy only: call boundaries, batch size, memory space, "lca_wave_cap", splits and the order in which
 * the device adds do not change it.
 * Stats: "tally" = 0 none, 1 open, 2 broken; "tally_queries" = the rows added as of the last read (0 without a tally);
 * while profiling is on "tally_us_add" (the row kernel of the last LCA or add call) and "tally_us_clade" (the last
 * read), microseconds.
 * How: tally_rows_kernel gives a 256-thread workgroup passes of 1024 rows.  A pass is entered into an open-addressing
 * table in LDS keyed by taxon (2048 slots of {key, count, best sum}, 32 KiB; LDS atomics; probing bounded by the table
 * size, which a pass cannot fill); after a barrier every occupied slot leaves with one 64-bit global atomic per array
 * and is cleared -- a read set that sends most of a batch to one taxon costs that taxon's cache line one add per pass,
 * not one per read.  Rows without a taxon and bad rows are counted per workgroup and leave once.  At read,
 * tally_clade_kernel takes a thread per taxon with direct > 0 and walks to its root, adding at every node, at most
 * "taxonomy_depth" + 1 steps.  Device state: 32 bytes per taxon and four words.  DESIGN.md 4.5g. */
typedef struct niqki_tally_totals {
  uint64_t queries;     /* rows added */
  uint64_t classified;  /* rows with a taxon */
  uint64_t no_hit;      /* NIQKI_TAXON_NONE, considered == 0 */
  uint64_t no_common;   /* NIQKI_TAXON_NONE, considered >= 1 */
} niqki_tally_totals;
int niqki_tally_begin(niqki_index *ix);
int niqki_tally_add(niqki_index *ix, const uint32_t *taxon, const uint32_t *best_count, const uint32_t *considered,
                    uint32_t n, int mem);
int niqki_tally_read(niqki_index *ix, uint64_t *direct, uint64_t *clade, uint64_t *direct_best,
                     uint64_t *clade_best, niqki_tally_totals *totals, int mem);
int niqki_tally_end(niqki_index *ix);

/* Drops genomes from the index.  keep: niqki_genome_count(ix) bytes, nonzero = the genome stays.  new_ids (may be
 * NULL; same length, same `mem` space) receives every old genome's new id, 0xFFFFFFFF for a dropped one; *n_kept (may
 * be NULL, host memory whatever mem is) the number of genomes left.  mem as in niqki_cluster: NIQKI_MEM_DEVICE uses
 * keep / new_ids in place, in stream order.  The call synchronises once (the kept count sizes the new store).
 * Definition: after the call the handle is indistinguishable, through every call of this header, from a fresh handle
 * with the same parameters and options into which niqki_get_sketches of the kept genomes was inserted in ascending
 * old-id order.  So a kept genome's new id is the number of kept genomes below it; niqki_genome_count,
 * niqki_get_sketches, every query call, niqki_matrix_range, the self-join calls and the dump bytes are those of that
 * fresh handle; genomes inserted afterwards get ids from n_kept on; min_score, top_k and all options are untouched.
 * All kept: nothing changes (a built index stays built, new_ids is the identity).  None kept: an empty, usable index.
 * No genomes: NIQKI_OK, *n_kept = 0.  Handles as niqki_cluster: whole-range single-GPU handles, resident or paged,
 * S <= 16; NIQKI_E_STATE on a slot-range shard.  Groups cannot drop genomes (out of scope: build a single-GPU index).
 * NIQKI_E_NOMEM (the new store could not be allocated): the genome set is unchanged, the index is rebuilt on the next
 * use, the handle stays consistent.
 * A rank pass turns the flags into ids and per-block destinations, a kernel compacts the kept columns of the sketch
 * store into a new, smaller one, and the inverted index (both segments) is dropped: the next use builds one main
 * segment (stats "store_bytes" shrinks, "delta_genomes" reads 0).  A paged handle's store is host memory and is
 * compacted in place by the host.  Staged batches and batches sketched ahead are untouched.
 * While profiling is on the call times its two device phases with events: "retain_us_rank", "retain_us_compact"
 * (microseconds, the last call; tools/bench_retain.py). */
int niqki_retain(niqki_index *ix, const uint8_t *keep, uint32_t *new_ids, uint32_t *n_kept, int mem);

/* Unites the indexed genomes by label: one entry per label, its sketch the sketch of the members' pooled k-mers (a pan
 * index, one sketch per species).  labels: one uint32_t per indexed genome with the value rules of niqki_set_labels --
 * arbitrary, not necessarily dense, 0 and 0xFFFFFFFF ordinary labels; n must equal niqki_genome_count(ix), else
 * NIQKI_E_INVALID and nothing changes.  new_ids (may be NULL; length n, same `mem` space) receives the number of every
 * genome's label; *n_labels (may be NULL, host memory whatever mem is) the number of distinct labels L.  mem as in
 * niqki_retain: NIQKI_MEM_DEVICE takes labels / new_ids in stream order; the call may synchronise once.
 * Definition: let c_g[s] be what niqki_get_sketches returns for genome g and slot s before the call.  The distinct
 * labels are numbered 0 .. L - 1 by the smallest genome id that carries them.  U_l[s] is the minimum of c_g[s] over the
 * members g of label l with c_g[s] >= 0, and -1 when no member has a valid cell there.  After the call the handle is
 * indistinguishable, through every call of this header, from a fresh handle with the same parameters and options into
 * which U_0 .. U_{L-1} were inserted in that order.  A cell holds the smallest fingerprint seen in its slot, so U_l is
 * what niqki_sketch makes of the members' records when they share one entry through entry_rec (before densification
 * fills a cell that no member has).  new_ids[g] is the number of g's label; genomes inserted afterwards get ids from L
 * on; min_score, top_k and all options are untouched.
 * All labels distinct: nothing changes (a built index stays built, new_ids is the identity).  One label for all: one
 * entry.  No genomes: NIQKI_OK, *n_labels = 0.
 * A labelling (niqki_set_labels) and a taxonomy (niqki_set_taxonomy) on the handle are removed whatever the labels are,
 * as niqki_retain removes them; the labels given here are consumed, not installed.  Handles as niqki_retain:
 * whole-range single-GPU handles, resident or paged, with or without a delta segment, S <= 16; NIQKI_E_STATE on a
 * slot-range shard and while an append is pending.  Groups have no such call (out of scope: unite on a single-GPU
 * handle).  NIQKI_E_NOMEM (the new store could not be allocated): the genome set is unchanged, the handle stays
 * consistent.  Staged batches and batches sketched ahead are untouched.
 * How: the host numbers the labels and lists every label's members, one-off work as in niqki_set_labels.  One kernel
 * then writes a new store of L columns: an empty cell is the largest 16-bit value, so a label's cell is the plain
 * unsigned minimum of its members' cells.  A wavefront owns 64 consecutive new columns of 16 rows; a label of few
 * members is folded by its own lane, a larger one by the whole wavefront, and every cell is written once by a plain
 * store (no atomics).  The inverted index (both segments) is dropped: the next use builds one main segment ("store_bytes"
 * shrinks, "delta_genomes" reads 0).  A paged handle's store is host memory; the host takes the minima in place.
 * While profiling is on: "unite_us_prepare" (the host's part and its copies), "unite_us_min" (the minimum pass), in
 * microseconds for the last call (tools/bench_unite.py).  DESIGN.md 4.6h. */
int niqki_unite(niqki_index *ix, const uint32_t *labels, uint32_t n, uint32_t *new_ids, uint32_t *n_labels, int mem);

/* Register histograms: what a genome's size is estimated from.  The top H bits of a cell are a HyperLogLog register
 * (get_fingerprint, src/niqki_index.cpp:277-287: max(0, 2^H - 1 - leading zeros of the hash); a slot keeps its smallest
 * fingerprint, so the most leading zeros), and a sketch's F registers give its number of distinct k-mers with standard
 * error 1.04 / sqrt(F).  These calls count the registers; the estimate itself is host arithmetic on the counts
 * (niqki_amd/host/size_estimate.h), so every device result is an integer that can be checked bit for bit.
 * Definition: let B = NIQKI_REGISTER_BINS(H) = 2^H + 1 and M = W - H.  A cell c is valid when 0 <= c < 2^W, the rule of
 * Index::query_sketch.  hist is uint32_t [rows][B] in `mem`: hist[j * B + (c >> M)] counts the valid cells of row j with
 * that register value, hist[j * B + 2^H] its cells that are not valid; every row sums to 2^S.
 * niqki_registers: row j is genome begin + j, its cells what niqki_get_sketches(ix, begin, end - begin) returns -- a
 * function of the genome set alone, whatever the tile count, paging, a delta segment, or an earlier niqki_retain,
 * niqki_unite or append.  niqki_sketch_registers: the n x 2^S cells given (same `mem`).  niqki_staged_registers: the
 * sketches of the staged batch (niqki_stage_raw), n_entry rows; the batch stays usable, as after niqki_staged_cover.
 * Refused: begin > end or end > niqki_genome_count (NIQKI_E_INVALID); H > 6 (NIQKI_E_INVALID: select_best_H picks 2..6,
 * and 65 bins are the most a lane's table should hold); fingerprint parts that are not regular, that is H changed by
 * niqki_select_best_H after construction (NIQKI_E_STATE: the top H bits are no register then); a slot-range shard
 * (NIQKI_E_STATE).  niqki_last_error says which.  An empty range, n = 0, an empty staged batch or an index without
 * genomes: NIQKI_OK, nothing is written.  Groups, the _shared and the _ahead calls have no such call.
 * mem as in niqki_cluster: NIQKI_MEM_DEVICE writes hist in stream order and does not synchronise (unless profiling is
 * on); NIQKI_MEM_HOST goes through one device workspace and crosses once.
 * How: the store is u16 [2^S][capacity], slot-major.  A wavefront takes 64 consecutive genome columns -- one row of them
 * is one 128-byte line -- and a chunk of the rows; each lane owns one genome and keeps its B 32-bit counters in LDS, laid
 * out [bin][lane], so no two lanes share a counter or, within a step, a bank.  The rows are cut into chunks so that a
 * small index still fills the device, and a chunk's counters leave with one global atomic add per (genome, bin),
 * contiguous in hist.  The row pass gives a wavefront one sketch (or a chunk of it), 64 cells a step, the same counters,
 * and sums them over the lanes at the end.  A paged handle's store is host memory: the host counts it.
 * While profiling is on: "registers_us_store", "registers_us_rows", the last call of each kernel in microseconds
 * (tools/bench_sizes.py).  DESIGN.md 4.6j. */
#define NIQKI_REGISTER_BINS(H) ((1u << (H)) + 1u)
int niqki_registers(niqki_index *ix, uint32_t begin, uint32_t end, uint32_t *hist, int mem);
int niqki_sketch_registers(niqki_index *ix, const int32_t *sketches, uint32_t n, uint32_t *hist, int mem);
int niqki_staged_registers(niqki_index *ix, uint32_t *hist, int mem);

/* dump_index_disk payload (src/niqki_index.cpp:42-55), before gzip and
 * without the trailing names: 6 x u32 header {lF,K,H,W,min_score,N} then per
 * bucket u32 size + size x u32 gid, buckets in fp + slot*2^W order, gids
 * ascending.  Call with buf == NULL to get the size.  Host memory only;
 * whole-range handles only. */
int niqki_export_dump(niqki_index *ix, uint8_t *buf, uint64_t capacity,
                      uint64_t *size);

/* Loading constructor (src/niqki_index.cpp:63-90) from the gunzipped bytes of
 * a dump (names excluded; *consumed = offset of the first name byte).  The
 * parameters stored in the dump override those given (like :67-72), except
 * device / tile_genomes / slot range, which are taken from `params`: a handle
 * created with a slot range keeps only its own slots of the dump (one shard of
 * a multi-GPU index), the bytes of the other slots are walked and skipped.  top_k and
 * resident_mib are taken from `params` too (the dump does not hold them). */
int niqki_import_dump(const niqki_params *params, const uint8_t *buf,
                      uint64_t len, uint64_t *consumed, niqki_index **out);

/* Streaming forms of the two calls above, for dumps that should not sit in one
 * buffer (13.6 GB at 100k genomes): the 24-byte header, the byte position of
 * every slot's first bucket in the payload (2^S + 1 entries, header excluded),
 * and the payload of a range of whole slots. */
/* On a slot-range handle (one shard of a multi-GPU index) the layout and the slot numbers of
 * niqki_export_dump_slots are relative to the shard's first slot (2^S -> slot_end - slot_begin):
 * the shards' payloads in rank order are the dump of the whole index. */
int niqki_export_dump_header(niqki_index *ix, uint8_t header[24]);
int niqki_export_dump_layout(niqki_index *ix, uint64_t *slot_bytes);
int niqki_export_dump_slots(niqki_index *ix, uint32_t slot_begin, uint32_t slot_end,
                            uint8_t *buf, uint64_t capacity, uint64_t *size);
/* niqki_import_begin creates the handle from the header (slot range from `params`,
 * as above); niqki_import_slots takes the payload of whole slots [slot_begin,
 * slot_end) in order (*consumed = bytes used; slots outside the handle's range are
 * validated and dropped); after the last slot the handle is a normal index (built
 * on first use). */
int niqki_import_begin(const niqki_params *params, const uint8_t header[24], niqki_index **out);
int niqki_import_slots(niqki_index *ix, uint32_t slot_begin, uint32_t slot_end,
                       const uint8_t *buf, uint64_t len, uint64_t *consumed);

/* Appends the genomes of a dump (the bytes niqki_import_dump reads) to a handle that may already hold genomes, without
 * a genome being sketched again.  Definition: let B be the handle niqki_import_dump makes from the same bytes, N_B its
 * genome count.  A committed append leaves ix indistinguishable, through every call of this header, from ix after
 * niqki_insert(ix, niqki_get_sketches(B, 0, N_B)): the dump's genome g becomes id n_before + g; min_score, top_k and
 * all options stay the handle's (the dump's min_score word is ignored); a delta segment or a rebuild follows as after
 * an insert (option "incremental_build"); the dump bytes afterwards are those of a fresh handle into which all
 * n_before + N_B sketches were inserted in that order.
 * The header's lF, K, W and H must equal the handle's current ones (H: the value after any niqki_select_best_H), else
 * NIQKI_E_INVALID, niqki_last_error names the field, nothing changes.
 * niqki_append_begin grows the sketch store (resident, or the paged host store) to n_before + N_B columns and presets
 * the new ones to empty.  niqki_append_slots takes the payload of whole slots [slot_begin, slot_end) (*consumed = the
 * bytes used): ascending, contiguous from slot 0, in any grouping.  The append COMMITS when slot 2^S - 1 has been
 * taken: the genome count grows by N_B and the inserts are pending for the next build.  Until then the index is the
 * old one for every reader (queries, niqki_genome_count, dumps), and the calls that add or drop genomes -- niqki_insert,
 * niqki_insert_shared, niqki_staged_insert, niqki_retain, a second niqki_append_begin -- return NIQKI_E_STATE.  A
 * failing niqki_append_slots (a payload that ends inside a slot, a genome id >= N_B, slots out of order:
 * NIQKI_E_INVALID) cancels the append itself; niqki_append_cancel (NIQKI_OK also when none is pending) and a failure
 * both leave the index exactly as before: same count, same dump bytes, still built if it was built.
 * N_B = 0 commits at once (no niqki_append_slots call follows).  An append into an empty handle equals an import.
 * niqki_append_dump is the one-shot form: header and payload in one buffer (*consumed = offset of the first name byte).
 * Handles as niqki_retain: whole-range single-GPU handles, resident or paged, S <= 16; NIQKI_E_STATE on a slot-range
 * shard.  Groups cannot append (out of scope: append on a single-GPU handle, or pair niqki_get_sketches with
 * niqki_insert in device memory).  DESIGN.md 4.6e. */
int niqki_append_begin(niqki_index *ix, const uint8_t header[24]);
int niqki_append_slots(niqki_index *ix, uint32_t slot_begin, uint32_t slot_end,
                       const uint8_t *buf, uint64_t len, uint64_t *consumed);
int niqki_append_cancel(niqki_index *ix);
int niqki_append_dump(niqki_index *ix, const uint8_t *buf, uint64_t len, uint64_t *consumed);

/* Reads back the stored sketches of genomes [begin, begin+n) as n x F int32
 * (slots outside the shard's range read -1). */
int niqki_get_sketches(niqki_index *ix, uint32_t begin, uint32_t n,
                       int32_t *sketches, int mem);

/* ---- one index over several GPUs: slot-range shards -----------------------------
 * No reference counterpart (the reference is one process on one host); this is how
 * Index::insert_sketch / Index::query_sketch (src/niqki_index.cpp:362-370, :633-687)
 * run when the F x 2^W inverted index is split by sketch-slot range over the GPUs
 * of a node.  Rank r of `world` owns slots niqki_group_slot_range(r) of EVERY
 * genome: a handle created with that slot range is one shard.  The hit count of a
 * genome is a sum over slots, so a batch needs one exchange of partial results,
 * done with RCCL over xGMI inside the library (librccl is loaded when the first
 * group is made).  Results are exactly those of one whole-range handle.
 * NIQKI_GROUP_TRANSPORT=ipc (environment, read by niqki_group_create and
 * niqki_group_new_id; one rank per process) replaces RCCL by direct peer access: every
 * rank maps its peers' exchange buffers through HIP IPC handles and pulls its part with
 * copy / summing kernels, ordered by sequence words in device memory -- a direct
 * all-to-all over all xGMI links, no host synchronisation inside a step, and ranks may
 * share a device (which RCCL refuses).
 *
 * A niqki_group is the set of ranks that live in the calling process:
 *   - one rank per process (n_local = 1, first_rank = this process' rank; `id` made
 *     once by niqki_group_new_id and carried to every process by the caller), or
 *   - all ranks in one process (n_local = world, first_rank = 0, id may be NULL).
 *     Shards of such a group may even share a device (tests; emulating G shards on
 *     one GPU): device-to-device copies then stand in for the collectives.
 * The per-rank arrays of the calls below have n_local entries, rank first_rank + i at
 * index i; sketch buffers are device memory of that rank's GPU, work is enqueued on
 * the shard handles' streams.  Calls are collective: every process of the group makes
 * the same calls in the same order. */
typedef struct niqki_group niqki_group; /* opaque */
#define NIQKI_GROUP_ID_BYTES 128

void niqki_group_slot_range(uint32_t rank, uint32_t world, uint32_t S, uint32_t *slot_begin,
                            uint32_t *slot_end);
int niqki_group_new_id(uint8_t id[NIQKI_GROUP_ID_BYTES]);
/* The shards must agree in K, S, W, min_score, top_k and genome count and own the slot ranges
 * of their ranks (S = 16: at least two shards).  On failure niqki_last_error(shards[0]) says why. */
int niqki_group_create(niqki_index *const *shards, uint32_t n_local, uint32_t first_rank,
                       uint32_t world, const uint8_t *id, niqki_group **out);
void niqki_group_destroy(niqki_group *g); /* the shard handles stay the caller's */
const char *niqki_group_last_error(const niqki_group *g);
/* "exchange": 0 = choose (sparse when min_score >= 4 * world; never with top_k > 0, whose batches always take the
 * dense exchange, stat "sparse" then reads 0), 1 = sparse (candidate
 * genomes only), 2 = dense (reduce-scatter of whole hit vectors); "cand_cap": candidate
 * ids per query and rank of the sparse form, even, default 256 (a step whose lists
 * overflow is redone densely, never answered wrongly); "surv_cap": survivors (genomes with a
 * partial count of at least half the candidate threshold) a shard keeps per query, default 1024,
 * at most 4096. */
int niqki_group_set_option(niqki_group *g, const char *key, int64_t value);
/* "overflows" (sparse steps redone densely so far), "rccl" (1 = RCCL transport),
 * "transport" (0 = device copies inside one process, 1 = RCCL, 2 = ipc),
 * "sparse" (1 = the sparse exchange is selected), "ipc_words_kind" (ipc transport: where this rank's
 * sequence words live -- 1 = fine-grained device memory mapped by the peers, 2 = the processes' shared block
 * page-locked and mapped into every device, 0 = plain device memory), "ipc_arena_fine" (1 = its exchange
 * buffers are fine-grained device memory), "ranks_seen" (how many ranks the transport itself knows of: the
 * communicator's size as RCCL reports it, the peers whose sequence words this process has mapped (ipc), the shards of
 * the process (local) -- equal to `world` when the group really spans what the caller thinks it spans). */
int niqki_group_get_stat(const niqki_group *g, const char *key, uint64_t *value);
/* Index::insert_sketch for a batch of world * per sketches of which rank r holds rows
 * [r*per, (r+1)*per) (local_sketches[i]: per x 2^S int32, device memory); the first
 * n_total rows of the batch (rank major) get the next genome ids, the rest is padding. */
int niqki_group_insert(niqki_group *g, const int32_t *const *local_sketches, uint32_t per,
                       uint32_t n_total);
/* Index::query_sketch for such a batch: rank r receives the hits of ITS rows against the
 * whole index -- hit_off[i] per+1 offsets, hit_counts[i] / hit_gids[i] capacity entries
 * each, in the memory space `mem` (as niqki_query).  NIQKI_MEM_DEVICE: a rank whose lists hold
 * more than `capacity` hits gets exact offsets and the first `capacity` entries of its lists in
 * their order; nothing is written behind them. */
int niqki_group_query(niqki_group *g, const int32_t *const *local_sketches, uint32_t per,
                      uint64_t *const *hit_off, uint32_t *const *hit_counts,
                      uint32_t *const *hit_gids, uint64_t capacity, int mem);
/* The same in two halves.  _begin enqueues the whole batch on the shards' streams (slice
 * exchange, gather, sparse or dense sum, threshold + order into the caller's device buffers)
 * and returns without waiting for the device: the caller can enqueue other work -- the sketch
 * kernel of the next batch on another handle's stream -- that then runs beside the exchange.
 * _end is the one place the host waits: it checks the batch's candidate-overflow word (a
 * sparse batch whose lists overflowed is redone densely here), copies host results out
 * (NIQKI_MEM_HOST) and reports a peer that never answered (ipc transport).  One batch in
 * flight per group; the argument arrays of _begin may go away after it returns, the buffers
 * they point to must stay until _end.  A _begin that fails leaves no batch in flight (an _end
 * after it returns NIQKI_E_STATE).  niqki_group_query = _begin + _end. */
int niqki_group_query_begin(niqki_group *g, const int32_t *const *local_sketches, uint32_t per,
                            uint64_t *const *hit_off, uint32_t *const *hit_counts,
                            uint32_t *const *hit_gids, uint64_t capacity, int mem);
int niqki_group_query_end(niqki_group *g);

/* The two calls above on the shards' STAGED batches (niqki_stage_raw on each shard handle --
 * how the `niqki` host program feeds a multi-GPU index from files; all ranks in one process):
 * rank r contributes the first n_entry[r] sketches of its staged batch (0: none) as rows
 * [r*per, r*per + n_entry[r]) of the batch, the rest of its rows is padding.  An insert gives
 * the entries their ids rank after rank (rank 0's entries first), like the id counter of
 * src/niqki_index.cpp:396-401 does in file order. */
int niqki_group_staged_insert(niqki_group *g, uint32_t per, const uint32_t *n_entry);
int niqki_group_staged_query(niqki_group *g, uint32_t per, const uint32_t *n_entry, uint64_t *const *hit_off,
                             uint32_t *const *hit_counts, uint32_t *const *hit_gids, uint64_t capacity,
                             int mem);

/* Sizes of the handle's state: "store_bytes" (sketch store), "index_bytes" (table + id lists of
 * the built index or resident page), "tiles", "pages" / "page_slots" (pages a query walks and
 * slots per page; 1 / all slots unless the index is paged), "delta_genomes" (genomes indexed by
 * the delta segment, see option "incremental_build"), "last_gather_form" (launch form the last
 * counter call used: bit 0 look-up pre-pass, bit 1 the packed copy of the table was prepared
 * for it -- its launches of at least 512 queries take the streamed-rows kernel, smaller ones
 * the random look-ups --, bit 2 locality order), "last_gather_kernel" (the gather kernel instantiation the last counter call launched:
 * BLOCK | UNROLL << 12 | (NT + 1) << 20 | PAD << 24 -- threads per workgroup, bucket lines per round trip,
 * NT = -1 look-ups from the pre-pass, 2..4 the stash form of that many tiles, 1 one look-up per tile; PAD = 1
 * the padded walk was launched, which takes "bucket_align_log2" 6 and a 1024-thread shape; option
 * "gather_variant" 1..5 = BLOCK, UNROLL 1024, 8 / 1024, 32 / 512, 16 / 256, 16 / 128, 16),
 * "last_densify_form" (the densification the last niqki_sketch / niqki_densify / staged sketch call chose: 0 = none
 * yet or an empty batch, 1 = the one-wavefront short-record kernel, 2 = plain passes inside the sketch kernel,
 * 3 = passes over distinct values inside the sketch kernel, 4 = distinct-value passes as a launch of its own,
 * 5 = the global-memory launch of sketches whose cells do not fit LDS; where a batch takes several launches, the first one's),
 * "bucket_align_log2" (the built index's bucket alignment, as set by the option or chosen from the tile size),
 * "last_hits_form" (1 =the last niqki_query* call took the hit-list form, option "hit_lists"), "class_mask" (1 = the built index carries its per-slot class mask: single-tile
 * indexes; the gather kernel then looks up only fingerprints whose sixteenth of the
 * fingerprint range holds a bucket in their slot -- a short read against a genome index
 * skips nearly all of its 2^S table look-ups; results are unaffected; NIQKI_HMASK=0 in the
 * environment builds indexes without it). */
int niqki_get_stat(const niqki_index *ix, const char *key, uint64_t *value);

#ifdef __cplusplus
}
#endif
#endif /* NIQKI_HIP_H */
