// nq_api_retain.hip -- niqki_retain behind the C ABI: drop genomes from a handle.  The sketch store's kept columns are
// compacted on the device into a new, smaller store (nq_index.hip: the rank pass and store_compact_kernel; block
// arithmetic in nq_retain_blocks.h) and both index segments are released (release_segments), so the next use builds ONE
// main segment from what is left.  A paged handle's store is page-locked host memory: the host compacts its rows in
// place.  How the handle takes the new store is shared with niqki_unite (nq_api_build.hip: adopt_store,
// host_store_rewritten).  DESIGN.md 4.6d.
#include "nq_handle.h"

#include <string>
#include <vector>

namespace nqi {

namespace {

// paged handle: every row of the host store, forward and in place (a kept column's destination is at or below it)
void compact_host_store(niqki_index *ix, const std::vector<uint64_t> &words, uint32_t n, uint32_t n_kept) {
  std::vector<uint32_t> col;
  col.reserve(n_kept);
  for (uint32_t c = 0; c < n; ++c)
    if ((words[c >> 6] >> (c & 63u)) & 1u) col.push_back(c);
  const uint32_t f_all = ix->full_end - ix->full_begin;
  for (uint32_t s = 0; s < f_all; ++s) {
    uint16_t *row = ix->host_store + (size_t)s * ix->host_cap;
    for (uint32_t j = 0; j < n_kept; ++j) row[j] = row[col[j]];
  }
}

// while profiling is on: events around the rank pass and the compaction (niqki_get_stat "retain_us_*")
struct PhaseEvents {
  niqki_index *ix;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  explicit PhaseEvents(niqki_index *ix_) : ix(ix_) {
    ix->retain_ms[0] = ix->retain_ms[1] = 0;
    if (ix->prof)
      for (auto &e : ev)
        if (hipEventCreate(&e) != hipSuccess) e = nullptr;
  }
  ~PhaseEvents() {
    for (auto &e : ev) if (e) (void)hipEventDestroy(e);
  }
  void mark(int k) { if (ev[k]) (void)hipEventRecord(ev[k], ix->stream); }
  void read(int phase) {   // after a synchronisation behind mark(2 * phase + 1)
    float ms = 0;
    if (ev[2 * phase] && ev[2 * phase + 1] && hipEventElapsedTime(&ms, ev[2 * phase], ev[2 * phase + 1]) == hipSuccess) ix->retain_ms[phase] = ms;
  }
};

int retain_run(niqki_index *ix, const uint8_t *keep, uint32_t *new_ids, uint32_t *n_kept, int mem) {
  const uint32_t N = ix->n_genomes;
  PhaseEvents phases(ix);
  const bool dev = mem == NIQKI_MEM_DEVICE;
  const uint32_t n_blocks = (uint32_t)(((uint64_t)N + nq::kRetainBlock - 1) / nq::kRetainBlock);
  // keep words, blk_dst[n_blocks + 1] (padded to 8 bytes), then the device copies of a host call's arrays
  const size_t words_bytes = (size_t)n_blocks * nq::kRetainWords * 8, blk_bytes = ((size_t)n_blocks + 2) / 2 * 8;
  int rc = ensure(ix, ix->ws_parent, words_bytes + blk_bytes + (dev ? 0 : (size_t)N * 5));
  if (rc) return rc;
  unsigned long long *words = (unsigned long long *)ix->ws_parent.p;
  uint32_t *blk_dst = (uint32_t *)((uint8_t *)ix->ws_parent.p + words_bytes);
  uint32_t *own_ids = (uint32_t *)((uint8_t *)blk_dst + blk_bytes);
  uint8_t *own_keep = (uint8_t *)(own_ids + N);
  const uint8_t *d_keep = keep;
  uint32_t *d_ids = !new_ids ? nullptr : dev ? new_ids : own_ids;
  if (!dev) {
    NQ_HIP(ix, hipMemcpyAsync(own_keep, keep, N, hipMemcpyHostToDevice, ix->stream));
    d_keep = own_keep;
  }
  phases.mark(0);
  {
    Span sp(ix, NIQKI_KC_BUILD);
    NQ_HIP(ix, nq::launch_retain_ranks(d_keep, N, words, blk_dst, d_ids, ix->stream));
  }
  phases.mark(1);
  uint32_t total = 0;
  std::vector<uint64_t> h_words;
  if (ix->resident_bytes) {
    h_words.resize((size_t)n_blocks * nq::kRetainWords);
    NQ_HIP(ix, hipMemcpyAsync(h_words.data(), words, words_bytes, hipMemcpyDeviceToHost, ix->stream));
  }
  if (!dev && new_ids) NQ_HIP(ix, hipMemcpyAsync(new_ids, d_ids, (size_t)N * 4, hipMemcpyDeviceToHost, ix->stream));
  NQ_HIP(ix, hipMemcpyAsync(&total, blk_dst + n_blocks, 4, hipMemcpyDeviceToHost, ix->stream));
  NQ_HIP(ix, hipStreamSynchronize(ix->stream));   // the one synchronisation: the kept count sizes the new store
  phases.read(0);
  if (n_kept) *n_kept = total;
  drop_labels(ix);   // (niqki_set_labels: also when all are kept, so that the call's effect does not depend on the flags)
  drop_taxonomy(ix);   // (niqki_set_taxonomy: the same)
  drop_sizes(ix);      // (niqki_set_sizes: the same)
  if (total == N) return NIQKI_OK;   // all kept: the handle, a built index included, stays as it is

  release_segments(ix);
  if (ix->resident_bytes) {
    compact_host_store(ix, h_words, N, total);
    host_store_rewritten(ix, total);
    return NIQKI_OK;
  }
  const uint32_t f_local = ix->d.slot_end - ix->d.slot_begin;
  const uint64_t cap = nq::retain_cap(total);
  uint16_t *ns = nullptr;
  // (on failure the genome set is unchanged; the index is rebuilt on the next use)
  if (hipMalloc((void **)&ns, (size_t)f_local * cap * 2) != hipSuccess) return fail(ix, NIQKI_E_NOMEM, "niqki_retain: sketch store allocation failed");
  hipError_t e;
  phases.mark(2);
  {
    Span sp(ix, NIQKI_KC_BUILD);
    e = nq::launch_store_compact(ix->store, ix->cap, N, ns, cap, f_local, words, blk_dst, ix->stream);
  }
  phases.mark(3);
  if (e == hipSuccess) e = hipStreamSynchronize(ix->stream);
  phases.read(1);
  if (e != hipSuccess) {
    (void)hipFree(ns);
    return fail(ix, NIQKI_E_HIP, std::string("niqki_retain: store compaction: ") + hipGetErrorString(e));
  }
  return adopt_store(ix, ns, cap, total);
}

}  // namespace

}  // namespace nqi

using namespace nqi;

extern "C" {

int niqki_retain(niqki_index *ix, const uint8_t *keep, uint32_t *new_ids, uint32_t *n_kept, int mem) {
  if (!ix || (!keep && ix->n_genomes)) return NIQKI_E_INVALID;
  if (!whole_range(ix)) return fail(ix, NIQKI_E_STATE, "niqki_retain: a slot-range shard holds part of every sketch; drop genomes on a whole-range handle");
  if (ix->append.active) return fail(ix, NIQKI_E_STATE, "niqki_retain: an append is pending: finish it or call niqki_append_cancel first");
  NQ_HIP(ix, hipSetDevice(ix->device));
  if (ix->n_genomes == 0) {
    if (n_kept) *n_kept = 0;
    return NIQKI_OK;
  }
  return retain_run(ix, keep, new_ids, n_kept, mem);
}

}  // extern "C"
