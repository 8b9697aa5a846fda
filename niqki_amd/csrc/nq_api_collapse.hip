// nq_api_collapse.hip -- niqki_set_labels, niqki_query_collapsed and niqki_staged_query_collapsed behind the C ABI: per
// query the best hit of every label (niqki_hip.h).  A batch's full lists are the query path's own (query_hits_dev at
// top_k = 0 into the handle's hit buffers, within the budget of the self-join calls), so every count, the threshold, the
// order and the ties are the pinned path's; the kernels of nq_collapse.hip only select from them.  The full lists never
// leave the device.  DESIGN.md 4.5d.
#include "nq_handle.h"

#include <algorithm>
#include <string>
#include <vector>

namespace nqi {

void drop_labels(niqki_index *ix) {
  ix->labels_set = false;
  ix->n_labels = 0;
}

namespace {

struct Collapse {
  niqki_index *ix;
  PhaseTimer ev;            // events of a leaf: 0-1 hits, 1-2 first, 2-3 scan + emit
  uint32_t k = 0;           // the handle's top_k: the cut of every list
  uint32_t n_tables = 0;    // global tables in ws_cl_tab (0: no list can be long)
  uint64_t staged = 0;      // entries of the current batch in ws_cl_stage
  explicit Collapse(niqki_index *ix_) : ix(ix_), ev(ix_, 4, ix_->collapse_stats.ms) {}
};

// The consumer of a leaf (HitLists): the full lists `out` of queries [q_at, q_at + n) of the batch; the first-of-label
// flags, the kept counts into ws_cl_nk[q_at ...), the kept entries behind the batch's earlier ones in ws_cl_stage.  A
// halved leaf finishes its first half before its second, so the stage fills in query order.
int collapse_consume(Collapse &c, const HitOut &out, uint32_t q_at, uint32_t n) {
  niqki_index *ix = c.ix;
  int rc;
  if ((rc = c.ev.mark(1))) return rc;
  // off[n + 1] of the leaf's kept entries, then the info words: one copy brings the total and the words back
  const size_t off_bytes = ((size_t)n + 1) * 8;
  if ((rc = ensure(ix, ix->ws_cl_off, off_bytes + nq::kCollapseInfoWords * 4))) return rc;
  if ((rc = ensure(ix, ix->ws_cl_keep, (size_t)std::max<uint64_t>(out.total, 1) * 4))) return rc;
  unsigned long long *d_off = (unsigned long long *)ix->ws_cl_off.p;
  uint32_t *info = (uint32_t *)((char *)ix->ws_cl_off.p + off_bytes);
  uint32_t *nk = (uint32_t *)ix->ws_cl_nk.p + q_at;
  NQ_HIP(ix, hipMemsetAsync(info, 0, nq::kCollapseInfoWords * 4, ix->stream));
  nq::CollapseArgs a{};
  a.hit_off = out.off;
  a.hit_gids = out.gids;
  a.dense = (const uint32_t *)ix->lab_dense.p;
  a.n_genomes = ix->n_genomes;
  a.n_labels = ix->n_labels;
  a.nq = n;
  a.lds_cap = ix->collapse_lds_cap;
  a.lds_slots = nq::collapse_lds_slots(a.lds_cap);
  a.top_k = c.k;
  a.tables = c.n_tables ? (unsigned long long *)ix->ws_cl_tab.p : nullptr;
  a.kept = (uint32_t *)ix->ws_cl_keep.p;
  a.n_kept = nk;
  a.info = info;
  NQ_HIP(ix, nq::launch_collapse_first(a, std::min<uint32_t>(n, c.n_tables ? c.n_tables : 4096u), ix->stream));
  if ((rc = c.ev.mark(2))) return rc;
  NQ_HIP(ix, nq::launch_collapse_scan(nk, n, d_off, ix->stream));
  struct {
    unsigned long long total;
    uint32_t info[nq::kCollapseInfoWords];
  } h = {0, {0, 0}};
  NQ_HIP(ix, hipMemcpyAsync(&h, d_off + n, 8 + nq::kCollapseInfoWords * 4, hipMemcpyDeviceToHost, ix->stream));
  NQ_HIP(ix, hipStreamSynchronize(ix->stream));   // the leaf's one synchronisation of its own: the total sizes the stage
  if (h.info[nq::kCollapseInfoBad] || h.total > out.total)
    return fail(ix, NIQKI_E_STATE, "niqki_query_collapsed: a hit no label table could take (a bug)");
  ix->collapse_stats.long_lists += h.info[nq::kCollapseInfoLong];
  const size_t entry = sizeof(nq::CollapsedHit);
  if ((rc = ensure_keep(ix, ix->ws_cl_stage, (size_t)c.staged * entry, (size_t)std::max<uint64_t>(c.staged + h.total, 1) * entry))) return rc;
  NQ_HIP(ix, nq::launch_collapse_emit(out.off, out.counts, out.gids, a.kept, nk, d_off, n, (nq::CollapsedHit *)ix->ws_cl_stage.p + c.staged,
                                      ix->stream));
  if ((rc = c.ev.mark(3))) return rc;
  if ((rc = c.ev.add(0, 1, 0)) || (rc = c.ev.add(1, 2, 1)) || (rc = c.ev.add(2, 3, 2))) return rc;
  c.staged += h.total;
  return NIQKI_OK;
}

// the global tables of the long route: as many as a quarter of the hit buffers' budget holds, one at least, and no more
// than a launch has workgroups; cleared once, and left cleared by every launch
int collapse_tables(Collapse &c, uint32_t batch) {
  niqki_index *ix = c.ix;
  c.n_tables = 0;
  if (ix->n_genomes <= ix->collapse_lds_cap) return NIQKI_OK;   // no list is longer than the genome count
  const uint64_t table_bytes = (uint64_t)ix->n_labels * 8;
  const uint64_t budget = ((uint64_t)std::max<uint32_t>(ix->cluster_ws_mib, 1) << 20) / 4;
  c.n_tables = (uint32_t)std::min<uint64_t>({std::max<uint64_t>(budget / table_bytes, 1), (uint64_t)batch, (uint64_t)1024});
  const size_t need = (size_t)(c.n_tables * table_bytes);
  const size_t was = ix->ws_cl_tab.n;
  int rc = ensure(ix, ix->ws_cl_tab, need);
  if (rc) return rc;
  if (ix->ws_cl_tab.n != was) ix->cl_tab_clean = false;   // (a new allocation)
  if (!ix->cl_tab_clean) NQ_HIP(ix, nq::launch_collapse_table_init((unsigned long long *)ix->ws_cl_tab.p, ix->ws_cl_tab.n / 8, ix->stream));
  ix->cl_tab_clean = false;   // (until the call has ended well)
  return NIQKI_OK;
}

int collapse_run(niqki_index *ix, const char *who, const SketchSource &src, uint32_t nq, uint64_t *hit_off, uint32_t *hit_counts,
                 uint32_t *hit_gids, uint32_t *hit_members, uint64_t capacity, int mem) {
  ix->collapse_stats = CollapseStats();
  if (!whole_range(ix)) return fail(ix, NIQKI_E_STATE, std::string(who) + ": a slot-range shard sees partial counts; the collapsed query needs a whole-range handle");
  const bool dev = mem == NIQKI_MEM_DEVICE;
  const uint32_t N = ix->n_genomes;
  if (N && !ix->labels_set)
    return fail(ix, NIQKI_E_STATE, std::string(who) + ": no labels on this genome set: call niqki_set_labels (again, after genomes were added or dropped)");
  if (nq == 0 || N == 0) {
    if (dev) NQ_HIP(ix, hipMemsetAsync(hit_off, 0, (size_t)(nq + 1) * 8, ix->stream));
    else std::fill(hit_off, hit_off + nq + 1, (uint64_t)0);
    return NIQKI_OK;
  }
  CallParams guard(ix, ix->d.min_score, 0);   // the query path at the handle's threshold and no top-k
  int rc = build_if_needed(ix);
  if (rc) return rc;
  Collapse c(ix);
  c.k = guard.k;
  if ((rc = c.ev.create())) return rc;
  const uint32_t qb = dev ? nq : std::max<uint32_t>(ix->query_batch, 1);
  if ((rc = collapse_tables(c, std::min(qb, nq)))) return rc;
  if ((rc = ensure(ix, ix->ws_cl_nk, (size_t)std::min(qb, nq) * 4))) return rc;
  std::vector<nq::CollapsedHit> h_hits;
  std::vector<uint32_t> h_nk;
  if (!dev) h_nk.resize(nq);
  uint64_t base = 0;
  HitLists hl{ix, "niqki_query_collapsed", c.ev, 0, ix->collapse_stats.splits, false};
  hl.consume = [&](const HitOut &out, const int32_t *, uint32_t q_at, uint32_t n) { return collapse_consume(c, out, q_at, n); };
  hl.after = [&](uint32_t q0, uint32_t n) {
    const nq::CollapsedHit *stage = (const nq::CollapsedHit *)ix->ws_cl_stage.p;
    if (dev) {   // one batch: the offsets in any case, the entries where the caller's arrays hold them
      NQ_HIP(ix, nq::launch_collapse_scan((const uint32_t *)ix->ws_cl_nk.p, n, (unsigned long long *)hit_off, ix->stream));
      if (c.n_tables) ix->cl_tab_clean = true;   // (every launch left them cleared)
      if (c.staged > capacity) return (int)NIQKI_E_CAPACITY;
      NQ_HIP(ix, nq::launch_collapse_unpack(stage, c.staged, hit_counts, hit_gids, hit_members, ix->stream));
      return (int)NIQKI_OK;
    }
    // host arrays: nothing reaches the caller's arrays before the total is known
    h_hits.resize(base + c.staged);
    NQ_HIP(ix, hipMemcpyAsync(h_nk.data() + q0, ix->ws_cl_nk.p, (size_t)n * 4, hipMemcpyDeviceToHost, ix->stream));
    if (c.staged)
      NQ_HIP(ix, hipMemcpyAsync(h_hits.data() + base, stage, (size_t)c.staged * sizeof(nq::CollapsedHit), hipMemcpyDeviceToHost, ix->stream));
    NQ_HIP(ix, hipStreamSynchronize(ix->stream));
    base += c.staged;
    c.staged = 0;   // (the next batch fills the stage from its start)
    return (int)NIQKI_OK;
  };
  if ((rc = hl.run(src, nq, qb)) || dev) return rc;
  if (c.n_tables) ix->cl_tab_clean = true;   // (every launch left them cleared)
  hit_off[0] = 0;
  for (uint32_t q = 0; q < nq; ++q) hit_off[q + 1] = hit_off[q] + h_nk[q];
  if (hit_off[nq] != base) return fail(ix, NIQKI_E_STATE, std::string(who) + ": the kept counts and the entries disagree (a bug)");
  if (base > capacity) return NIQKI_E_CAPACITY;
  for (uint64_t j = 0; j < base; ++j) {
    hit_counts[j] = h_hits[j].count;
    hit_gids[j] = h_hits[j].gid;
    if (hit_members) hit_members[j] = h_hits[j].members;
  }
  return NIQKI_OK;
}


}  // namespace

}  // namespace nqi

using namespace nqi;

extern "C" {

int niqki_set_labels(niqki_index *ix, const uint32_t *labels, uint32_t n, int mem) {
  if (!ix) return NIQKI_E_INVALID;
  if (!labels || n == 0) {
    drop_labels(ix);
    return NIQKI_OK;
  }
  if (n != ix->n_genomes) return fail(ix, NIQKI_E_INVALID, "niqki_set_labels: " + std::to_string(n) + " labels for " + std::to_string(ix->n_genomes) + " genomes");
  NQ_HIP(ix, hipSetDevice(ix->device));
  std::vector<uint32_t> h(n);
  if (mem == NIQKI_MEM_DEVICE) {
    NQ_HIP(ix, hipMemcpyAsync(h.data(), labels, (size_t)n * 4, hipMemcpyDeviceToHost, ix->stream));
    NQ_HIP(ix, hipStreamSynchronize(ix->stream));
  } else {
    std::copy(labels, labels + n, h.begin());
  }
  // dense ids: a label's rank among the distinct values (one-off work on the host)
  std::vector<uint32_t> uniq(h);
  std::sort(uniq.begin(), uniq.end());
  uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
  for (auto &v : h) v = (uint32_t)(std::lower_bound(uniq.begin(), uniq.end(), v) - uniq.begin());
  drop_labels(ix);
  int rc = ensure(ix, ix->lab_dense, (size_t)n * 4);
  if (rc) return rc;
  NQ_HIP(ix, hipMemcpyAsync(ix->lab_dense.p, h.data(), (size_t)n * 4, hipMemcpyHostToDevice, ix->stream));
  NQ_HIP(ix, hipStreamSynchronize(ix->stream));   // (h leaves scope)
  ix->n_labels = (uint32_t)uniq.size();
  ix->labels_set = true;
  return NIQKI_OK;
}

int niqki_query_collapsed(niqki_index *ix, const int32_t *sketches, uint32_t nq, uint64_t *hit_off, uint32_t *hit_counts, uint32_t *hit_gids,
                          uint32_t *hit_members, uint64_t capacity, int mem) {
  if (!ix || !hit_off || (!sketches && nq) || (capacity && (!hit_counts || !hit_gids))) return NIQKI_E_INVALID;
  NQ_HIP(ix, hipSetDevice(ix->device));
  return collapse_run(ix, "niqki_query_collapsed", mem == NIQKI_MEM_DEVICE ? device_rows(ix, sketches) : host_rows(ix, sketches), nq, hit_off,
                      hit_counts, hit_gids, hit_members, capacity, mem);
}

int niqki_staged_query_collapsed(niqki_index *ix, uint64_t *hit_off, uint32_t *hit_counts, uint32_t *hit_gids, uint32_t *hit_members,
                                 uint64_t capacity, int mem) {
  if (!ix || !hit_off || (capacity && (!hit_counts || !hit_gids))) return NIQKI_E_INVALID;
  NQ_HIP(ix, hipSetDevice(ix->device));
  int rc = staged_sketch_ws(ix);
  if (rc) return rc;
  // (the staged sketches are only read, so niqki_staged_query answers as before)
  return collapse_run(ix, "niqki_staged_query_collapsed", device_rows(ix, (const int32_t *)ix->ws_stsk.p), ix->staged.n_entry, hit_off,
                      hit_counts, hit_gids, hit_members, capacity, mem);
}

}  // extern "C"
