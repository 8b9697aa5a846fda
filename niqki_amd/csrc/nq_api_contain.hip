// nq_api_contain.hip -- niqki_set_sizes, niqki_query_contained and niqki_staged_query_contained behind the C ABI: per
// query the hits whose containment reaches a threshold, ordered by it and cut to top_k (niqki_hip.h).  A batch's full
// lists are the query path's own (query_hits_dev at top_k = 0 into the handle's hit buffers, within the budget of the
// self-join calls), so every count, the floor, H's order and its ties are the pinned path's; the kernels of
// nq_contain.hip compute the shares, select and order.  The full lists never leave the device.  DESIGN.md 4.5h.
#include "nq_contain_share.h"
#include "nq_handle.h"

#include <algorithm>
#include <string>
#include <vector>

namespace nqi {

void drop_sizes(niqki_index *ix) { ix->sizes_set = false; }

namespace {

struct Contain {
  niqki_index *ix;
  PhaseTimer ev;            // events of a leaf: 0-1 hits, 1-2 share, 2-3 order + scan + emit
  uint32_t k = 0;           // the handle's top_k: the cut of every list
  uint32_t mode = 0, min_share = 0;
  uint32_t qb = 0;          // queries of a batch at most: ws_ct_n holds 3 x qb words (kept, unsized, a leaf's survivors)
  const unsigned long long *d_qs = nullptr;   // the running batch's query sizes (device)
  uint64_t staged = 0;      // entries of the current batch in ws_ct_stage
  explicit Contain(niqki_index *ix_) : ix(ix_), ev(ix_, 4, ix_->contain_stats.ms) {}
};

// The consumer of a leaf (HitLists): the full lists `out` of queries [q_at, q_at + n) of the batch; the shares and the
// survivors in ws_tc / ws_tg (the hit step's scratch, free once the lists stand), their order, the kept counts into
// ws_ct_n[q_at ...), the kept entries behind the batch's earlier ones in ws_ct_stage.  A halved leaf finishes its first
// half before its second, so the stage fills in query order.
int contain_consume(Contain &c, const char *who, const HitOut &out, uint32_t q_at, uint32_t n) {
  niqki_index *ix = c.ix;
  int rc;
  if ((rc = c.ev.mark(1))) return rc;
  const size_t off_bytes = ((size_t)n + 1) * 8;
  const size_t places = (size_t)std::max<uint64_t>(out.total, 1);
  if ((rc = ensure(ix, ix->ws_ct_off, off_bytes + nq::kContainInfoWords * 4))) return rc;
  if ((rc = ensure(ix, ix->ws_tc, places * 4)) || (rc = ensure(ix, ix->ws_tg, places * 4)) || (rc = ensure(ix, ix->ws_ct_tmp, places * 8))) return rc;
  unsigned long long *d_off = (unsigned long long *)ix->ws_ct_off.p;
  uint32_t *info = (uint32_t *)((char *)ix->ws_ct_off.p + off_bytes);
  uint32_t *per_q = (uint32_t *)ix->ws_ct_n.p;
  NQ_HIP(ix, hipMemsetAsync(info, 0, nq::kContainInfoWords * 4, ix->stream));
  nq::ContainArgs a{};
  a.hit_off = out.off;
  a.hit_counts = out.counts;
  a.hit_gids = out.gids;
  a.sizes = (const unsigned long long *)ix->sizes_dev.p;
  a.qsizes = c.d_qs + q_at;
  a.n_genomes = ix->n_genomes;
  a.nq = n;
  a.F = ix->d.F;
  a.mode = c.mode;
  a.min_share = c.min_share;
  a.top_k = c.k;
  a.a_share = (uint32_t *)ix->ws_tc.p;
  a.a_npos = (uint32_t *)ix->ws_tg.p;
  a.b_share = (uint32_t *)ix->ws_ct_tmp.p;
  a.b_npos = a.b_share + places;
  a.n_kept = per_q + q_at;
  a.n_unsized = per_q + c.qb + q_at;
  a.n_surv = per_q + 2 * (size_t)c.qb + q_at;
  a.info = info;
  NQ_HIP(ix, nq::launch_contain_share(a, ix->stream));
  if ((rc = c.ev.mark(2))) return rc;
  NQ_HIP(ix, nq::launch_contain_order(a, ix->stream));
  NQ_HIP(ix, nq::launch_collapse_scan(a.n_kept, n, d_off, ix->stream));
  struct {
    unsigned long long total;
    uint32_t info[nq::kContainInfoWords];
  } h = {0, {0, 0, 0}};
  NQ_HIP(ix, hipMemcpyAsync(&h, d_off + n, 8 + nq::kContainInfoWords * 4, hipMemcpyDeviceToHost, ix->stream));
  NQ_HIP(ix, hipStreamSynchronize(ix->stream));   // the leaf's one synchronisation of its own: the total sizes the stage
  if (h.info[nq::kContainInfoBadSize]) return fail(ix, NIQKI_E_INVALID, std::string(who) + ": a query size of 2^40 or more");
  if (h.info[nq::kContainInfoBad] || h.total > out.total) return fail(ix, NIQKI_E_STATE, std::string(who) + ": a hit outside the genome set (a bug)");
  ix->contain_stats.long_lists += h.info[nq::kContainInfoLong];
  const size_t entry = sizeof(nq::ContainedHit);
  if ((rc = ensure_keep(ix, ix->ws_ct_stage, (size_t)c.staged * entry, (size_t)std::max<uint64_t>(c.staged + h.total, 1) * entry))) return rc;
  NQ_HIP(ix, nq::launch_contain_emit(a, d_off, (nq::ContainedHit *)ix->ws_ct_stage.p + c.staged, ix->stream));
  if ((rc = c.ev.mark(3))) return rc;
  if ((rc = c.ev.add(0, 1, 0)) || (rc = c.ev.add(1, 2, 1)) || (rc = c.ev.add(2, 3, 2))) return rc;
  c.staged += h.total;
  return NIQKI_OK;
}

int contain_run(niqki_index *ix, const char *who, const SketchSource &src, const uint64_t *qsizes, uint32_t nq, uint32_t mode, uint32_t min_share,
                uint64_t *hit_off, uint32_t *hit_shares, uint32_t *hit_counts, uint32_t *hit_gids, uint32_t *n_unsized, uint64_t capacity,
                int mem) {
  ix->contain_stats = ContainStats();
  if (!whole_range(ix)) return fail(ix, NIQKI_E_STATE, std::string(who) + ": a slot-range shard sees partial counts; the contained query needs a whole-range handle");
  if (mode > NIQKI_CONTAIN_MAX) return fail(ix, NIQKI_E_INVALID, std::string(who) + ": mode " + std::to_string(mode) + " (NIQKI_CONTAIN_QUERY, _GENOME or _MAX)");
  const bool dev = mem == NIQKI_MEM_DEVICE;
  const uint32_t N = ix->n_genomes;
  if (N && !ix->sizes_set)
    return fail(ix, NIQKI_E_STATE, std::string(who) + ": no sizes on this genome set: call niqki_set_sizes (again, after genomes were added or dropped)");
  if (nq == 0 || N == 0) {
    if (dev) {
      NQ_HIP(ix, hipMemsetAsync(hit_off, 0, (size_t)(nq + 1) * 8, ix->stream));
      if (n_unsized && nq) NQ_HIP(ix, hipMemsetAsync(n_unsized, 0, (size_t)nq * 4, ix->stream));
    } else {
      std::fill(hit_off, hit_off + nq + 1, (uint64_t)0);
      if (n_unsized) std::fill(n_unsized, n_unsized + nq, 0u);
    }
    return NIQKI_OK;
  }
  if (!dev)   // (a device array is checked where the kernel reads it)
    for (uint32_t q = 0; q < nq; ++q)
      if (!nq::contain_size_fits(qsizes[q])) return fail(ix, NIQKI_E_INVALID, std::string(who) + ": a query size of 2^40 or more");
  CallParams guard(ix, ix->d.min_score, 0);   // the query path at the handle's threshold and no top-k
  int rc = build_if_needed(ix);
  if (rc) return rc;
  Contain c(ix);
  c.k = guard.k;
  c.mode = mode;
  c.min_share = min_share;
  if ((rc = c.ev.create())) return rc;
  const uint32_t qb = dev ? nq : std::max<uint32_t>(ix->query_batch, 1);
  c.qb = std::min(qb, nq);
  if ((rc = ensure(ix, ix->ws_ct_n, (size_t)c.qb * 12))) return rc;
  if (!dev && (rc = ensure(ix, ix->ws_ct_qs, (size_t)c.qb * 8))) return rc;
  // a batch's sketches, and its sizes beside them
  const SketchSource sized = [&](uint32_t q0, uint32_t n, const int32_t **d_sk) {
    int r = src(q0, n, d_sk);
    if (r) return r;
    if (dev) {
      c.d_qs = (const unsigned long long *)qsizes + q0;
    } else {
      NQ_HIP(ix, hipMemcpyAsync(ix->ws_ct_qs.p, qsizes + q0, (size_t)n * 8, hipMemcpyHostToDevice, ix->stream));
      c.d_qs = (const unsigned long long *)ix->ws_ct_qs.p;
    }
    return (int)NIQKI_OK;
  };
  std::vector<nq::ContainedHit> h_hits;
  std::vector<uint32_t> h_n;   // per query: kept, then (from nq on) unsized
  if (!dev) h_n.resize((size_t)nq * 2);
  uint64_t base = 0;
  HitLists hl{ix, who, c.ev, 0, ix->contain_stats.splits, false};
  hl.consume = [&](const HitOut &out, const int32_t *, uint32_t q_at, uint32_t n) { return contain_consume(c, who, out, q_at, n); };
  hl.after = [&](uint32_t q0, uint32_t n) {
    const nq::ContainedHit *stage = (const nq::ContainedHit *)ix->ws_ct_stage.p;
    const uint32_t *per_q = (const uint32_t *)ix->ws_ct_n.p;
    if (dev) {   // one batch: the offsets in any case, the rest where the caller's arrays hold the entries
      NQ_HIP(ix, nq::launch_collapse_scan(per_q, n, (unsigned long long *)hit_off, ix->stream));
      if (c.staged > capacity) return (int)NIQKI_E_CAPACITY;
      NQ_HIP(ix, nq::launch_contain_unpack(stage, c.staged, hit_shares, hit_counts, hit_gids, ix->stream));
      if (n_unsized) NQ_HIP(ix, hipMemcpyAsync(n_unsized, per_q + c.qb, (size_t)n * 4, hipMemcpyDeviceToDevice, ix->stream));
      return (int)NIQKI_OK;
    }
    // host arrays: nothing reaches the caller's arrays before the total is known
    h_hits.resize(base + c.staged);
    NQ_HIP(ix, hipMemcpyAsync(h_n.data() + q0, per_q, (size_t)n * 4, hipMemcpyDeviceToHost, ix->stream));
    NQ_HIP(ix, hipMemcpyAsync(h_n.data() + nq + q0, per_q + c.qb, (size_t)n * 4, hipMemcpyDeviceToHost, ix->stream));
    if (c.staged)
      NQ_HIP(ix, hipMemcpyAsync(h_hits.data() + base, stage, (size_t)c.staged * sizeof(nq::ContainedHit), hipMemcpyDeviceToHost, ix->stream));
    NQ_HIP(ix, hipStreamSynchronize(ix->stream));
    base += c.staged;
    c.staged = 0;   // (the next batch fills the stage from its start)
    return (int)NIQKI_OK;
  };
  if ((rc = hl.run(sized, nq, qb)) || dev) return rc;
  hit_off[0] = 0;
  for (uint32_t q = 0; q < nq; ++q) hit_off[q + 1] = hit_off[q] + h_n[q];
  if (hit_off[nq] != base) return fail(ix, NIQKI_E_STATE, std::string(who) + ": the kept counts and the entries disagree (a bug)");
  if (base > capacity) return NIQKI_E_CAPACITY;
  for (uint64_t j = 0; j < base; ++j) {
    hit_shares[j] = h_hits[j].share;
    hit_counts[j] = h_hits[j].count;
    hit_gids[j] = h_hits[j].gid;
  }
  if (n_unsized) std::copy(h_n.begin() + nq, h_n.end(), n_unsized);
  return NIQKI_OK;
}

}  // namespace

}  // namespace nqi

using namespace nqi;

extern "C" {

int niqki_set_sizes(niqki_index *ix, const uint64_t *sizes, uint32_t n, int mem) {
  if (!ix) return NIQKI_E_INVALID;
  if (!sizes || n == 0) {
    drop_sizes(ix);
    return NIQKI_OK;
  }
  if (n != ix->n_genomes) return fail(ix, NIQKI_E_INVALID, "niqki_set_sizes: " + std::to_string(n) + " sizes for " + std::to_string(ix->n_genomes) + " genomes");
  NQ_HIP(ix, hipSetDevice(ix->device));
  std::vector<uint64_t> h(n);
  if (mem == NIQKI_MEM_DEVICE) {
    NQ_HIP(ix, hipMemcpyAsync(h.data(), sizes, (size_t)n * 8, hipMemcpyDeviceToHost, ix->stream));
    NQ_HIP(ix, hipStreamSynchronize(ix->stream));
  } else {
    std::copy(sizes, sizes + n, h.begin());
  }
  for (uint32_t g = 0; g < n; ++g)
    if (!nq::contain_size_fits(h[g])) return fail(ix, NIQKI_E_INVALID, "niqki_set_sizes: the size of genome " + std::to_string(g) + " is 2^40 or more");
  drop_sizes(ix);
  int rc = ensure(ix, ix->sizes_dev, (size_t)n * 8);
  if (rc) return rc;
  NQ_HIP(ix, hipMemcpyAsync(ix->sizes_dev.p, h.data(), (size_t)n * 8, hipMemcpyHostToDevice, ix->stream));
  NQ_HIP(ix, hipStreamSynchronize(ix->stream));   // (h leaves scope)
  ix->sizes_set = true;
  return NIQKI_OK;
}

int niqki_query_contained(niqki_index *ix, const int32_t *sketches, const uint64_t *qsizes, uint32_t nq, uint32_t mode, uint32_t min_share,
                          uint64_t *hit_off, uint32_t *hit_shares, uint32_t *hit_counts, uint32_t *hit_gids, uint32_t *n_unsized,
                          uint64_t capacity, int mem) {
  if (!ix || !hit_off || ((!sketches || !qsizes) && nq) || (capacity && (!hit_shares || !hit_counts || !hit_gids))) return NIQKI_E_INVALID;
  NQ_HIP(ix, hipSetDevice(ix->device));
  return contain_run(ix, "niqki_query_contained", mem == NIQKI_MEM_DEVICE ? device_rows(ix, sketches) : host_rows(ix, sketches), qsizes, nq, mode,
                     min_share, hit_off, hit_shares, hit_counts, hit_gids, n_unsized, capacity, mem);
}

int niqki_staged_query_contained(niqki_index *ix, const uint64_t *qsizes, uint32_t mode, uint32_t min_share, uint64_t *hit_off,
                                 uint32_t *hit_shares, uint32_t *hit_counts, uint32_t *hit_gids, uint32_t *n_unsized, uint64_t capacity,
                                 int mem) {
  if (!ix || !hit_off || (capacity && (!hit_shares || !hit_counts || !hit_gids))) return NIQKI_E_INVALID;
  NQ_HIP(ix, hipSetDevice(ix->device));
  int rc = staged_sketch_ws(ix);
  if (rc) return rc;
  if (!qsizes && ix->staged.n_entry) return fail(ix, NIQKI_E_INVALID, "niqki_staged_query_contained: no query sizes");
  // (the staged sketches are only read, so niqki_staged_query answers as before)
  return contain_run(ix, "niqki_staged_query_contained", device_rows(ix, (const int32_t *)ix->ws_stsk.p), qsizes, ix->staged.n_entry, mode,
                     min_share, hit_off, hit_shares, hit_counts, hit_gids, n_unsized, capacity, mem);
}

}  // extern "C"
