// nq_api_lca.hip -- niqki_set_taxonomy, niqki_query_lca and niqki_staged_query_lca behind the C ABI: per query the
// lowest taxon that holds all its near-best hits (niqki_hip.h).  A batch's full lists are the query path's own
// (query_hits_dev at top_k = 0 into the handle's hit buffers, within the budget of the self-join calls), so every count,
// the threshold, the order and the ties are the pinned path's; the kernel of nq_lca.hip only folds a prefix of them.
// The lists never leave the device: four words a query do.  DESIGN.md 4.5e.
#include "nq_handle.h"

#include <algorithm>
#include <string>
#include <vector>

namespace nqi {

void drop_taxonomy(niqki_index *ix) {
  ix->tax_set = false;
  ix->n_taxa = 0;
  ix->tax_depth = 0;
  end_tally(ix);   // (niqki_tally_begin: the tally belongs to the taxonomy)
}

namespace {

struct Lca {
  niqki_index *ix;
  PhaseTimer ev;   // events of a leaf: 0-1 hits, 1-2 fold, 2-3 the rows into an open tally
  bool tally = false;   // a tally is open: every leaf's rows go into it (out[0], out[1] and out[3] are all there)
  uint32_t top_permille = 0;
  uint32_t *out[4] = {nullptr, nullptr, nullptr, nullptr};   // device rows of the batch: taxon, best_count, best_gid, considered
  explicit Lca(niqki_index *ix_) : ix(ix_), ev(ix_, 4, ix_->lca_stats.ms) {}
};

// The consumer of a leaf (HitLists): the full lists `hits` of queries [q_at, q_at + n) of the batch; one launch that
// writes the leaf's result rows at q_at.
int lca_consume(Lca &c, const HitOut &hits, uint32_t q_at, uint32_t n) {
  niqki_index *ix = c.ix;
  int rc;
  if ((rc = c.ev.mark(1))) return rc;
  nq::LcaArgs a{};
  a.hit_off = hits.off;
  a.hit_counts = hits.counts;
  a.hit_gids = hits.gids;
  a.nodes = (const nq::TaxNode *)ix->tax_nodes.p;
  a.genome_taxon = (const uint32_t *)ix->tax_genome.p;
  a.n_genomes = ix->n_genomes;
  a.n_taxa = ix->n_taxa;
  a.max_depth = ix->tax_depth;
  a.nq = n;
  a.top_permille = c.top_permille;
  a.wave_cap = ix->lca_wave_cap;
  a.taxon = c.out[0] + q_at;
  a.best_count = c.out[1] ? c.out[1] + q_at : nullptr;
  a.best_gid = c.out[2] ? c.out[2] + q_at : nullptr;
  a.considered = c.out[3] ? c.out[3] + q_at : nullptr;
  a.info = (uint32_t *)ix->ws_lca_info.p;
  NQ_HIP(ix, nq::launch_lca(a, ix->stream));
  if ((rc = c.ev.mark(2))) return rc;
  if (c.tally) {   // the rows the caller gets, exactly once: a halved batch comes here leaf by leaf
    if ((rc = tally_rows_dev(ix, c.out[0] + q_at, c.out[1] + q_at, c.out[3] + q_at, n))) return rc;
    if ((rc = c.ev.mark(3))) return rc;
  }
  if ((rc = c.ev.add(0, 1, 0)) || (rc = c.ev.add(1, 2, 1))) return rc;
  if (c.tally && (rc = c.ev.add(2, 3, 2))) return rc;
  return NIQKI_OK;
}

// an open tally that a failing call leaves with part of its rows is broken; a call that ends well disarms it
struct TallyGuard {
  niqki_index *ix;
  const char *who;
  bool armed = false;
  ~TallyGuard() {
    if (armed) break_tally(ix, std::string(who) + " failed after its first batch had begun");
  }
};

// rows [0, n) of a query without a hit
int lca_no_hit(niqki_index *ix, uint32_t *const out[4], uint32_t n, bool dev) {
  static const int fill[4] = {0xFF, 0, 0xFF, 0};   // NIQKI_TAXON_NONE, 0, 0xFFFFFFFF, 0
  for (int j = 0; j < 4; ++j) {
    if (!out[j] || !n) continue;
    if (dev) NQ_HIP(ix, hipMemsetAsync(out[j], fill[j], (size_t)n * 4, ix->stream));
    else std::fill(out[j], out[j] + n, fill[j] ? 0xFFFFFFFFu : 0u);
  }
  return NIQKI_OK;
}

int lca_run(niqki_index *ix, const char *who, const SketchSource &src, uint32_t nq, uint32_t top_permille, uint32_t *taxon,
            uint32_t *best_count, uint32_t *best_gid, uint32_t *considered, int mem) {
  ix->lca_stats = LcaStats();
  if (!whole_range(ix)) return fail(ix, NIQKI_E_STATE, std::string(who) + ": a slot-range shard sees partial counts; the LCA query needs a whole-range handle");
  if (top_permille > 1000) return fail(ix, NIQKI_E_INVALID, std::string(who) + ": top_permille " + std::to_string(top_permille) + " is above 1000");
  const bool dev = mem == NIQKI_MEM_DEVICE;
  const uint32_t N = ix->n_genomes;
  if (N && !ix->tax_set)
    return fail(ix, NIQKI_E_STATE, std::string(who) + ": no taxonomy on this genome set: call niqki_set_taxonomy (again, after genomes were added or dropped)");
  uint32_t *const user[4] = {taxon, best_count, best_gid, considered};
  const bool tally = ix->tally_state == 1;
  if (tally) ix->tally_ms[0] = 0;
  if (nq == 0 || N == 0) {   // (no genomes under a taxonomy of taxa alone: every row is a no-hit row)
    if (!tally || !nq) return lca_no_hit(ix, user, nq, dev);
    // the rows go into the tally from a workspace of the library's (the caller's may be host memory or left out), after
    // they were written: rows that were not returned are not added
    int rc = ensure(ix, ix->ws_tally_rows, (size_t)nq * 4);
    if (rc || (rc = lca_no_hit(ix, user, nq, dev))) return rc;
    const auto add = [&]() -> int {
      NQ_HIP(ix, hipMemsetAsync(ix->ws_tally_rows.p, 0xFF, (size_t)nq * 4, ix->stream));
      return tally_rows_dev(ix, (const uint32_t *)ix->ws_tally_rows.p, nullptr, nullptr, nq);
    };
    if ((rc = add())) break_tally(ix, std::string(who) + " failed while its rows were added");
    return rc;
  }
  CallParams guard(ix, ix->d.min_score, 0);   // the query path at the handle's threshold and no top-k
  int rc = build_if_needed(ix);
  if (rc) return rc;
  Lca c(ix);
  c.top_permille = top_permille;
  c.tally = tally;
  if ((rc = c.ev.create())) return rc;
  const uint32_t qb = dev ? nq : std::max<uint32_t>(ix->query_batch, 1);
  const uint32_t rows = std::min(qb, nq);
  if ((rc = ensure(ix, ix->ws_lca_info, nq::kLcaInfoWords * 4))) return rc;
  NQ_HIP(ix, hipMemsetAsync(ix->ws_lca_info.p, 0, nq::kLcaInfoWords * 4, ix->stream));
  const auto wanted = [&](int j) { return user[j] || (tally && (j == 1 || j == 3)); };   // (the tally reads best_count and considered)
  if (dev) {
    for (int j = 0; j < 4; ++j) c.out[j] = user[j];
    if (tally && (!user[1] || !user[3])) {   // ... in a workspace of the library's where the caller left them out
      if ((rc = ensure(ix, ix->ws_tally_rows, (size_t)nq * 8))) return rc;
      if (!user[1]) c.out[1] = (uint32_t *)ix->ws_tally_rows.p;
      if (!user[3]) c.out[3] = (uint32_t *)ix->ws_tally_rows.p + nq;
    }
  } else {   // a batch's rows: four arrays of `rows` words, the ones nobody asked for left out
    if ((rc = ensure(ix, ix->ws_lca_out, (size_t)rows * 16))) return rc;
    for (int j = 0; j < 4; ++j) c.out[j] = wanted(j) ? (uint32_t *)ix->ws_lca_out.p + (size_t)j * rows : nullptr;
  }
  TallyGuard guard_tally{ix, who, tally};
  HitLists hl{ix, who, c.ev, 0, ix->lca_stats.splits, false};
  hl.consume = [&](const HitOut &hits, const int32_t *, uint32_t q_at, uint32_t n) { return lca_consume(c, hits, q_at, n); };
  if (!dev)   // (device memory: one batch, its rows are the caller's)
    hl.after = [&](uint32_t q0, uint32_t n) {
      for (int j = 0; j < 4; ++j)
        if (user[j]) NQ_HIP(ix, hipMemcpyAsync(user[j] + q0, c.out[j], (size_t)n * 4, hipMemcpyDeviceToHost, ix->stream));
      NQ_HIP(ix, hipStreamSynchronize(ix->stream));   // (the next batch writes the same rows)
      return (int)NIQKI_OK;
    };
  if ((rc = hl.run(src, nq, qb))) return rc;
  uint32_t info[nq::kLcaInfoWords] = {0, 0, 0};
  NQ_HIP(ix, hipMemcpyAsync(info, ix->ws_lca_info.p, sizeof info, hipMemcpyDeviceToHost, ix->stream));
  NQ_HIP(ix, hipStreamSynchronize(ix->stream));
  if (info[nq::kLcaInfoBad]) return fail(ix, NIQKI_E_STATE, std::string(who) + ": a hit outside the index or a taxon outside the taxonomy (a bug)");
  ix->lca_stats.long_lists = info[nq::kLcaInfoLong];
  ix->lca_stats.no_common = info[nq::kLcaInfoNoCommon];
  guard_tally.armed = false;
  if (tally) ix->tally_ms[0] = ix->lca_stats.ms[2];
  return NIQKI_OK;
}


}  // namespace

}  // namespace nqi

using namespace nqi;

extern "C" {

int niqki_set_taxonomy(niqki_index *ix, const uint32_t *genome_taxon, uint32_t n_genomes, const uint32_t *parent, uint32_t n_taxa, int mem) {
  if (!ix) return NIQKI_E_INVALID;
  if (!genome_taxon || !parent || n_taxa == 0) {
    drop_taxonomy(ix);
    return NIQKI_OK;
  }
  const char *who = "niqki_set_taxonomy: ";
  if (n_genomes != ix->n_genomes)
    return fail(ix, NIQKI_E_INVALID, who + std::to_string(n_genomes) + " genome taxa for " + std::to_string(ix->n_genomes) + " genomes");
  if (n_taxa >= 0xFFFFFFFEu) return fail(ix, NIQKI_E_INVALID, who + std::to_string(n_taxa) + " taxa: the count must be below 4294967294");
  NQ_HIP(ix, hipSetDevice(ix->device));
  std::vector<uint32_t> gt(n_genomes), par(n_taxa);
  if (mem == NIQKI_MEM_DEVICE) {
    if (n_genomes) NQ_HIP(ix, hipMemcpyAsync(gt.data(), genome_taxon, (size_t)n_genomes * 4, hipMemcpyDeviceToHost, ix->stream));
    NQ_HIP(ix, hipMemcpyAsync(par.data(), parent, (size_t)n_taxa * 4, hipMemcpyDeviceToHost, ix->stream));
    NQ_HIP(ix, hipStreamSynchronize(ix->stream));
  } else {
    std::copy(genome_taxon, genome_taxon + n_genomes, gt.begin());
    std::copy(parent, parent + n_taxa, par.begin());
  }
  // validation and depths: one-off work on the host
  for (uint32_t g = 0; g < n_genomes; ++g)
    if (gt[g] >= n_taxa)
      return fail(ix, NIQKI_E_INVALID, who + std::string("genome ") + std::to_string(g) + " has taxon " + std::to_string(gt[g]) + ", not below " + std::to_string(n_taxa));
  for (uint32_t t = 0; t < n_taxa; ++t)
    if (par[t] >= n_taxa)
      return fail(ix, NIQKI_E_INVALID, who + std::string("taxon ") + std::to_string(t) + " has parent " + std::to_string(par[t]) + ", not below " + std::to_string(n_taxa));
  // every taxon's depth from the first settled ancestor above it; a walk that meets its own trail has found a cycle
  std::vector<nq::TaxNode> nodes(n_taxa);
  std::vector<uint8_t> state(n_taxa, 0);   // 0 = untouched, 1 = on the trail of the walk under way, 2 = settled
  std::vector<uint32_t> trail;
  uint32_t deepest = 0;
  for (uint32_t t0 = 0; t0 < n_taxa; ++t0) {
    if (state[t0]) continue;
    trail.clear();
    uint32_t t = t0, d = 0;
    for (;;) {
      if (state[t] == 2) {
        d = nodes[t].depth + 1;
        break;
      }
      if (state[t] == 1) return fail(ix, NIQKI_E_INVALID, who + std::string("taxon ") + std::to_string(t) + " lies on a cycle of parents");
      if (par[t] == t) {   // a root
        nodes[t] = nq::TaxNode{t, 0};
        state[t] = 2;
        d = 1;
        break;
      }
      state[t] = 1;
      trail.push_back(t);
      t = par[t];
    }
    for (size_t j = trail.size(); j-- > 0;) {
      const uint32_t u = trail[j];
      nodes[u] = nq::TaxNode{par[u], d};
      state[u] = 2;
      deepest = std::max(deepest, d);
      d += 1;
    }
  }
  Buf nb, gb;   // the new arrays first: the taxonomy the handle had stays when memory runs out
  int rc = ensure(ix, nb, (size_t)n_taxa * sizeof(nq::TaxNode));
  if (!rc) rc = ensure(ix, gb, std::max<size_t>((size_t)n_genomes * 4, 4));
  if (rc) {
    if (nb.p) (void)hipFree(nb.p);
    return rc;
  }
  hipError_t e = hipMemcpyAsync(nb.p, nodes.data(), (size_t)n_taxa * sizeof(nq::TaxNode), hipMemcpyHostToDevice, ix->stream);
  if (e == hipSuccess && n_genomes) e = hipMemcpyAsync(gb.p, gt.data(), (size_t)n_genomes * 4, hipMemcpyHostToDevice, ix->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ix->stream);   // (the vectors leave scope; earlier launches are through with the old arrays)
  if (e != hipSuccess) {
    (void)hipFree(nb.p);
    (void)hipFree(gb.p);
    NQ_HIP(ix, e);
  }
  if (ix->tax_nodes.p) (void)hipFree(ix->tax_nodes.p);
  if (ix->tax_genome.p) (void)hipFree(ix->tax_genome.p);
  ix->tax_nodes = nb;
  ix->tax_genome = gb;
  ix->n_taxa = n_taxa;
  ix->tax_depth = deepest;
  ix->tax_set = true;
  end_tally(ix);   // (a tally counted under the taxonomy this one replaces)
  return NIQKI_OK;
}

int niqki_query_lca(niqki_index *ix, const int32_t *sketches, uint32_t nq, uint32_t top_permille, uint32_t *taxon, uint32_t *best_count,
                    uint32_t *best_gid, uint32_t *considered, int mem) {
  if (!ix || ((!sketches || !taxon) && nq)) return NIQKI_E_INVALID;
  NQ_HIP(ix, hipSetDevice(ix->device));
  return lca_run(ix, "niqki_query_lca", mem == NIQKI_MEM_DEVICE ? device_rows(ix, sketches) : host_rows(ix, sketches), nq, top_permille, taxon,
                 best_count, best_gid, considered, mem);
}

int niqki_staged_query_lca(niqki_index *ix, uint32_t top_permille, uint32_t *taxon, uint32_t *best_count, uint32_t *best_gid,
                           uint32_t *considered, int mem) {
  if (!ix) return NIQKI_E_INVALID;
  NQ_HIP(ix, hipSetDevice(ix->device));
  int rc = staged_sketch_ws(ix);
  if (rc) return rc;
  if (!taxon && ix->staged.n_entry) return NIQKI_E_INVALID;
  // (the staged sketches are only read, so niqki_staged_query answers as before)
  return lca_run(ix, "niqki_staged_query_lca", device_rows(ix, (const int32_t *)ix->ws_stsk.p), ix->staged.n_entry, top_permille, taxon,
                 best_count, best_gid, considered, mem);
}

}  // extern "C"
