// nq_api_tally.hip -- niqki_tally_begin, niqki_tally_add, niqki_tally_read and niqki_tally_end behind the C ABI: the
// result rows of the LCA calls counted per taxon and per clade on the device (niqki_hip.h).  The accumulators sit
// beside the taxonomy; nq_api_lca.hip hands every leaf's rows to tally_rows_dev while a tally is open, and a read adds
// every taxon's counts to its ancestors'.  Nothing here looks at a hit or at the index.  DESIGN.md 4.5g.
#include "nq_handle.h"

#include <algorithm>
#include <string>

namespace nqi {

namespace {

constexpr uint32_t kStageRows = 1u << 20;   // rows of a host call staged at a time (12 MiB)

unsigned long long *tally_words(niqki_index *ix) { return (unsigned long long *)ix->tally_acc.p; }
// array j of the accumulators: 0 direct, 1 direct_best, 2 clade, 3 clade_best
unsigned long long *tally_array(niqki_index *ix, int j) { return tally_words(ix) + nq::kTallyWords + (size_t)j * ix->tally_taxa; }

// E_STATE unless a tally is open
int tally_usable(niqki_index *ix, const char *who) {
  if (ix->tally_state == 1) return NIQKI_OK;
  if (ix->tally_state == 2) return fail(ix, NIQKI_E_STATE, std::string(who) + ": the tally is broken (" + ix->tally_why + "); niqki_tally_begin starts afresh");
  return fail(ix, NIQKI_E_STATE, std::string(who) + ": no tally is open: call niqki_tally_begin (again, after the taxonomy was set or dropped)");
}

// the bad rows counted so far; synchronises
int tally_bad_rows(niqki_index *ix, unsigned long long *bad) {
  NQ_HIP(ix, hipMemcpyAsync(bad, tally_words(ix) + nq::kTallyBad, 8, hipMemcpyDeviceToHost, ix->stream));
  NQ_HIP(ix, hipStreamSynchronize(ix->stream));
  return NIQKI_OK;
}

int tally_bad(niqki_index *ix, const char *who, unsigned long long bad) {
  break_tally(ix, std::to_string(bad) + " bad rows were added beside good ones");
  return fail(ix, NIQKI_E_INVALID, std::string(who) + ": " + std::to_string(bad) + " bad rows (a taxon that is neither below " + std::to_string(ix->tally_taxa) +
                                       " nor NIQKI_TAXON_NONE); the other rows were added, the tally is broken");
}

}  // namespace

void end_tally(niqki_index *ix) {
  ix->tally_state = 0;
  ix->tally_queries = 0;
  ix->tally_why.clear();
}

void break_tally(niqki_index *ix, const std::string &why) {
  if (ix->tally_state != 1) return;
  ix->tally_state = 2;
  ix->tally_why = why;
}

int tally_rows_dev(niqki_index *ix, const uint32_t *taxon, const uint32_t *best_count, const uint32_t *considered, uint32_t n) {
  nq::TallyArgs a{};
  a.taxon = taxon;
  a.best_count = best_count;
  a.considered = considered;
  a.n = n;
  a.n_taxa = ix->tally_taxa;
  a.direct = tally_array(ix, 0);
  a.direct_best = tally_array(ix, 1);
  a.words = tally_words(ix);
  NQ_HIP(ix, nq::launch_tally_rows(a, ix->stream));
  return NIQKI_OK;
}

}  // namespace nqi

using namespace nqi;

extern "C" {

int niqki_tally_begin(niqki_index *ix) {
  if (!ix) return NIQKI_E_INVALID;
  if (!whole_range(ix)) return fail(ix, NIQKI_E_STATE, "niqki_tally_begin: a slot-range shard has no LCA query and no tally");
  if (!ix->tax_set) return fail(ix, NIQKI_E_STATE, "niqki_tally_begin: no taxonomy on this genome set: call niqki_set_taxonomy first");
  NQ_HIP(ix, hipSetDevice(ix->device));
  end_tally(ix);
  const size_t bytes = ((size_t)nq::kTallyWords + 4 * (size_t)ix->n_taxa) * 8;
  int rc = ensure(ix, ix->tally_acc, bytes);   // (earlier launches on the stream are through with a buffer hipFree releases)
  if (rc) return rc;
  ix->tally_taxa = ix->n_taxa;
  NQ_HIP(ix, hipMemsetAsync(ix->tally_acc.p, 0, bytes, ix->stream));
  ix->tally_ms[0] = ix->tally_ms[1] = 0;
  ix->tally_state = 1;
  return NIQKI_OK;
}

int niqki_tally_add(niqki_index *ix, const uint32_t *taxon, const uint32_t *best_count, const uint32_t *considered, uint32_t n, int mem) {
  if (!ix || (!taxon && n)) return NIQKI_E_INVALID;
  const char *who = "niqki_tally_add";
  int rc = tally_usable(ix, who);
  if (rc) return rc;
  if (n == 0) return NIQKI_OK;
  NQ_HIP(ix, hipSetDevice(ix->device));
  ix->tally_ms[0] = 0;
  PhaseTimer ev(ix, 2, ix->tally_ms);
  if ((rc = ev.create())) return rc;
  if (mem == NIQKI_MEM_DEVICE) {   // in stream order, no synchronise: bad rows show at the next read
    if ((rc = ev.mark(0)) || (rc = tally_rows_dev(ix, taxon, best_count, considered, n))) {
      break_tally(ix, "an add call failed");
      return rc;
    }
    if ((rc = ev.mark(1))) return rc;
    return ev.add(0, 1, 0);
  }
  const uint32_t room = std::min(n, kStageRows);
  if ((rc = ensure(ix, ix->ws_tally_rows, (size_t)room * 12))) return rc;
  uint32_t *d[3] = {(uint32_t *)ix->ws_tally_rows.p, (uint32_t *)ix->ws_tally_rows.p + room, (uint32_t *)ix->ws_tally_rows.p + 2 * (size_t)room};
  const uint32_t *h[3] = {taxon, best_count, considered};
  const auto chunks = [&]() -> int {
    for (uint32_t at = 0; at < n; at += room) {
      const uint32_t m = std::min(room, n - at);
      for (int j = 0; j < 3; ++j)
        if (h[j]) NQ_HIP(ix, hipMemcpyAsync(d[j], h[j] + at, (size_t)m * 4, hipMemcpyHostToDevice, ix->stream));
      int r;
      if ((r = ev.mark(0)) || (r = tally_rows_dev(ix, d[0], h[1] ? d[1] : nullptr, h[2] ? d[2] : nullptr, m)) || (r = ev.mark(1)) || (r = ev.add(0, 1, 0))) return r;
    }
    return NIQKI_OK;
  };
  unsigned long long bad = 0;
  if ((rc = chunks()) || (rc = tally_bad_rows(ix, &bad))) {
    break_tally(ix, "an add call failed");
    return rc;
  }
  return bad ? tally_bad(ix, who, bad) : NIQKI_OK;
}

int niqki_tally_read(niqki_index *ix, uint64_t *direct, uint64_t *clade, uint64_t *direct_best, uint64_t *clade_best, niqki_tally_totals *totals,
                     int mem) {
  if (!ix) return NIQKI_E_INVALID;
  const char *who = "niqki_tally_read";
  int rc = tally_usable(ix, who);
  if (rc) return rc;
  NQ_HIP(ix, hipSetDevice(ix->device));
  const uint32_t T = ix->tally_taxa;
  ix->tally_ms[1] = 0;
  PhaseTimer ev(ix, 2, ix->tally_ms);
  if ((rc = ev.create())) return rc;
  // the clades anew from the direct counts: a read changes nothing a later read or add depends on
  NQ_HIP(ix, hipMemsetAsync(tally_array(ix, 2), 0, (size_t)T * 16, ix->stream));
  nq::TallyCladeArgs a{};
  a.nodes = (const nq::TaxNode *)ix->tax_nodes.p;
  a.n_taxa = T;
  a.max_depth = ix->tax_depth;
  a.direct = tally_array(ix, 0);
  a.direct_best = tally_array(ix, 1);
  a.clade = tally_array(ix, 2);
  a.clade_best = tally_array(ix, 3);
  if ((rc = ev.mark(0))) return rc;
  NQ_HIP(ix, nq::launch_tally_clade(a, ix->stream));
  if ((rc = ev.mark(1))) return rc;
  unsigned long long w[nq::kTallyWords] = {0, 0, 0, 0};
  NQ_HIP(ix, hipMemcpyAsync(w, tally_words(ix), sizeof w, hipMemcpyDeviceToHost, ix->stream));
  uint64_t *const user[4] = {direct, direct_best, clade, clade_best};
  for (int j = 0; j < 4; ++j)
    if (user[j] && T)
      NQ_HIP(ix, hipMemcpyAsync(user[j], tally_array(ix, j), (size_t)T * 8, mem == NIQKI_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ix->stream));
  NQ_HIP(ix, hipStreamSynchronize(ix->stream));
  if ((rc = ev.add(0, 1, 1))) return rc;
  if (w[nq::kTallyBad]) return tally_bad(ix, who, w[nq::kTallyBad]);   // (rows of an add call in device memory)
  ix->tally_queries = w[nq::kTallyClassified] + w[nq::kTallyNoHit] + w[nq::kTallyNoCommon];
  if (totals) {
    totals->queries = ix->tally_queries;
    totals->classified = w[nq::kTallyClassified];
    totals->no_hit = w[nq::kTallyNoHit];
    totals->no_common = w[nq::kTallyNoCommon];
  }
  return NIQKI_OK;
}

int niqki_tally_end(niqki_index *ix) {
  if (!ix) return NIQKI_E_INVALID;
  end_tally(ix);
  return NIQKI_OK;
}

}  // extern "C"
