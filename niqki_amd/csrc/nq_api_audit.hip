// nq_api_audit.hip -- niqki_audit behind the C ABI: the leave-one-out neighbours of every indexed genome read against
// the labelling of niqki_set_labels (niqki_hip.h).  One self-join (SelfJoin, nq_api_selfjoin.hip) at max(threshold, 1)
// whose consumer is the kernel of nq_audit.hip: a batch's ordered hit lists are the query path's own, so every count,
// the threshold, the order and the ties are the pinned path's, and the kernel writes seven words a genome where the
// lists lie.  The lists never leave the device.  DESIGN.md 4.6i.
#include "nq_handle.h"

#include <algorithm>
#include <string>

namespace nqi {

namespace {

constexpr int kAuditOuts = 7;   // verdict, own_count, own_gid, other_count, other_gid, vote_gid, vote_n

int audit_run(niqki_index *ix, uint32_t k, uint32_t *const user[kAuditOuts], int mem) {
  const uint32_t N = ix->n_genomes;
  const bool dev = mem == NIQKI_MEM_DEVICE;
  int rc = build_if_needed(ix);
  if (rc) return rc;
  // the info words, then (host results) seven arrays of N words
  const size_t head = nq::kAuditInfoWords;
  if ((rc = ensure(ix, ix->ws_audit, (head + (dev ? 0 : (size_t)kAuditOuts * N)) * 4))) return rc;
  uint32_t *info = (uint32_t *)ix->ws_audit.p, *out[kAuditOuts];
  for (int j = 0; j < kAuditOuts; ++j) out[j] = dev ? user[j] : user[j] ? info + head + (size_t)j * N : nullptr;
  SelfJoin r(ix, "niqki_audit", ix->audit_stats, 3);
  r.count_pairs = true;
  r.consume = [&](const unsigned long long *off, const uint32_t *hc, const uint32_t *hg, uint32_t t0, uint32_t n) {
    nq::AuditArgs a{};
    a.hit_off = off;
    a.hit_counts = hc;
    a.hit_gids = hg;
    a.labels = (const uint32_t *)ix->lab_dense.p;
    a.n_genomes = N;
    a.t0 = t0;
    a.nq = n;   // (the kernel writes no row at or above N)
    a.k = k;
    a.verdict = out[0];
    a.own_count = out[1];
    a.own_gid = out[2];
    a.other_count = out[3];
    a.other_gid = out[4];
    a.vote_gid = out[5];
    a.vote_n = out[6];
    a.info = info;
    NQ_HIP(ix, nq::launch_audit(a, ix->stream));
    return r.ev.mark(4);
  };
  NQ_HIP(ix, hipMemsetAsync(info, 0, nq::kAuditInfoWords * 4, ix->stream));
  if ((rc = self_join_batches(r, N))) return rc;
  uint32_t got[nq::kAuditInfoWords] = {0};
  if (!dev)
    for (int j = 0; j < kAuditOuts; ++j)
      if (user[j]) NQ_HIP(ix, hipMemcpyAsync(user[j], out[j], (size_t)N * 4, hipMemcpyDeviceToHost, ix->stream));
  NQ_HIP(ix, hipMemcpyAsync(got, info, sizeof got, hipMemcpyDeviceToHost, ix->stream));
  NQ_HIP(ix, hipStreamSynchronize(ix->stream));
  if (got[nq::kAuditInfoBad]) return fail(ix, NIQKI_E_STATE, "niqki_audit: a hit outside the index or a list longer than it (a bug)");
  return NIQKI_OK;
}

}  // namespace

}  // namespace nqi

using namespace nqi;

extern "C" {

int niqki_audit(niqki_index *ix, uint32_t threshold, uint32_t k, uint32_t *verdict, uint32_t *own_count, uint32_t *own_gid,
                uint32_t *other_count, uint32_t *other_gid, uint32_t *vote_gid, uint32_t *vote_n, int mem) {
  if (!ix) return NIQKI_E_INVALID;
  if (k < 1 || k > nq::kAuditMaxK) return fail(ix, NIQKI_E_INVALID, "niqki_audit: k " + std::to_string(k) + " is not in 1..63");
  if (!whole_range(ix)) return fail(ix, NIQKI_E_STATE, "niqki_audit: a slot-range shard sees partial counts; the self-join needs a whole-range handle");
  NQ_HIP(ix, hipSetDevice(ix->device));
  ix->audit_stats = SelfJoinStats();
  if (ix->n_genomes == 0) return NIQKI_OK;   // (also without a labelling, which an empty index cannot have)
  if (!ix->labels_set)
    return fail(ix, NIQKI_E_STATE, "niqki_audit: no labels on this genome set: call niqki_set_labels (again, after genomes were added or dropped)");
  uint32_t *const user[kAuditOuts] = {verdict, own_count, own_gid, other_count, other_gid, vote_gid, vote_n};
  CallParams guard(ix, std::max(threshold, 1u), 0);
  return audit_run(ix, k, user, mem);
}

}  // extern "C"
