// nq_api_lists.hip -- what the calls that consume full hit lists on the device share (nq_handle.h, "full hit lists"):
// the guard of a call's query parameters, the phase timer, the room of the fixed hit buffers, the halving leaf with its
// batch loop, and the buffer growth that keeps what a batch has written.  The consumers are nq_api_selfjoin.hip,
// nq_api_audit.hip, nq_api_cover.hip, nq_api_collapse.hip, nq_api_contain.hip and nq_api_lca.hip.  DESIGN.md 4.5f.
#include "nq_handle.h"

#include <algorithm>
#include <string>

namespace nqi {

CallParams::CallParams(niqki_index *ix_, uint32_t min_score, uint32_t top_k)
    : ix(ix_), ms(ix_->d.min_score), pms(ix_->p.min_score), k(ix_->p.top_k) {
  ix->d.min_score = min_score;
  ix->p.min_score = min_score;
  ix->p.top_k = top_k;
}
CallParams::~CallParams() {
  ix->d.min_score = ms;
  ix->p.min_score = pms;
  ix->p.top_k = k;
}

PhaseTimer::~PhaseTimer() {
  for (auto &e : ev) if (e) (void)hipEventDestroy(e);
}
int PhaseTimer::create() {
  if (ix->prof) for (auto &e : ev) NQ_HIP(ix, hipEventCreate(&e));
  return NIQKI_OK;
}
int PhaseTimer::mark(int k) {
  if (ix->prof) NQ_HIP(ix, hipEventRecord(ev[k], ix->stream));
  return NIQKI_OK;
}
int PhaseTimer::add(int a, int b, int to) {
  if (!ix->prof) return NIQKI_OK;
  float t = 0;
  NQ_HIP(ix, hipEventSynchronize(ev[b]));
  NQ_HIP(ix, hipEventElapsedTime(&t, ev[a], ev[b]));
  ms[to] += t;
  return NIQKI_OK;
}

// hit_counts + hit_gids and the two scratch arrays of the same size the hit kernels order them in: 16 bytes a hit;
// never below N, the hits of one query
uint64_t hit_room(const niqki_index *ix) {
  return std::max<uint64_t>(((uint64_t)std::max<uint32_t>(ix->cluster_ws_mib, 1) << 20) / 16, ix->n_genomes);
}

int ensure_keep(niqki_index *ix, Buf &b, size_t keep, size_t bytes) {
  if (bytes <= b.n && b.p) return NIQKI_OK;
  if (!keep) return ensure(ix, b, bytes);
  Buf nb;
  int rc = ensure(ix, nb, bytes * 2);
  if (rc) return rc;
  NQ_HIP(ix, hipMemcpyAsync(nb.p, b.p, keep, hipMemcpyDeviceToDevice, ix->stream));
  NQ_HIP(ix, hipStreamSynchronize(ix->stream));
  NQ_HIP(ix, hipFree(b.p));
  b = nb;
  return NIQKI_OK;
}

// The total is known only after the gather and the count, so a split loses that work.
int HitLists::leaf(const int32_t *d_sk, uint32_t q_at, uint32_t n, uint32_t *fitted) {
  const uint64_t stride = NIQKI_ROW_STRIDE(ix->n_genomes);
  int rc;
  Planes pl;
  HitOut out;
  if ((rc = counter_planes(ix, n, stride, pl))) return rc;
  if ((rc = hit_out_ws(ix, n, hit_room(ix), out))) return rc;
  if ((rc = ev.mark(ev_hits))) return rc;
  rc = query_hits_dev(ix, d_sk, n, pl, stride, out);
  if (rc == NIQKI_E_CAPACITY) {
    if (n == 1) return fail(ix, NIQKI_E_STATE, std::string(who) + ": one query's hits exceed the genome count");   // (room >= N)
    splits += 1;
    const uint32_t h = n / 2;
    uint32_t f1 = 0, f2 = 0;
    if ((rc = leaf(d_sk, q_at, h, &f1))) return rc;
    if ((rc = leaf(d_sk + (size_t)h * ix->d.F, q_at + h, n - h, &f2))) return rc;
    *fitted = std::max(1u, std::min(f1, f2));
    return NIQKI_OK;
  }
  if (rc) return rc;
  *fitted = n;
  return consume(out, d_sk, q_at, n);
}

int HitLists::run(const SketchSource &src, uint32_t nq, uint32_t qb) {
  int rc;
  for (q0 = 0; q0 < nq;) {
    const uint32_t n = std::min(qb, nq - q0);
    const int32_t *d_sk = nullptr;
    uint32_t fitted = n;
    if ((rc = src(q0, n, &d_sk))) return rc;
    if ((rc = leaf(d_sk, 0, n, &fitted))) return rc;
    if (after && (rc = after(q0, n))) return rc;
    if (shrink && fitted < n) qb = fitted;   // a split batch: do not gather the following ones twice
    q0 += n;
  }
  return NIQKI_OK;
}

}  // namespace nqi
