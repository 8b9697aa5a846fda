// nq_api_cover.hip -- niqki_cover / niqki_staged_cover behind the C ABI: the greedy cover of a query (niqki_hip.h).
// A round is the query path itself (query_hits_dev at top_k = 1 on the masked sketches of the still-active queries),
// so every count and every tie is the pinned path's; the kernels of nq_cover.hip only mask the winner's slots, keep
// the active rows together and turn the pick log into lists.  The host reads four words back per round and bounds the
// rounds; nothing on the device waits.  DESIGN.md 4.5c.
#include "nq_handle.h"

#include <algorithm>
#include <string>
#include <vector>

namespace nqi {

namespace {

// The rounds of one batch: n queries whose sketches as given lie at d_orig.  Leaves the pick log (*n_log entries in
// ws_cv_log) and the per-query pick counts (*n_picks, device) and returns the batch's picks.
int cover_rounds(niqki_index *ix, const int32_t *d_orig, uint32_t n, uint32_t max_picks, uint32_t bound, PhaseTimer &ev, uint64_t *n_log,
                 uint64_t *picks, const uint32_t **n_picks) {
  const uint32_t F = ix->d.F, N = ix->n_genomes;
  const uint64_t stride = NIQKI_ROW_STRIDE(ix->built_n);
  int rc;
  for (auto &b : ix->ws_cv_sk)
    if ((rc = ensure(ix, b, (size_t)n * F * 4))) return rc;
  // qidx[2][n], flag[n], pos[n + 1], n_picks[n], info
  if ((rc = ensure(ix, ix->ws_cv_idx, ((size_t)n * 5 + 1 + nq::kCoverInfoWords) * 4))) return rc;
  uint32_t *qidx[2] = {(uint32_t *)ix->ws_cv_idx.p, (uint32_t *)ix->ws_cv_idx.p + n};
  uint32_t *flag = qidx[1] + n, *pos = flag + n, *npk = pos + n + 1, *info = npk + n;
  int32_t *sk[2] = {(int32_t *)ix->ws_cv_sk[0].p, (int32_t *)ix->ws_cv_sk[1].p};
  NQ_HIP(ix, hipMemcpyAsync(sk[0], d_orig, (size_t)n * F * 4, hipMemcpyDeviceToDevice, ix->stream));
  NQ_HIP(ix, hipMemsetAsync(info, 0, nq::kCoverInfoWords * 4, ix->stream));
  NQ_HIP(ix, nq::launch_cover_init(qidx[0], npk, n, ix->stream));
  *n_picks = npk;
  *n_log = 0;
  *picks = 0;
  uint32_t active = n, round = 0;
  int cur = 0;
  while (active) {
    if (round >= bound) return fail(ix, NIQKI_E_STATE, "niqki_cover: more rounds than a cover can have picks (a bug)");
    round += 1;
    if ((rc = ensure_keep(ix, ix->ws_cv_log, (size_t)*n_log * sizeof(nq::CoverPick), (size_t)(*n_log + active) * sizeof(nq::CoverPick)))) return rc;
    Planes pl;
    HitOut out;
    if ((rc = counter_planes(ix, active, stride, pl))) return rc;
    if ((rc = hit_out_ws(ix, active, active, out))) return rc;   // (top_k = 1: at most one hit a row)
    out.check = false;
    NQ_HIP(ix, hipMemsetAsync(info, 0, 8, ix->stream));   // kCoverInfoActive, kCoverInfoPicks
    if ((rc = ev.mark(0))) return rc;
    if ((rc = query_hits_dev(ix, sk[cur], active, pl, stride, out))) return rc;
    if ((rc = ev.mark(1))) return rc;
    nq::CoverPickArgs a;
    a.hit_off = out.off;
    a.hit_counts = out.counts;
    a.hit_gids = out.gids;
    a.qidx = qidx[cur];
    a.orig = d_orig;
    a.masked = sk[cur];
    a.store = ix->store;
    a.cap = ix->cap;
    a.n_genomes = N;
    a.F = F;
    a.R = ix->d.R;
    a.max_picks = max_picks;
    a.n_picks = npk;
    a.flag = flag;
    a.log = (nq::CoverPick *)ix->ws_cv_log.p + *n_log;
    a.info = info;
    NQ_HIP(ix, nq::launch_cover_pick(a, active, ix->stream));
    if ((rc = ev.mark(2))) return rc;
    NQ_HIP(ix, nq::launch_cover_compact_scan(flag, active, pos, info, ix->stream));
    if ((rc = ev.mark(3))) return rc;
    uint32_t h[nq::kCoverInfoWords] = {0, 0, 0, 0};
    NQ_HIP(ix, hipMemcpyAsync(h, info, sizeof(h), hipMemcpyDeviceToHost, ix->stream));
    NQ_HIP(ix, hipStreamSynchronize(ix->stream));   // the round's one synchronisation
    if ((rc = ev.add(0, 1, 0)) || (rc = ev.add(1, 2, 1)) || (rc = ev.add(2, 3, 2))) return rc;
    *n_log += active;
    *picks += h[nq::kCoverInfoPicks];
    ix->cover_stats.rounds = std::max<uint64_t>(ix->cover_stats.rounds, round);
    ix->cover_stats.picks += h[nq::kCoverInfoPicks];
    ix->cover_stats.mismatches += h[nq::kCoverInfoMismatch];
    if (h[nq::kCoverInfoMismatch]) NQ_HIP(ix, hipMemsetAsync(info + nq::kCoverInfoMismatch, 0, 4, ix->stream));
    if (h[nq::kCoverInfoStuck]) return fail(ix, NIQKI_E_STATE, "niqki_cover: a pick explained no slot of its query (a bug)");
    const uint32_t next = h[nq::kCoverInfoActive];
    if (next > active || h[nq::kCoverInfoPicks] > active) return fail(ix, NIQKI_E_STATE, "niqki_cover: more active queries than the round had (a bug)");
    if (next && next < active) {   // (all rows go on: they are where they belong)
      if ((rc = ev.mark(4))) return rc;
      NQ_HIP(ix, nq::launch_cover_compact(flag, pos, sk[cur], qidx[cur], sk[cur ^ 1], qidx[cur ^ 1], F, active, ix->stream));
      if ((rc = ev.mark(5)) || (rc = ev.add(4, 5, 2))) return rc;
      cur ^= 1;
    }
    active = next;
  }
  return NIQKI_OK;
}

// the greedy cover of the nq whole sketches of src (niqki_hip.h); the outputs in host or device memory
int cover_run(niqki_index *ix, const SketchSource &src, uint32_t nq, uint32_t max_picks, uint64_t *hit_off, uint32_t *hit_counts,
              uint32_t *hit_gids, uint32_t *hit_totals, uint64_t capacity, int mem) {
  ix->cover_stats = CoverStats();
  if (ix->resident_bytes) return fail(ix, NIQKI_E_STATE, "niqki_cover: not on a paged index (resident_bytes): its sketch store is host memory");
  if (!whole_range(ix)) return fail(ix, NIQKI_E_STATE, "niqki_cover: a slot-range shard sees partial counts; the cover needs a whole-range handle");
  const bool dev = mem == NIQKI_MEM_DEVICE;
  int rc = build_if_needed(ix);
  if (rc) return rc;
  const uint32_t N = ix->n_genomes, F = ix->d.F;
  if (nq == 0 || N == 0) {
    if (dev) NQ_HIP(ix, hipMemsetAsync(hit_off, 0, (size_t)(nq + 1) * 8, ix->stream));
    else std::fill(hit_off, hit_off + nq + 1, (uint64_t)0);
    return NIQKI_OK;
  }
  // the query path at the handle's threshold raised to at least 1 and top_k = 1
  CallParams guard(ix, std::max(ix->d.min_score, 1u), 1);
  uint32_t bound = std::min(N, F / ix->d.min_score);
  if (max_picks) bound = std::min(bound, max_picks);
  bound += 1;
  // events of a batch: 0-1 hits, 1-2 pick, 2-3 compact scan, 4-5 compact, 6-7 finish
  PhaseTimer ev(ix, 8, ix->cover_stats.ms);
  if ((rc = ev.create())) return rc;
  const uint32_t qb = dev ? nq : std::max<uint32_t>(ix->query_batch, 1);
  std::vector<uint32_t> hc, hg, ht;
  std::vector<unsigned long long> off;
  uint64_t base = 0;
  for (uint32_t q0 = 0; q0 < nq; q0 += qb) {
    const uint32_t n = std::min(qb, nq - q0);
    const int32_t *d_orig = nullptr;
    if ((rc = src(q0, n, &d_orig))) return rc;
    uint64_t n_log = 0, picks = 0;
    const uint32_t *npk = nullptr;
    if ((rc = cover_rounds(ix, d_orig, n, max_picks, bound, ev, &n_log, &picks, &npk))) return rc;
    const nq::CoverPick *log = (const nq::CoverPick *)ix->ws_cv_log.p;
    if ((rc = ev.mark(6))) return rc;
    if (dev) {   // one batch: straight into the caller's arrays, where they hold the picks
      NQ_HIP(ix, nq::launch_cover_finish(npk, n, (unsigned long long *)hit_off, ix->stream));
      if (picks > capacity) return NIQKI_E_CAPACITY;
      NQ_HIP(ix, nq::launch_cover_scatter(log, n_log, (const unsigned long long *)hit_off, hit_counts, hit_gids, hit_totals, capacity, ix->stream));
      if ((rc = ev.mark(7)) || (rc = ev.add(6, 7, 3))) return rc;
      return NIQKI_OK;
    }
    // host arrays: the batch's lists through ws_cv_out; nothing reaches the caller's arrays before the total is known
    const size_t off_bytes = ((size_t)n + 2) / 2 * 2 * 8;
    if ((rc = ensure(ix, ix->ws_cv_out, off_bytes + (size_t)std::max<uint64_t>(picks, 1) * 12))) return rc;
    unsigned long long *d_off = (unsigned long long *)ix->ws_cv_out.p;
    uint32_t *d_hc = (uint32_t *)((char *)ix->ws_cv_out.p + off_bytes), *d_hg = d_hc + picks, *d_ht = d_hg + picks;
    NQ_HIP(ix, nq::launch_cover_finish(npk, n, d_off, ix->stream));
    NQ_HIP(ix, nq::launch_cover_scatter(log, n_log, d_off, d_hc, d_hg, d_ht, picks, ix->stream));
    if ((rc = ev.mark(7))) return rc;
    off.resize((size_t)n + 1);
    hc.resize(base + picks);
    hg.resize(base + picks);
    ht.resize(base + picks);
    NQ_HIP(ix, hipMemcpyAsync(off.data(), d_off, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost, ix->stream));
    if (picks) {
      NQ_HIP(ix, hipMemcpyAsync(hc.data() + base, d_hc, (size_t)picks * 4, hipMemcpyDeviceToHost, ix->stream));
      NQ_HIP(ix, hipMemcpyAsync(hg.data() + base, d_hg, (size_t)picks * 4, hipMemcpyDeviceToHost, ix->stream));
      NQ_HIP(ix, hipMemcpyAsync(ht.data() + base, d_ht, (size_t)picks * 4, hipMemcpyDeviceToHost, ix->stream));
    }
    NQ_HIP(ix, hipStreamSynchronize(ix->stream));
    if ((rc = ev.add(6, 7, 3))) return rc;
    if (off[n] != picks) return fail(ix, NIQKI_E_STATE, "niqki_cover: the pick log and the per-query counts disagree (a bug)");
    for (uint32_t i = 0; i <= n; ++i) hit_off[q0 + i] = base + off[i];
    base += picks;
  }
  if (base > capacity) return NIQKI_E_CAPACITY;
  std::copy(hc.begin(), hc.end(), hit_counts);
  std::copy(hg.begin(), hg.end(), hit_gids);
  if (hit_totals) std::copy(ht.begin(), ht.end(), hit_totals);
  return NIQKI_OK;
}

}  // namespace

}  // namespace nqi

using namespace nqi;

extern "C" {

int niqki_cover(niqki_index *ix, const int32_t *sketches, uint32_t nq, uint32_t max_picks, uint64_t *hit_off, uint32_t *hit_counts,
                uint32_t *hit_gids, uint32_t *hit_totals, uint64_t capacity, int mem) {
  if (!ix || !hit_off || (!sketches && nq) || (capacity && (!hit_counts || !hit_gids))) return NIQKI_E_INVALID;
  NQ_HIP(ix, hipSetDevice(ix->device));
  return cover_run(ix, mem == NIQKI_MEM_DEVICE ? device_rows(ix, sketches) : host_rows(ix, sketches), nq, max_picks, hit_off, hit_counts, hit_gids,
                   hit_totals, capacity, mem);
}

int niqki_staged_cover(niqki_index *ix, uint32_t max_picks, uint64_t *hit_off, uint32_t *hit_counts, uint32_t *hit_gids,
                       uint32_t *hit_totals, uint64_t capacity, int mem) {
  if (!ix || !hit_off || (capacity && (!hit_counts || !hit_gids))) return NIQKI_E_INVALID;
  NQ_HIP(ix, hipSetDevice(ix->device));
  int rc = staged_sketch_ws(ix);
  if (rc) return rc;
  // (the staged sketches are only read: the rounds work on copies, so niqki_staged_query answers as before)
  return cover_run(ix, device_rows(ix, (const int32_t *)ix->ws_stsk.p), ix->staged.n_entry, max_picks, hit_off, hit_counts, hit_gids, hit_totals,
                   capacity, mem);
}

}  // extern "C"
