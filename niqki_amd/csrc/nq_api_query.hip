// nq_api_query.hip -- Index::query_sketch / query_range behind the C ABI (src/niqki_index.cpp:570-687): counter
// launches (resident, delta segment, paged walks), threshold + order (counter rows or hit lists), host staging,
// the matrix path, and the counter / candidate calls of niqki_hip_bench.h.
#include "nq_handle.h"

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

namespace nqi {

// ---- paged index ---------------------------------------------------------------------------
// slots per page so that a page's sketch-store rows and its inverted index stay within the budget
uint32_t page_slots(const niqki_index *ix) {
  const uint64_t N = std::max<uint64_t>(ix->n_genomes, 1), R = ix->d.R;
  const uint64_t nt = (N + nq::kPadMaxTile - 1) / nq::kPadMaxTile;
  const uint64_t per_slot = (N + 63) / 64 * 64 * 2      // store row
                            + R * nt * sizeof(nq::Entry)  // table row
                            + (N + R * nt * 32) * 2;      // id lists with their alignment padding (estimate)
  uint64_t f = ix->resident_bytes / per_slot / 32 * 32;
  const uint32_t f_all = ix->full_end - ix->full_begin;
  if (f < 32) f = 32;
  return (uint32_t)std::min<uint64_t>({f, (uint64_t)f_all, (uint64_t)nq::kPassSlots});
}

// Makes slots [s0, s1) (relative to the handle's first slot) the resident page: store rows from host
// memory, then the normal index build on them.
int load_page(niqki_index *ix, uint32_t s0, uint32_t s1) {
  if (ix->page_begin == s0 && ix->page_end == s1 && ix->page_n == ix->n_genomes && ix->built) return NIQKI_OK;
  const uint32_t N = ix->n_genomes;
  const uint64_t cap = ((uint64_t)N + 63) / 64 * 64;
  int rc = ensure(ix, ix->pg_store, std::max<size_t>((size_t)(s1 - s0) * cap * 2, 4));
  if (rc) return rc;
  if (N)
    NQ_HIP(ix, hipMemcpy2DAsync(ix->pg_store.p, cap * 2, ix->host_store + (size_t)s0 * ix->host_cap, ix->host_cap * 2,
                                (size_t)N * 2, s1 - s0, hipMemcpyHostToDevice, ix->stream));
  ix->d.slot_begin = ix->full_begin + s0;
  ix->d.slot_end = ix->full_begin + s1;
  ix->store = (uint16_t *)ix->pg_store.p;
  ix->cap = cap;
  ix->page_begin = s0;
  ix->page_end = s1;
  ix->page_n = N;
  ix->built = false;
  return niqki_build(ix);
}

// counts over a paged index: page after page, the gather kernel adding to the rows from the second on
int counts_paged(niqki_index *ix, const int32_t *sketches, uint32_t q_stride, uint32_t q_off, uint32_t nq, uint16_t *counts,
                 uint64_t stride, uint16_t *counts2) {
  const uint32_t f_all = ix->full_end - ix->full_begin, f_page = page_slots(ix);
  if (stride < ix->n_genomes || (stride & 1)) return fail(ix, NIQKI_E_INVALID, "stride must be even and >= genome count");
  if (f_all > nq::kPassSlots && !counts2) return fail(ix, NIQKI_E_INVALID, "S = 16: counts reach 2^16, use niqki_query_counts32 (or the hit calls)");
  ix->built_n = ix->n_genomes;
  if (nq == 0 || ix->n_genomes == 0) return NIQKI_OK;
  // the pages of slots [0, 2^15) add up in `counts`, those of the slots behind (S = 16 only) in `counts2`:
  // either sum stays <= 2^15
  for (uint32_t h0 = 0; h0 < f_all; h0 += nq::kPassSlots) {
    const uint32_t h1 = std::min(f_all, h0 + nq::kPassSlots);
    for (uint32_t s0 = h0; s0 < h1; s0 += f_page) {
      const uint32_t s1 = std::min(h1, s0 + f_page);
      int rc = load_page(ix, s0, s1);
      if (rc) return rc;
      // q_off addresses the handle's first slot in a sketch row; the page starts s0 slots further
      if ((rc = counts_resident(ix, sketches, q_stride, q_off + s0, nq, h0 ? counts2 : counts, stride, s0 != h0))) return rc;
    }
  }
  return NIQKI_OK;
}

// counts for nq device-resident sketches into a device buffer
int counts_dev(niqki_index *ix, const int32_t *sketches, uint32_t q_stride, uint32_t q_off, uint32_t nq,
               uint16_t *counts, uint64_t stride, uint16_t *counts2, const nq::CandOut *co) {
  if (co && co->hl) {   // hit lists (query_hits_dev has checked the index shape)
    if (ix->resident_bytes || two_planes(ix) || co->cand || !counts) return fail(ix, NIQKI_E_INVALID, "hit lists: resident single-plane handles, with counter rows to fall back on");
    return counts_resident(ix, sketches, q_stride, q_off, nq, counts, stride, false, nullptr, co);
  }
  if (co && (ix->resident_bytes || two_planes(ix) || !co->cand || !co->n || !co->cap))
    return fail(ix, NIQKI_E_INVALID, "candidate lists: not on a paged or whole-range S = 16 handle; cand, n_cand and cap > 0 needed");
  if (ix->resident_bytes) return counts_paged(ix, sketches, q_stride, q_off, nq, counts, stride, counts2);
  if (two_planes(ix) && !counts2) return fail(ix, NIQKI_E_INVALID, "S = 16: counts reach 2^16, use niqki_query_counts32 (or the hit calls)");
  if (!counts && !(co && co->surv)) return fail(ix, NIQKI_E_INVALID, "no counter rows: only together with survivor lists");
  if (co && co->surv && (!co->surv_n || !co->surv_cap || co->surv_thr > co->thr))
    return fail(ix, NIQKI_E_INVALID, "survivor lists need surv_n, surv_cap > 0 and surv_thr <= thr");
  if (co && nq) {
    NQ_HIP(ix, hipMemsetAsync(co->n, 0, (size_t)nq * 4, ix->stream));
    NQ_HIP(ix, hipMemsetAsync(co->cand, 0xFF, (size_t)nq * co->cap * 4, ix->stream));
    if (co->surv) NQ_HIP(ix, hipMemsetAsync(co->surv_n, 0, (size_t)nq * 4, ix->stream));
  }
  return counts_resident(ix, sketches, q_stride, q_off, nq, counts, stride, false, counts2, co);
}

// the counter launches of counts_resident over one segment
static int counts_segment(niqki_index *ix, niqki_index::Seg &seg, const int32_t *sketches, uint32_t q_stride, uint32_t q_off, uint32_t nq,
                          uint16_t *counts, uint64_t stride, bool accumulate, uint16_t *counts2, const nq::CandOut *co) {
  int rc;
  nq::IndexView v = view(ix, seg);
  v.q_stride = q_stride;
  v.q_off = q_off;
  v.accumulate = accumulate ? 1u : 0u;
  // what the launches run, how many queries each takes and the scratch they need: the plan (nq_gather_plan.h)
  const bool aligned = (((uintptr_t)(sketches + q_off)) & 15) == 0 && (q_stride & 3) == 0;
  const nq::GatherPlan plan = nq::gather_plan(nq::gather_facts(v), nq::GatherOptions{ix->lookup_prepass, ix->query_order, ix->gather_variant, ix->resident_bytes != 0},
                                              aligned, nq::gather_pad_at_zero(), nq, co && co->hl ? co->hl_cap : 0u);
  const uint32_t chunk = plan.chunk;
  if (plan.stash_bytes && (rc = ensure(ix, ix->ws_stash, plan.stash_bytes))) return rc;
  if (plan.pre_bytes && (rc = ensure(ix, ix->ws_pre, plan.pre_bytes))) return rc;
  if (plan.order_bytes && (rc = ensure(ix, ix->ws_order, plan.order_bytes))) return rc;
  if (plan.packed_table && !seg.ptab_ok) {   // packed copy of the table, once per build
    const size_t want = (size_t)v.f_local * ix->d.R * seg.n_tiles * 4;
    if (want > seg.ptab_bytes) {
      if (seg.ptab) NQ_HIP(ix, hipFree(seg.ptab));
      seg.ptab = nullptr; seg.ptab_bytes = 0;
      NQ_HIP(ix, hipMalloc((void **)&seg.ptab, want));
      seg.ptab_bytes = want;
    }
    NQ_HIP(ix, nq::launch_pack_entries(v, seg.ptab, ix->stream));
    seg.ptab_ok = true;
    v.ptab = seg.ptab;
  }
  ix->last_form = (plan.pre ? 1u : 0u) | (plan.packed_table ? 2u : 0u) | (plan.ordered ? 4u : 0u);
  ix->last_kernel = nq::gather_shape_code(plan.shape);   // what launch_gather launches below
  for (uint32_t q0 = 0; q0 < nq; q0 += chunk) {
    const uint32_t n = std::min(chunk, nq - q0);
    Span sp(ix, NIQKI_KC_GATHER);
    const uint32_t *order = nullptr;
    const nq::OrderForm of = nq::order_form(plan, n);   // fork: probe + order beside the pre-pass (both only read the sketches)
    if (of.fork) {
      if (!ix->aux_stream) {
        if (ix->stream_prio_set) NQ_HIP(ix, hipStreamCreateWithPriority(&ix->aux_stream, hipStreamNonBlocking, ix->stream_prio));
        else NQ_HIP(ix, hipStreamCreateWithFlags(&ix->aux_stream, hipStreamNonBlocking));
        NQ_HIP(ix, hipEventCreateWithFlags(&ix->ev_fork, hipEventDisableTiming));
        NQ_HIP(ix, hipEventCreateWithFlags(&ix->ev_join, hipEventDisableTiming));
      }
      NQ_HIP(ix, hipEventRecord(ix->ev_fork, ix->stream));
      NQ_HIP(ix, hipStreamWaitEvent(ix->aux_stream, ix->ev_fork, 0));
    }
    if (of.ordered) {
      uint32_t *keys = (uint32_t *)ix->ws_order.p;
      NQ_HIP(ix, nq::launch_order(v, sketches + (size_t)q0 * q_stride, n, keys, keys + chunk, of.fork ? ix->aux_stream : ix->stream));
      order = keys + chunk;
      if (of.fork) NQ_HIP(ix, hipEventRecord(ix->ev_join, ix->aux_stream));
    }
    if (plan.pre)
      NQ_HIP(ix, nq::launch_lookup(v, sketches + (size_t)q0 * q_stride, n, (uint32_t *)ix->ws_pre.p, nq::lookup_form(plan, n), ix->stream));
    if (of.fork) NQ_HIP(ix, hipStreamWaitEvent(ix->stream, ix->ev_join, 0));
    nq::CandOut c;
    if (co) {
      c = *co;
      if (co->cand) { c.cand += (size_t)q0 * co->cap; c.n += q0; }
      if (co->surv) { c.surv += (size_t)q0 * co->surv_cap; c.surv_n += q0; }
      if (co->hl) { c.hl += (size_t)q0 * co->hl_cap; c.hl_n += q0; }
    }
    NQ_HIP(ix, nq::launch_gather(v, sketches + (size_t)q0 * q_stride, n, counts ? counts + (size_t)q0 * stride : nullptr,
                                 counts2 ? counts2 + (size_t)q0 * stride : nullptr, stride,
                                 plan.pre ? (nq::Entry *)ix->ws_pre.p : (nq::Entry *)ix->ws_stash.p, order, plan.shape,
                                 plan.lds_bytes, ix->stream, c));
  }
  return NIQKI_OK;
}

int counts_resident(niqki_index *ix, const int32_t *sketches, uint32_t q_stride, uint32_t q_off, uint32_t nq,
                    uint16_t *counts, uint64_t stride, bool accumulate, uint16_t *counts2, const nq::CandOut *co) {
  int rc = ix->resident_bytes ? NIQKI_OK : build_if_needed(ix);
  if (rc) return rc;
  if (nq == 0) return NIQKI_OK;
  if (counts && (stride < ix->built_n || (stride & 1))) return fail(ix, NIQKI_E_INVALID, "stride must be even and >= genome count");
  if ((uintptr_t)counts & 3) return fail(ix, NIQKI_E_INVALID, "counts must be 4-byte aligned (rows are written as packed u16 pairs)");
  if (ix->built_n == 0) return NIQKI_OK;
  // the delta segment first (its columns are its own), then the main one: the stats of the last launch are the main segment's
  if (ix->delta.n && !ix->resident_bytes &&
      (rc = counts_segment(ix, ix->delta, sketches, q_stride, q_off, nq, counts, stride, accumulate, counts2, co)))
    return rc;
  return counts_segment(ix, ix->main, sketches, q_stride, q_off, nq, counts, stride, accumulate, counts2, co);
}

int counter_planes(niqki_index *ix, uint32_t n, uint64_t stride, Planes &pl, bool zeroed) {
  const size_t plane = (size_t)n * stride * 2, bytes = std::max<size_t>(plane * (two_planes(ix) ? 2 : 1), 4);
  int rc = ensure(ix, ix->ws_counts, bytes);
  if (rc) return rc;
  pl.c1 = (uint16_t *)ix->ws_counts.p;
  pl.c2 = two_planes(ix) ? (uint16_t *)((char *)ix->ws_counts.p + plane) : nullptr;
  if (zeroed) NQ_HIP(ix, hipMemsetAsync(ix->ws_counts.p, 0, bytes, ix->stream));
  return NIQKI_OK;
}

int hit_out_ws(niqki_index *ix, uint32_t n, uint64_t capacity, HitOut &out) {
  int rc;
  if ((rc = ensure(ix, ix->ws_hitoff, (size_t)(n + 1) * 8))) return rc;
  if ((rc = ensure(ix, ix->ws_hc, (size_t)std::max<uint64_t>(capacity, 1) * 4))) return rc;
  if ((rc = ensure(ix, ix->ws_hg, (size_t)std::max<uint64_t>(capacity, 1) * 4))) return rc;
  out = HitOut{(unsigned long long *)ix->ws_hitoff.p, (uint32_t *)ix->ws_hc.p, (uint32_t *)ix->ws_hg.p, capacity, true};
  return NIQKI_OK;
}

int hits_to_host(niqki_index *ix, int rc, const HitOut &out, uint32_t n, void *hit_off, uint32_t *hit_counts, uint32_t *hit_gids) {
  if (rc && rc != NIQKI_E_CAPACITY) return rc;
  NQ_HIP(ix, hipMemcpyAsync(hit_off, out.off, (size_t)(n + 1) * 8, hipMemcpyDeviceToHost, ix->stream));
  if (rc == NIQKI_OK && out.total) {
    NQ_HIP(ix, hipMemcpyAsync(hit_counts, out.counts, (size_t)out.total * 4, hipMemcpyDeviceToHost, ix->stream));
    NQ_HIP(ix, hipMemcpyAsync(hit_gids, out.gids, (size_t)out.total * 4, hipMemcpyDeviceToHost, ix->stream));
  }
  NQ_HIP(ix, hipStreamSynchronize(ix->stream));
  return rc;
}

// What the two forms of the hit step share: the rows, the output, the top-k clamp and the scratch the hits are ordered
// in (ws_tc / ws_tg).  The block scratch (ws_blk) is each form's own.
static int hits_args(niqki_index *ix, const uint16_t *counts, const uint16_t *counts2, uint32_t nq, uint64_t stride, uint32_t gid_begin,
                     uint32_t n_gids, const HitOut &out, nq::HitsArgs &a) {
  a = nq::HitsArgs{};
  a.counts = counts;
  a.counts2 = counts2;
  a.stride = stride;
  a.nq = nq;
  a.gid_begin = gid_begin;
  a.n_gids = n_gids;
  a.min_score = ix->d.min_score;
  a.n_blk = (n_gids + nq::kHitsBlk - 1) / nq::kHitsBlk;
  a.hit_off = out.off;
  a.hit_counts = out.counts;
  a.hit_gids = out.gids;
  a.capacity = out.capacity;
  // top-k (k < n_gids: k >= n_gids cuts nothing): the output holds <= nq x k entries
  a.top_k = ix->p.top_k < n_gids ? ix->p.top_k : 0u;
  const uint64_t room = a.top_k ? std::min<uint64_t>(out.capacity, (uint64_t)nq * a.top_k) : out.capacity;
  int rc;
  if ((rc = ensure(ix, ix->ws_tc, (size_t)std::max<uint64_t>(room, 1) * 4))) return rc;
  if ((rc = ensure(ix, ix->ws_tg, (size_t)std::max<uint64_t>(room, 1) * 4))) return rc;
  a.tmp_counts = (uint32_t *)ix->ws_tc.p;
  a.tmp_gids = (uint32_t *)ix->ws_tg.p;
  return NIQKI_OK;
}

// between a form's count and emit launches, with out.check: the total back, NIQKI_E_CAPACITY where it does not fit
static int check_capacity(niqki_index *ix, uint32_t nq, HitOut &out) {
  if (!out.check) return NIQKI_OK;
  unsigned long long total = 0;
  NQ_HIP(ix, hipMemcpyAsync(&total, out.off + nq, 8, hipMemcpyDeviceToHost, ix->stream));
  NQ_HIP(ix, hipStreamSynchronize(ix->stream));
  out.total = total;
  return total > out.capacity ? NIQKI_E_CAPACITY : NIQKI_OK;
}

// hits from device-resident counters into device buffers; out.off device (nq+1)
int hits_dev(niqki_index *ix, const uint16_t *counts, const uint16_t *counts2, uint32_t nq, uint64_t stride, uint32_t gid_begin,
             uint32_t n_gids, HitOut &out) {
  out.total = 0;
  if (nq == 0 || n_gids == 0) {   // (before any scratch is sized)
    NQ_HIP(ix, hipMemsetAsync(out.off, 0, (size_t)(nq + 1) * 8, ix->stream));
    return NIQKI_OK;
  }
  nq::HitsArgs a;
  int rc = hits_args(ix, counts, counts2, nq, stride, gid_begin, n_gids, out, a);
  if (rc) return rc;
  // with top-k the select replaces the hit count
  const size_t nb = (size_t)nq * a.n_blk;
  if ((rc = ensure(ix, ix->ws_blk, (a.top_k ? nb * (2 + nq::kSelBlkWords) + nq : nb) * 4))) return rc;
  a.blk_counts = (uint32_t *)ix->ws_blk.p;
  if (a.top_k) {
    a.blk_skip = a.blk_counts + nb;
    a.blk_tmp = a.blk_skip + nb;
    a.thr = a.blk_tmp + nb * nq::kSelBlkWords;
  }
  Span sp(ix, NIQKI_KC_HITS);
  NQ_HIP(ix, nq::launch_hits_count(a, ix->stream));
  if ((rc = check_capacity(ix, nq, out))) return rc;
  NQ_HIP(ix, nq::launch_hits_emit(a, ix->stream));
  return NIQKI_OK;
}

// the list capacity of the hit-list form: hit_list_cap rounded up to whole 16-byte pieces
static uint32_t hit_list_cap(const niqki_index *ix) {
  return std::min<uint32_t>((std::max<uint32_t>(ix->hit_list_cap, 1) + 3u) & ~3u, nq::kHitListMaxCap);
}

// the built index takes the hit-list form of query_hits_dev (one segment, resident, one plane, counts < 2^16, the
// gather kernel's counters + queues + list within a workgroup's LDS).  An index of at most kHitListMaxTile genomes is
// one tile unless option tile_genomes splits it; such a split index keeps counter rows, as it did before the form took
// several tiles.  There is no speed or correctness reason for that: it keeps the behaviour the top-k tile tests pin
// (tests/test_gpu_topk.py, form "tiles": counter rows on 3 000 genomes in tiles of 512).
// At min_score 0 every genome is a hit and every query of an index larger than kHitListMaxTile (beyond the cap) falls
// back to its row with N hits: there counter rows are faster (100 000 genomes: 7.8 ms against 23.0 in the emit's wave
// radix passes, tools/bench_hitlists_overflow.py), and such an index keeps them.
static bool hit_lists_apply(const niqki_index *ix) {
  const uint32_t N = ix->built_n;
  return ix->hit_lists && N && !ix->resident_bytes && !two_planes(ix) && ix->delta.n == 0 &&
         (ix->d.min_score > 0 || N <= nq::kHitListMaxTile) &&
         (ix->main.n_tiles == 1 || N > nq::kHitListMaxTile) && nq::hit_list_lds(ix->main.tile, hit_list_cap(ix)) <= nq::kGatherMaxLds;
}

// Index::query_sketch (src/niqki_index.cpp:633-687) for nq device-resident whole sketches into device buffers: counters,
// threshold, order.  pl: counter planes of nq rows (counter_planes).  On a single-segment, single-plane index
// (hit_lists_apply) the hits leave the gather kernel as ordered lists and no counter row is written or read again,
// except for a query with more than hit_list_cap hits.
int query_hits_dev(niqki_index *ix, const int32_t *sketches, uint32_t nq, const Planes &pl, uint64_t stride, HitOut &out) {
  int rc = build_if_needed(ix);
  if (rc) return rc;
  const uint32_t N = ix->built_n;
  const bool lists = nq && hit_lists_apply(ix);
  ix->last_hits_form = lists ? 1u : 0u;
  if (!lists) {
    if ((rc = counts_dev(ix, sketches, ix->d.F, first_slot(ix), nq, pl.c1, stride, pl.c2))) return rc;
    return hits_dev(ix, pl.c1, pl.c2, nq, stride, 0, N, out);
  }
  out.total = 0;
  const uint32_t cap = hit_list_cap(ix);
  nq::HitsArgs a;   // (top-k: a query's segment is the first min(n, k) of its list; ws_tc / ws_tg: lists of > 2048 hits)
  if ((rc = hits_args(ix, pl.c1, nullptr, nq, stride, 0, N, out, a))) return rc;
  if ((rc = ensure(ix, ix->ws_hl, (size_t)nq * cap * 8))) return rc;
  if ((rc = ensure(ix, ix->ws_blk, ((size_t)nq * 2 + 1) * 4))) return rc;   // the lists' sizes, then the overflowing queries
  nq::CandOut co;
  co.hl = (unsigned long long *)ix->ws_hl.p;
  co.hl_n = (uint32_t *)ix->ws_blk.p;
  co.hl_over = co.hl_n + nq;
  co.hl_cap = cap;
  co.hl_min = ix->d.min_score;
  if ((rc = counts_dev(ix, sketches, ix->d.F, first_slot(ix), nq, pl.c1, stride, nullptr, &co))) return rc;
  Span sp(ix, NIQKI_KC_HITS);
  NQ_HIP(ix, nq::launch_hitlist_scan(co.hl_n, a, cap, co.hl_over, ix->stream));
  if ((rc = check_capacity(ix, nq, out))) return rc;
  NQ_HIP(ix, nq::launch_hitlist_emit(a, co.hl_n, co.hl, cap, co.hl_over, ix->stream));
  return NIQKI_OK;
}

SketchSource host_rows(niqki_index *ix, const int32_t *sketches) {
  return [=](uint32_t q0, uint32_t n, const int32_t **d_sk) {
    const size_t bytes = (size_t)n * ix->d.F * 4;
    int rc = ensure(ix, ix->ws_sk, bytes);
    if (rc) return rc;
    NQ_HIP(ix, hipMemcpyAsync(ix->ws_sk.p, sketches + (size_t)q0 * ix->d.F, bytes, hipMemcpyHostToDevice, ix->stream));
    *d_sk = (const int32_t *)ix->ws_sk.p;
    return (int)NIQKI_OK;
  };
}

SketchSource device_rows(niqki_index *ix, const int32_t *sketches) {
  return [=](uint32_t q0, uint32_t, const int32_t **d_sk) {
    *d_sk = sketches + (size_t)q0 * ix->d.F;
    return (int)NIQKI_OK;
  };
}

SketchSource stored_rows(niqki_index *ix, uint32_t begin) {
  return [=](uint32_t q0, uint32_t n, const int32_t **d_sk) {
    int rc = ensure(ix, ix->ws_misc, (size_t)n * ix->d.F * 4);
    if (rc) return rc;
    *d_sk = (const int32_t *)ix->ws_misc.p;
    return stored_sketch_rows(ix, begin + q0, n, (int32_t *)ix->ws_misc.p);
  };
}

// queries per round of launches: option "query_batch" bounds the counter rows (2N bytes per query); a small index
// (<= 12 288 genomes) that takes the hit-list form writes rows only for the rare overflowing query, so a whole staged
// batch of short reads goes through in one round (64 rounds of 1024 cost the lines-mode host path twice its kernels'
// time)
uint32_t query_rows_per_batch(const niqki_index *ix) {
  return hit_lists_apply(ix) && ix->built_n <= nq::kHitListMaxTile ? std::max<uint32_t>(ix->query_batch, 65536u) : ix->query_batch;
}

// Every hit_off entry is a true total, whatever the capacity; nothing is written beyond it, and NIQKI_E_CAPACITY comes
// at the end.
int query_to_host(niqki_index *ix, const SketchSource &src, uint32_t nq, uint32_t qb, uint64_t *hit_off, uint32_t *hit_counts,
                  uint32_t *hit_gids, uint64_t capacity) {
  int rc;
  const uint64_t stride = NIQKI_ROW_STRIDE(ix->built_n);
  uint64_t base = 0;
  bool overflow = false;
  hit_off[0] = 0;
  std::vector<unsigned long long> off(std::min(qb, nq) + 1);
  for (uint32_t q0 = 0; q0 < nq; q0 += qb) {
    const uint32_t n = std::min(qb, nq - q0);
    const int32_t *d_sk = nullptr;
    Planes pl;
    HitOut out;
    if ((rc = src(q0, n, &d_sk))) return rc;
    if ((rc = counter_planes(ix, n, stride, pl))) return rc;
    if ((rc = hit_out_ws(ix, n, overflow || base > capacity ? 0 : capacity - base, out))) return rc;
    rc = query_hits_dev(ix, d_sk, n, pl, stride, out);
    rc = hits_to_host(ix, rc, out, n, off.data(), hit_counts + base, hit_gids + base);
    if (rc == NIQKI_E_CAPACITY) overflow = true;
    else if (rc) return rc;
    for (uint32_t i = 0; i < n; ++i) hit_off[q0 + i + 1] = base + off[i + 1];
    base += off[n];
  }
  return overflow ? NIQKI_E_CAPACITY : NIQKI_OK;
}

}  // namespace nqi

using namespace nqi;

extern "C" {

int niqki_query_counts(niqki_index *ix, const int32_t *sketches, uint32_t nq, uint16_t *counts,
                       uint64_t stride, int mem) {
  if (!ix || (!sketches && nq) || (!counts && nq)) return NIQKI_E_INVALID;
  NQ_HIP(ix, hipSetDevice(ix->device));
  if (mem == NIQKI_MEM_DEVICE) return counts_dev(ix, sketches, ix->d.F, first_slot(ix), nq, counts, stride);
  if (stride < ix->n_genomes || (stride & 1)) return fail(ix, NIQKI_E_INVALID, "stride must be even and >= genome count");
  const uint32_t qb = ix->query_batch;
  for (uint32_t q0 = 0; q0 < nq; q0 += qb) {
    const uint32_t n = std::min(qb, nq - q0);
    int rc;
    if ((rc = ensure(ix, ix->ws_sk, (size_t)n * ix->d.F * 4))) return rc;
    if ((rc = ensure(ix, ix->ws_counts, (size_t)n * stride * 2))) return rc;
    NQ_HIP(ix, hipMemcpyAsync(ix->ws_sk.p, sketches + (size_t)q0 * ix->d.F, (size_t)n * ix->d.F * 4, hipMemcpyHostToDevice, ix->stream));
    NQ_HIP(ix, hipMemsetAsync(ix->ws_counts.p, 0, (size_t)n * stride * 2, ix->stream));
    if ((rc = counts_dev(ix, (const int32_t *)ix->ws_sk.p, ix->d.F, first_slot(ix), n, (uint16_t *)ix->ws_counts.p, stride))) return rc;
    NQ_HIP(ix, hipMemcpyAsync(counts + (size_t)q0 * stride, ix->ws_counts.p, (size_t)n * stride * 2, hipMemcpyDeviceToHost, ix->stream));
    NQ_HIP(ix, hipStreamSynchronize(ix->stream));
  }
  return NIQKI_OK;
}

int niqki_query_counts32(niqki_index *ix, const int32_t *sketches, uint32_t nq, uint32_t *counts, uint64_t stride, int mem) {
  if (!ix || (!sketches && nq) || (!counts && nq)) return NIQKI_E_INVALID;
  NQ_HIP(ix, hipSetDevice(ix->device));
  int rc = build_if_needed(ix);
  if (rc) return rc;
  if (stride < ix->n_genomes || (stride & 1)) return fail(ix, NIQKI_E_INVALID, "stride must be even and >= genome count");
  const uint32_t qb = mem == NIQKI_MEM_DEVICE ? std::min<uint32_t>(nq, 4096) : ix->query_batch;
  for (uint32_t q0 = 0; q0 < nq; q0 += qb) {
    const uint32_t n = std::min(qb, nq - q0);
    Planes pl;
    if ((rc = counter_planes(ix, n, stride, pl, true))) return rc;
    const int32_t *d_sk = sketches + (size_t)q0 * ix->d.F;
    uint32_t *d_out = counts + (size_t)q0 * stride;
    if (mem == NIQKI_MEM_HOST) {
      if ((rc = ensure(ix, ix->ws_sk, (size_t)n * ix->d.F * 4))) return rc;
      if ((rc = ensure(ix, ix->ws_misc, (size_t)n * stride * 4))) return rc;
      NQ_HIP(ix, hipMemcpyAsync(ix->ws_sk.p, d_sk, (size_t)n * ix->d.F * 4, hipMemcpyHostToDevice, ix->stream));
      d_sk = (const int32_t *)ix->ws_sk.p;
      d_out = (uint32_t *)ix->ws_misc.p;
    }
    if ((rc = counts_dev(ix, d_sk, ix->d.F, first_slot(ix), n, pl.c1, stride, pl.c2))) return rc;
    NQ_HIP(ix, nq::launch_plane_sum32(pl.c1, pl.c2, d_out, (uint64_t)n * stride, ix->stream));
    if (mem == NIQKI_MEM_HOST) {
      NQ_HIP(ix, hipMemcpyAsync(counts + (size_t)q0 * stride, d_out, (size_t)n * stride * 4, hipMemcpyDeviceToHost, ix->stream));
      NQ_HIP(ix, hipStreamSynchronize(ix->stream));
    }
  }
  return NIQKI_OK;
}

int niqki_hits_from_counts(niqki_index *ix, const uint16_t *counts, uint32_t nq, uint64_t stride,
                           uint32_t gid_begin, uint32_t n_gids, uint64_t *hit_off, uint32_t *hit_counts,
                           uint32_t *hit_gids, uint64_t capacity, int mem) {
  if (!ix || !hit_off || (!counts && nq)) return NIQKI_E_INVALID;
  if ((uint64_t)gid_begin + n_gids > stride) return fail(ix, NIQKI_E_INVALID, "gid range exceeds stride");
  if (ix->d.S > 15) return fail(ix, NIQKI_E_INVALID, "S = 16: u16 counters cannot hold a count of 2^16; use niqki_query");
  NQ_HIP(ix, hipSetDevice(ix->device));
  HitOut out{(unsigned long long *)hit_off, hit_counts, hit_gids, capacity};
  if (mem == NIQKI_MEM_DEVICE) return hits_dev(ix, counts, nullptr, nq, stride, gid_begin, n_gids, out);
  int rc;
  if ((rc = ensure(ix, ix->ws_counts, std::max<size_t>((size_t)nq * stride * 2, 2)))) return rc;   // (one plane: S <= 15)
  if ((rc = hit_out_ws(ix, nq, capacity, out))) return rc;
  if (nq) NQ_HIP(ix, hipMemcpyAsync(ix->ws_counts.p, counts, (size_t)nq * stride * 2, hipMemcpyHostToDevice, ix->stream));
  rc = hits_dev(ix, (const uint16_t *)ix->ws_counts.p, nullptr, nq, stride, gid_begin, n_gids, out);
  return hits_to_host(ix, rc, out, nq, hit_off, hit_counts, hit_gids);
}

int niqki_candidates_from_counts(niqki_index *ix, const uint16_t *counts, uint32_t nq, uint64_t stride,
                                 uint32_t n_gids, uint32_t threshold, uint32_t cap, int32_t *cand, int32_t *n_cand,
                                 int mem) {
  if (!ix || (nq && (!counts || !cand || !n_cand)) || n_gids > stride || cap == 0) return NIQKI_E_INVALID;
  if (mem != NIQKI_MEM_DEVICE) return fail(ix, NIQKI_E_INVALID, "niqki_candidates_from_counts is device-memory only");
  NQ_HIP(ix, hipSetDevice(ix->device));
  Span sp(ix, NIQKI_KC_HITS);
  NQ_HIP(ix, nq::launch_candidates(counts, stride, nq, n_gids, threshold, cap, cand, n_cand, ix->stream));
  return NIQKI_OK;
}

int niqki_query_counts_candidates(niqki_index *ix, const int32_t *sketches, uint32_t nq, uint16_t *counts, uint64_t stride,
                                  uint32_t threshold, uint32_t cap, int32_t *cand, int32_t *n_cand, int mem) {
  if (!ix || (nq && (!sketches || !counts || !cand || !n_cand)) || cap == 0) return NIQKI_E_INVALID;
  if (mem != NIQKI_MEM_DEVICE) return fail(ix, NIQKI_E_INVALID, "niqki_query_counts_candidates is device-memory only");
  NQ_HIP(ix, hipSetDevice(ix->device));
  nq::CandOut co;
  co.cand = cand;
  co.n = n_cand;
  co.thr = threshold;
  co.cap = cap;
  return counts_dev(ix, sketches, ix->d.F, first_slot(ix), nq, counts, stride, nullptr, &co);
}

int niqki_query(niqki_index *ix, const int32_t *sketches, uint32_t nq, uint64_t *hit_off,
                uint32_t *hit_counts, uint32_t *hit_gids, uint64_t capacity, int mem) {
  if (!ix || !hit_off || (!sketches && nq)) return NIQKI_E_INVALID;
  NQ_HIP(ix, hipSetDevice(ix->device));
  int rc = build_if_needed(ix);
  if (rc) return rc;
  const uint32_t N = ix->built_n;
  const uint64_t stride = NIQKI_ROW_STRIDE(N);
  if (mem == NIQKI_MEM_DEVICE) {
    Planes pl;
    HitOut out{(unsigned long long *)hit_off, hit_counts, hit_gids, capacity};
    if ((rc = counter_planes(ix, nq, stride, pl))) return rc;
    return query_hits_dev(ix, sketches, nq, pl, stride, out);
  }
  return query_to_host(ix, host_rows(ix, sketches), nq, query_rows_per_batch(ix), hit_off, hit_counts, hit_gids, capacity);
}

int niqki_query_sequences(niqki_index *ix, const uint8_t *seqs, const uint64_t *rec_off, uint32_t n_rec,
                          const uint32_t *entry_rec, uint32_t n_entry, uint64_t *hit_off,
                          uint32_t *hit_counts, uint32_t *hit_gids, uint64_t capacity, int mem) {
  if (!ix) return NIQKI_E_INVALID;
  NQ_HIP(ix, hipSetDevice(ix->device));
  if (mem == NIQKI_MEM_DEVICE) {
    int rc = ensure(ix, ix->ws_sk, std::max<size_t>((size_t)n_entry * ix->d.F * 4, 4));
    if (rc) return rc;
    if ((rc = niqki_sketch(ix, seqs, rec_off, n_rec, entry_rec, n_entry, (int32_t *)ix->ws_sk.p, NIQKI_MEM_DEVICE))) return rc;
    return niqki_query(ix, (const int32_t *)ix->ws_sk.p, n_entry, hit_off, hit_counts, hit_gids, capacity, NIQKI_MEM_DEVICE);
  }
  std::vector<int32_t> sk((size_t)n_entry * ix->d.F);
  int rc = niqki_sketch(ix, seqs, rec_off, n_rec, entry_rec, n_entry, sk.data(), NIQKI_MEM_HOST);
  if (rc) return rc;
  return niqki_query(ix, sk.data(), n_entry, hit_off, hit_counts, hit_gids, capacity, NIQKI_MEM_HOST);
}

// ---- sketches made ahead: batch i + 1 is sketched beside batch i's gather and hit kernels -------------------------
// The sketch kernel is bound by vector instruction issue, the gather launch by random HBM lines; a step of the query
// path is the one after the other (18.9 + 7.3 ms per 4096 genomes).  With the coming batch's sketch kernel on a lane of
// its own the two overlap where either leaves CUs idle (the tails of both launches): + 5 % genomes/s.
int niqki_sketch_ahead(niqki_index *ix, const uint8_t *seqs, const uint64_t *rec_off, uint32_t n_rec, const uint32_t *entry_rec,
                       uint32_t n_entry, int mem) {
  if (!ix || (!seqs && n_rec) || !rec_off) return NIQKI_E_INVALID;
  if (mem != NIQKI_MEM_DEVICE) return fail(ix, NIQKI_E_INVALID, "niqki_sketch_ahead is device-memory only (host records: niqki_query_sequences)");
  if (!entry_rec && n_entry != n_rec) return fail(ix, NIQKI_E_INVALID, "n_entry must equal n_rec without entry_rec");
  if (ix->ahead_n >= 2) return fail(ix, NIQKI_E_STATE, "two batches are sketched ahead already: niqki_query_ahead takes the older one");
  NQ_HIP(ix, hipSetDevice(ix->device));
  if (!ix->sk_stream) {
    // the sketch lane never outranks the handle's stream: what a query is waiting for runs there
    int cus = 0;
    NQ_HIP(ix, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ix->device));
    if (ix->sk_lane_cus && (int)ix->sk_lane_cus < cus) {
      std::vector<uint32_t> mask(((size_t)cus + 31) / 32, 0u);
      for (int c = cus - (int)ix->sk_lane_cus; c < cus; ++c) mask[(size_t)c / 32] |= 1u << (c % 32);
      NQ_HIP(ix, hipExtStreamCreateWithCUMask(&ix->sk_stream, (uint32_t)mask.size(), mask.data()));
    } else if (ix->stream_prio_set) {
      int least = 0, greatest = 0;
      NQ_HIP(ix, hipDeviceGetStreamPriorityRange(&least, &greatest));
      NQ_HIP(ix, hipStreamCreateWithPriority(&ix->sk_stream, hipStreamNonBlocking, least));
    } else {
      NQ_HIP(ix, hipStreamCreateWithFlags(&ix->sk_stream, hipStreamNonBlocking));
    }
  }
  auto &a = ix->ahead[(ix->ahead_head + ix->ahead_n) & 1u];
  if (!a.done) {
    NQ_HIP(ix, hipEventCreateWithFlags(&a.done, hipEventDisableTiming));
    NQ_HIP(ix, hipEventCreateWithFlags(&a.used, hipEventDisableTiming));
  }
  const size_t bytes = std::max<size_t>((size_t)n_entry * ix->d.F * 4, 4);
  if (bytes > a.sk.n && a.used_set) NQ_HIP(ix, hipEventSynchronize(a.used));   // (growing the slot frees what its last query read)
  int rc = ensure(ix, a.sk, bytes);
  if (rc) return rc;
  if (a.used_set) NQ_HIP(ix, hipStreamWaitEvent(ix->sk_stream, a.used, 0));
  uint64_t total = ix->record_len_hint * n_entry;
  if (total == 0 && n_entry) {   // only to pick the launch shape: the last offset
    NQ_HIP(ix, hipMemcpyAsync(&total, rec_off + n_rec, 8, hipMemcpyDeviceToHost, ix->sk_stream));
    NQ_HIP(ix, hipStreamSynchronize(ix->sk_stream));
  }
  hipStream_t main = ix->stream;
  ix->stream = ix->sk_stream;      // (sketch_dev and its profiling spans enqueue on the handle's current stream)
  rc = sketch_dev(ix, seqs, rec_off, n_rec, entry_rec, n_entry, (int32_t *)a.sk.p, total);
  ix->stream = main;
  if (rc) return rc;
  NQ_HIP(ix, hipEventRecord(a.done, ix->sk_stream));
  a.n_entry = n_entry;
  ix->ahead_n += 1;
  return NIQKI_OK;
}

int niqki_query_ahead(niqki_index *ix, uint32_t *n_entry, uint64_t *hit_off, uint32_t *hit_counts, uint32_t *hit_gids, uint64_t capacity,
                      int32_t *sketches, int mem) {
  if (!ix || !hit_off) return NIQKI_E_INVALID;
  if (ix->ahead_n == 0) return fail(ix, NIQKI_E_STATE, "no batch sketched ahead (niqki_sketch_ahead first)");
  NQ_HIP(ix, hipSetDevice(ix->device));
  auto &a = ix->ahead[ix->ahead_head];
  if (n_entry) *n_entry = a.n_entry;
  NQ_HIP(ix, hipStreamWaitEvent(ix->stream, a.done, 0));
  int rc;
  if (mem == NIQKI_MEM_DEVICE) {
    rc = niqki_query(ix, (const int32_t *)a.sk.p, a.n_entry, hit_off, hit_counts, hit_gids, capacity, NIQKI_MEM_DEVICE);
  } else {
    if ((rc = build_if_needed(ix))) return rc;
    rc = query_to_host(ix, device_rows(ix, (const int32_t *)a.sk.p), a.n_entry, query_rows_per_batch(ix), hit_off, hit_counts, hit_gids, capacity);
  }
  if (rc == NIQKI_E_CAPACITY) return rc;   // the batch stays the oldest one: the same call again with larger arrays
  if (!rc && sketches && a.n_entry)
    NQ_HIP(ix, hipMemcpyAsync(sketches, a.sk.p, (size_t)a.n_entry * ix->d.F * 4,
                              mem == NIQKI_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, ix->stream));
  NQ_HIP(ix, hipEventRecord(a.used, ix->stream));
  if (!rc && sketches && mem == NIQKI_MEM_HOST) NQ_HIP(ix, hipStreamSynchronize(ix->stream));
  a.used_set = true;
  ix->ahead_head ^= 1u;
  ix->ahead_n -= 1;
  return rc;
}

int niqki_matrix_range(niqki_index *ix, uint32_t begin, uint32_t end, uint16_t *counts, uint64_t stride,
                       int mem) {
  if (!ix || begin > end || end > ix->n_genomes || (!counts && end > begin)) return NIQKI_E_INVALID;
  NQ_HIP(ix, hipSetDevice(ix->device));
  // (a paged index: the counters come from the paged walk)
  int rc = ix->resident_bytes ? NIQKI_OK : build_if_needed(ix);
  if (rc) return rc;
  const uint32_t n_all = ix->resident_bytes ? ix->n_genomes : ix->built_n;
  if (stride < n_all || (stride & 1)) return fail(ix, NIQKI_E_INVALID, "stride must be even and >= genome count");
  // The bucket co-occurrence count of (a, t) equals the hit count of genome a
  // for the stored sketch of t: both count the slots where the two sketches
  // hold the same valid fingerprint.  So the range is answered by the gather
  // kernel on the stored sketches of [begin, end).
  const uint32_t qb = std::min<uint32_t>(ix->query_batch, 256);
  for (uint32_t t0 = begin; t0 < end; t0 += qb) {
    const uint32_t n = std::min(qb, end - t0);
    if ((rc = ensure(ix, ix->ws_misc, (size_t)n * ix->d.F * 4))) return rc;
    if ((rc = stored_sketch_rows(ix, t0, n, (int32_t *)ix->ws_misc.p))) return rc;
    uint16_t *dst = counts + (size_t)(t0 - begin) * stride;
    if (mem == NIQKI_MEM_DEVICE) {
      uint16_t *c2 = nullptr;
      if (two_planes(ix)) {
        if ((rc = ensure(ix, ix->ws_counts, (size_t)n * stride * 2))) return rc;
        c2 = (uint16_t *)ix->ws_counts.p;
      }
      if ((rc = counts_dev(ix, (const int32_t *)ix->ws_misc.p, ix->d.F, first_slot(ix), n, dst, stride, c2))) return rc;
      // uint16 counters whatever S (src/niqki_index.cpp:572): at S = 16 a count of 2^16 reads 0, as in the reference
      if (c2) NQ_HIP(ix, nq::launch_plane_add16(dst, c2, (uint64_t)n * stride, ix->stream));
    } else {
      Planes pl;
      if ((rc = counter_planes(ix, n, stride, pl, true))) return rc;
      if ((rc = counts_dev(ix, (const int32_t *)ix->ws_misc.p, ix->d.F, first_slot(ix), n, pl.c1, stride, pl.c2))) return rc;
      if (pl.c2) NQ_HIP(ix, nq::launch_plane_add16(pl.c1, pl.c2, (uint64_t)n * stride, ix->stream));
      NQ_HIP(ix, hipMemcpyAsync(dst, pl.c1, (size_t)n * stride * 2, hipMemcpyDeviceToHost, ix->stream));
      NQ_HIP(ix, hipStreamSynchronize(ix->stream));
    }
  }
  return NIQKI_OK;
}


int niqki_query_gathered(niqki_index *ix, const int32_t *sketches, uint32_t nq, uint64_t *gathered, int mem) {
  if (!ix || (!sketches && nq) || (!gathered && nq)) return NIQKI_E_INVALID;
  NQ_HIP(ix, hipSetDevice(ix->device));
  if (ix->resident_bytes) return fail(ix, NIQKI_E_STATE, "niqki_query_gathered is not available on a paged index (resident_bytes)");
  int rc = build_single(ix);
  if (rc) return rc;
  if (nq == 0) return NIQKI_OK;
  const int32_t *d_sk = sketches;
  if (mem == NIQKI_MEM_HOST) {
    if ((rc = ensure(ix, ix->ws_sk, (size_t)nq * ix->d.F * 4))) return rc;
    NQ_HIP(ix, hipMemcpyAsync(ix->ws_sk.p, sketches, (size_t)nq * ix->d.F * 4, hipMemcpyHostToDevice, ix->stream));
    d_sk = (const int32_t *)ix->ws_sk.p;
  }
  if ((rc = ensure(ix, ix->ws_misc, (size_t)nq * 8))) return rc;
  NQ_HIP(ix, hipMemsetAsync(ix->ws_misc.p, 0, (size_t)nq * 8, ix->stream));
  if (ix->built_n) NQ_HIP(ix, nq::launch_gathered(view(ix), d_sk, nq, (unsigned long long *)ix->ws_misc.p, ix->stream));
  NQ_HIP(ix, hipMemcpyAsync(gathered, ix->ws_misc.p, (size_t)nq * 8, hipMemcpyDeviceToHost, ix->stream));
  NQ_HIP(ix, hipStreamSynchronize(ix->stream));
  return NIQKI_OK;
}

}  // extern "C"
