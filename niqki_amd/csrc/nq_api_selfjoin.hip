// nq_api_selfjoin.hip -- the self-join of an index behind the C ABI: niqki_neighbors_range (the hits of the stored
// sketches, the sparse form of Index::query_range, src/niqki_index.cpp:570-610), niqki_cluster (single-linkage
// clusters: the link and flatten kernels over the hit lists of the stored sketches) and niqki_dereplicate /
// niqki_dereplicate_from (greedy representatives in index order, the genomes below `first` given: the decide, assign
// and finish kernels over the same hit lists) and niqki_linkage (the single-linkage forest and hierarchy: the forest
// kernels over the same hit lists, then a host pass over fewer than N edges).  The kernels are in nq_cluster.hip, the
// hit lists come from the query path (nq_api_query.hip).  DESIGN.md 4.6b, 4.6c, 4.6f, 4.6g.  The driver of the
// self-join (SelfJoin, self_join_batches: nq_handle.h) also serves niqki_audit (nq_api_audit.hip).
#include "nq_handle.h"
#include "nq_linkage_key.h"

#include <algorithm>
#include <chrono>
#include <functional>
#include <string>
#include <vector>

namespace nqi {

bool whole_range(const niqki_index *ix) {
  const uint32_t b = first_slot(ix), e = ix->resident_bytes ? ix->full_end : ix->d.slot_end;
  return b == 0 && e == ix->d.F;
}

// The events, then the batches of genomes [begin, n_run) in index order: a batch's stored rows, read once, their hits at
// the threshold into the fixed hit buffers, then the consumer's kernels.  A split loses the gather and the count of the
// batch, so the following batches start from the size that fitted and stay there (HitLists::shrink).
int self_join_batches(SelfJoin &r, uint32_t n_run, uint32_t begin) {
  niqki_index *ix = r.ix;
  int rc = r.ev.create();
  if (rc) return rc;
  const SketchSource rows = stored_rows(ix, begin);
  const SketchSource timed_rows = [&](uint32_t q0, uint32_t n, const int32_t **d_sk) {
    int rc_ = r.ev.mark(0);
    if (!rc_) rc_ = rows(q0, n, d_sk);
    return rc_ ? rc_ : r.ev.mark(1);
  };
  HitLists hl{ix, r.who, r.ev, 2, r.stats.splits, true};
  hl.consume = [&](const HitOut &out, const int32_t *, uint32_t q_at, uint32_t n) {
    int rc_ = r.ev.mark(3);
    if (!rc_) rc_ = r.consume(out.off, out.counts, out.gids, begin + hl.q0 + q_at, n);
    for (int k = 1; k < r.phases && !rc_; ++k) rc_ = r.ev.add(k + 1, k + 2, k);
    if (!rc_ && (ix->prof || r.count_pairs)) r.stats.pairs += out.total;
    return rc_;
  };
  hl.after = [&](uint32_t, uint32_t) { return r.ev.add(0, 1, 0); };
  return hl.run(timed_rows, n_run - begin, std::max<uint32_t>(ix->query_batch, 1));
}

namespace {

int cluster_run(niqki_index *ix, uint32_t *labels, uint32_t *n_clusters, int mem) {
  const uint32_t N = ix->n_genomes;
  int rc = build_if_needed(ix);
  if (rc) return rc;
  // parent[N], labels[N] (device copy of a host result), the root count
  if ((rc = ensure(ix, ix->ws_parent, ((size_t)N * 2 + 1) * 4))) return rc;
  uint32_t *parent = (uint32_t *)ix->ws_parent.p;
  uint32_t *d_labels = mem == NIQKI_MEM_DEVICE ? labels : parent + N, *d_roots = parent + 2 * (size_t)N;
  SelfJoin r(ix, "niqki_cluster", ix->cluster_stats, 3);
  r.consume = [&](const unsigned long long *off, const uint32_t *, const uint32_t *hg, uint32_t t0, uint32_t n) {
    NQ_HIP(ix, nq::launch_cluster_link(parent, N, off, hg, t0, n, ix->stream));
    return r.ev.mark(4);
  };
  NQ_HIP(ix, nq::launch_cluster_init(parent, N, ix->stream));
  if ((rc = self_join_batches(r, N))) return rc;
  if ((rc = r.ev.mark(0))) return rc;
  NQ_HIP(ix, nq::launch_cluster_flatten(parent, N, d_labels, d_roots, ix->stream));
  if ((rc = r.ev.mark(1))) return rc;
  uint32_t roots = 0;
  if (mem != NIQKI_MEM_DEVICE) NQ_HIP(ix, hipMemcpyAsync(labels, d_labels, (size_t)N * 4, hipMemcpyDeviceToHost, ix->stream));
  NQ_HIP(ix, hipMemcpyAsync(&roots, d_roots, 4, hipMemcpyDeviceToHost, ix->stream));
  NQ_HIP(ix, hipStreamSynchronize(ix->stream));
  if ((rc = r.ev.add(0, 1, 3))) return rc;   // flatten
  if (n_clusters) *n_clusters = roots;
  return NIQKI_OK;
}

// threshold 0 links every pair, so genome 0 is the only representative: only ITS list is made (at min_score 0 it holds
// every genome with its count), the other genomes start as covered.
// first > 0 (niqki_dereplicate_from): the genomes below it start as representatives and have no lists; the batches
// start at `first` and each one also takes the given representatives' offers from its own lists (nq_cluster.hip).
int derep_run(niqki_index *ix, uint32_t first, uint32_t threshold, uint32_t *labels, uint32_t *label_counts, uint32_t *n_reps, int mem) {
  const uint32_t N = ix->n_genomes;
  int rc = build_if_needed(ix);
  if (rc) return rc;
  // best[N] (8 bytes), labels[N] and label_counts[N] (device copies of host results), info[4], state[N]
  const bool dev = mem == NIQKI_MEM_DEVICE;
  if ((rc = ensure(ix, ix->ws_parent, (size_t)N * 17 + 16))) return rc;
  unsigned long long *best = (unsigned long long *)ix->ws_parent.p;
  uint32_t *own_labels = (uint32_t *)(best + N), *own_counts = own_labels + N;
  uint32_t *info = own_counts + N;   // [0] rounds, [1] [2] flags of a batch's first two rounds, [3] the representative count
  uint8_t *state = (uint8_t *)(info + 4);
  uint32_t *d_labels = dev ? labels : own_labels, *d_counts = !label_counts ? nullptr : dev ? label_counts : own_counts;
  SelfJoin r(ix, "niqki_dereplicate", ix->derep_stats, 4);
  r.consume = [&](const unsigned long long *off, const uint32_t *hc, const uint32_t *hg, uint32_t t0, uint32_t n) {
    NQ_HIP(ix, nq::launch_derep_decide(state, N, off, hg, t0, n, info, ix->stream));
    int rc_ = r.ev.mark(4);
    if (rc_) return rc_;
    NQ_HIP(ix, nq::launch_derep_assign(state, best, N, off, hc, hg, t0, n, ix->stream));
    NQ_HIP(ix, nq::launch_derep_given(best, N, first, off, hc, hg, t0, n, ix->stream));
    return r.ev.mark(5);
  };
  NQ_HIP(ix, hipMemsetAsync(best, 0, (size_t)N * 8, ix->stream));
  NQ_HIP(ix, hipMemsetAsync(info, 0, 16, ix->stream));
  // (with given genomes threshold 0 needs no special case: every list holds a given representative)
  const bool all_linked = !threshold && !first;
  NQ_HIP(ix, hipMemsetAsync(state, all_linked ? nq::kCovered : nq::kUndecided, N, ix->stream));
  if (all_linked) NQ_HIP(ix, hipMemsetAsync(state, nq::kUndecided, 1, ix->stream));
  if (first) NQ_HIP(ix, hipMemsetAsync(state, nq::kRep, first, ix->stream));
  if ((rc = self_join_batches(r, all_linked ? 1 : N, first))) return rc;
  uint32_t out[4] = {0, 0, 0, 0};
  NQ_HIP(ix, nq::launch_derep_finish(state, best, N, d_labels, d_counts, info + 3, ix->stream));
  if (!dev) NQ_HIP(ix, hipMemcpyAsync(labels, d_labels, (size_t)N * 4, hipMemcpyDeviceToHost, ix->stream));
  if (!dev && label_counts) NQ_HIP(ix, hipMemcpyAsync(label_counts, d_counts, (size_t)N * 4, hipMemcpyDeviceToHost, ix->stream));
  NQ_HIP(ix, hipMemcpyAsync(out, info, 16, hipMemcpyDeviceToHost, ix->stream));
  NQ_HIP(ix, hipStreamSynchronize(ix->stream));
  ix->derep_stats.rounds = out[0];
  if (n_reps) *n_reps = out[3];
  return NIQKI_OK;
}

// smallest-id-root union-find on the host (the hierarchy of niqki_linkage); find() halves paths, no recursion
struct HostForest {
  std::vector<uint32_t> parent;
  explicit HostForest(uint32_t n) : parent(n) {
    for (uint32_t g = 0; g < n; ++g) parent[g] = g;
  }
  uint32_t find(uint32_t x) {
    while (parent[x] != x) {
      parent[x] = parent[parent[x]];
      x = parent[x];
    }
    return x;
  }
};

// One self-join at max(floor, 1); the consumer keeps the maximum spanning forest of everything seen so far (nq_cluster.hip).
// After the last batch the forest, fewer than N keys, crosses to the host once, is sorted into the edge order and gives
// the edge arrays and the hierarchy: a union-find with the smaller id as root, level by level (a level = the edges of
// one count); merge_into is the root at the END of the level that took g's root status.
int linkage_run(niqki_index *ix, uint32_t floor, uint32_t *merge_into, uint32_t *merge_count, uint32_t *edge_lo, uint32_t *edge_hi,
                uint32_t *edge_count, uint32_t *n_roots, int mem) {
  const uint32_t N = ix->n_genomes;
  int rc = build_if_needed(ix);
  if (rc) return rc;
  // best[N], two forests [N] (8 bytes each), comp[N], info
  const uint32_t info_words = nq::kLinkageInfoHead + nq::linkage_rounds(N);
  if ((rc = ensure(ix, ix->ws_parent, (size_t)N * 28 + (size_t)info_words * 4))) return rc;
  unsigned long long *best = (unsigned long long *)ix->ws_parent.p, *forest[2] = {best + N, best + 2 * (size_t)N};
  uint32_t *comp = (uint32_t *)(best + 3 * (size_t)N), *info = comp + N;
  int cur = 0;   // forest[cur] holds the forest so far
  SelfJoin r(ix, "niqki_linkage", ix->linkage_stats, 3);
  r.count_pairs = true;
  r.consume = [&](const unsigned long long *off, const uint32_t *hc, const uint32_t *hg, uint32_t t0, uint32_t n) {
    NQ_HIP(ix, nq::launch_linkage_batch(comp, best, forest[cur], forest[cur ^ 1], info, N, off, hc, hg, t0, n, ix->stream));
    cur ^= 1;
    return r.ev.mark(4);
  };
  NQ_HIP(ix, hipMemsetAsync(info, 0, (size_t)info_words * 4, ix->stream));
  if ((rc = self_join_batches(r, N))) return rc;
  const auto t_finish = std::chrono::steady_clock::now();
  uint32_t head[4] = {0, 0, 0, 0};
  std::vector<unsigned long long> keys(N);
  NQ_HIP(ix, hipMemcpyAsync(head, info, 16, hipMemcpyDeviceToHost, ix->stream));
  NQ_HIP(ix, hipMemcpyAsync(keys.data(), forest[cur], (size_t)N * 8, hipMemcpyDeviceToHost, ix->stream));
  NQ_HIP(ix, hipStreamSynchronize(ix->stream));
  ix->linkage_stats.rounds = head[2];
  if (head[3] || head[0] >= N) return fail(ix, NIQKI_E_STATE, "niqki_linkage: the forest rounds did not end (a bug)");
  keys.resize(head[0]);
  std::sort(keys.begin(), keys.end(), std::greater<unsigned long long>());
  const uint32_t n_tree = (uint32_t)keys.size();
  // floor 0: every remaining root r > 0 joins genome 0 at count 0, ascending r, behind the others
  std::vector<uint32_t> into(N), cnt(N, 0u), losers;
  HostForest uf(N);
  for (uint32_t g = 0; g < N; ++g) into[g] = g;
  for (uint32_t e = 0; e < n_tree;) {
    const uint32_t c = nq::linkage_count(keys[e]);
    losers.clear();
    for (; e < n_tree && nq::linkage_count(keys[e]) == c; ++e) {
      const uint32_t a = uf.find(nq::linkage_lo(keys[e])), b = uf.find(nq::linkage_hi(keys[e]));
      if (a == b) return fail(ix, NIQKI_E_STATE, "niqki_linkage: the forest holds a cycle (a bug)");
      uf.parent[std::max(a, b)] = std::min(a, b);
      losers.push_back(std::max(a, b));
    }
    for (uint32_t g : losers) {
      into[g] = uf.find(g);
      cnt[g] = c;
    }
  }
  std::vector<uint32_t> zero_roots;
  if (floor == 0)
    for (uint32_t g = 1; g < N; ++g)
      if (into[g] == g) {
        zero_roots.push_back(g);
        into[g] = 0;
      }
  const uint32_t n_edges = n_tree + (uint32_t)zero_roots.size();
  std::vector<uint32_t> el, eh, ec;
  if (edge_lo) {
    el.resize(n_edges);
    eh.resize(n_edges);
    ec.resize(n_edges);
    for (uint32_t e = 0; e < n_tree; ++e) {
      el[e] = nq::linkage_lo(keys[e]);
      eh[e] = nq::linkage_hi(keys[e]);
      ec[e] = nq::linkage_count(keys[e]);
    }
    for (uint32_t k = 0; k < zero_roots.size(); ++k) {
      el[n_tree + k] = 0;
      eh[n_tree + k] = zero_roots[k];
      ec[n_tree + k] = 0;
    }
  }
  if (mem == NIQKI_MEM_DEVICE) {
    if (merge_into) {
      NQ_HIP(ix, hipMemcpyAsync(merge_into, into.data(), (size_t)N * 4, hipMemcpyHostToDevice, ix->stream));
      NQ_HIP(ix, hipMemcpyAsync(merge_count, cnt.data(), (size_t)N * 4, hipMemcpyHostToDevice, ix->stream));
    }
    if (edge_lo && n_edges) {
      NQ_HIP(ix, hipMemcpyAsync(edge_lo, el.data(), (size_t)n_edges * 4, hipMemcpyHostToDevice, ix->stream));
      NQ_HIP(ix, hipMemcpyAsync(edge_hi, eh.data(), (size_t)n_edges * 4, hipMemcpyHostToDevice, ix->stream));
      NQ_HIP(ix, hipMemcpyAsync(edge_count, ec.data(), (size_t)n_edges * 4, hipMemcpyHostToDevice, ix->stream));
    }
    NQ_HIP(ix, hipStreamSynchronize(ix->stream));   // (the vectors leave scope)
  } else {
    if (merge_into) {
      std::copy(into.begin(), into.end(), merge_into);
      std::copy(cnt.begin(), cnt.end(), merge_count);
    }
    if (edge_lo) {
      std::copy(el.begin(), el.end(), edge_lo);
      std::copy(eh.begin(), eh.end(), edge_hi);
      std::copy(ec.begin(), ec.end(), edge_count);
    }
  }
  if (ix->prof) ix->linkage_stats.ms[3] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_finish).count();
  if (n_roots) *n_roots = N - n_edges;
  return NIQKI_OK;
}

}  // namespace

}  // namespace nqi

using namespace nqi;

extern "C" {

int niqki_neighbors_range(niqki_index *ix, uint32_t begin, uint32_t end, uint64_t *hit_off, uint32_t *hit_counts,
                          uint32_t *hit_gids, uint64_t capacity, int mem) {
  if (!ix || !hit_off) return NIQKI_E_INVALID;
  if (begin > end || end > ix->n_genomes) return fail(ix, NIQKI_E_INVALID, "genome range out of bounds");
  if (!whole_range(ix)) return fail(ix, NIQKI_E_STATE, "niqki_neighbors_range: a slot-range shard sees partial counts; the self-join needs a whole-range handle");
  NQ_HIP(ix, hipSetDevice(ix->device));
  int rc = build_if_needed(ix);
  if (rc) return rc;
  const uint32_t nq = end - begin;
  if (mem == NIQKI_MEM_DEVICE) {
    const uint64_t stride = NIQKI_ROW_STRIDE(ix->built_n);
    Planes pl;
    HitOut out{(unsigned long long *)hit_off, hit_counts, hit_gids, capacity};
    if ((rc = ensure(ix, ix->ws_misc, std::max<size_t>((size_t)nq * ix->d.F * 4, 4)))) return rc;
    if ((rc = counter_planes(ix, nq, stride, pl))) return rc;
    if ((rc = stored_sketch_rows(ix, begin, nq, (int32_t *)ix->ws_misc.p))) return rc;
    return query_hits_dev(ix, (const int32_t *)ix->ws_misc.p, nq, pl, stride, out);
  }
  // batches of query_batch stored sketches through the host path of niqki_query
  return query_to_host(ix, stored_rows(ix, begin), nq, std::max<uint32_t>(ix->query_batch, 1), hit_off, hit_counts, hit_gids, capacity);
}

int niqki_cluster(niqki_index *ix, uint32_t threshold, uint32_t *labels, uint32_t *n_clusters, int mem) {
  if (!ix || (!labels && ix->n_genomes)) return NIQKI_E_INVALID;
  if (!whole_range(ix)) return fail(ix, NIQKI_E_STATE, "niqki_cluster: a slot-range shard sees partial counts; the self-join needs a whole-range handle");
  NQ_HIP(ix, hipSetDevice(ix->device));
  const uint32_t N = ix->n_genomes;
  ix->cluster_stats = SelfJoinStats();
  if (N == 0) {
    if (n_clusters) *n_clusters = 0;
    return NIQKI_OK;
  }
  if (threshold == 0) {   // every pair is linked
    if (mem == NIQKI_MEM_DEVICE) {
      NQ_HIP(ix, hipMemsetAsync(labels, 0, (size_t)N * 4, ix->stream));
    } else {
      std::fill(labels, labels + N, 0u);
    }
    if (n_clusters) *n_clusters = 1;
    return NIQKI_OK;
  }
  CallParams guard(ix, threshold, 0);
  return cluster_run(ix, labels, n_clusters, mem);
}

int niqki_dereplicate_from(niqki_index *ix, uint32_t first, uint32_t threshold, uint32_t *labels, uint32_t *label_counts,
                           uint32_t *n_representatives, int mem) {
  if (!ix || (!labels && ix->n_genomes)) return NIQKI_E_INVALID;
  if (!whole_range(ix)) return fail(ix, NIQKI_E_STATE, "niqki_dereplicate: a slot-range shard sees partial counts; the self-join needs a whole-range handle");
  NQ_HIP(ix, hipSetDevice(ix->device));
  ix->derep_stats = SelfJoinStats();
  const uint32_t N = ix->n_genomes;
  if (N == 0) {
    if (n_representatives) *n_representatives = 0;
    return NIQKI_OK;
  }
  if (first >= N) {   // every genome is given: all are representatives, no kernel runs
    if (mem == NIQKI_MEM_DEVICE) {
      std::vector<uint32_t> ids(N);
      for (uint32_t g = 0; g < N; ++g) ids[g] = g;
      NQ_HIP(ix, hipMemcpyAsync(labels, ids.data(), (size_t)N * 4, hipMemcpyHostToDevice, ix->stream));
      if (label_counts) NQ_HIP(ix, hipMemsetAsync(label_counts, 0, (size_t)N * 4, ix->stream));
      NQ_HIP(ix, hipStreamSynchronize(ix->stream));   // (ids leaves scope)
    } else {
      for (uint32_t g = 0; g < N; ++g) labels[g] = g;
      if (label_counts) std::fill(label_counts, label_counts + N, 0u);
    }
    if (n_representatives) *n_representatives = N;
    return NIQKI_OK;
  }
  CallParams guard(ix, threshold, 0);
  return derep_run(ix, first, threshold, labels, label_counts, n_representatives, mem);
}

int niqki_dereplicate(niqki_index *ix, uint32_t threshold, uint32_t *labels, uint32_t *label_counts, uint32_t *n_representatives,
                      int mem) {
  return niqki_dereplicate_from(ix, 0, threshold, labels, label_counts, n_representatives, mem);
}

int niqki_linkage(niqki_index *ix, uint32_t floor, uint32_t *merge_into, uint32_t *merge_count, uint32_t *edge_lo, uint32_t *edge_hi,
                  uint32_t *edge_count, uint32_t *n_roots, int mem) {
  if (!ix) return NIQKI_E_INVALID;
  if (!merge_into != !merge_count) return fail(ix, NIQKI_E_INVALID, "niqki_linkage: merge_into and merge_count go together");
  if (!edge_lo != !edge_hi || !edge_lo != !edge_count) return fail(ix, NIQKI_E_INVALID, "niqki_linkage: the three edge arrays go together");
  if (!whole_range(ix)) return fail(ix, NIQKI_E_STATE, "niqki_linkage: a slot-range shard sees partial counts; the self-join needs a whole-range handle");
  NQ_HIP(ix, hipSetDevice(ix->device));
  ix->linkage_stats = SelfJoinStats();
  const uint32_t N = ix->n_genomes;
  if (N == 0) {
    if (n_roots) *n_roots = 0;
    return NIQKI_OK;
  }
  if (!nq::linkage_fits(N)) return fail(ix, NIQKI_E_INVALID, "niqki_linkage: more than 2^23 genomes (the edge key holds 23 bits an id)");
  CallParams guard(ix, std::max(floor, 1u), 0);
  return linkage_run(ix, floor, merge_into, merge_count, edge_lo, edge_hi, edge_count, n_roots, mem);
}

}  // extern "C"
