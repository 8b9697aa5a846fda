// nq_cluster.hip -- the self-join of an index: niqki_neighbors_range (the hits of the stored sketches, the sparse form
// of Index::query_range, src/niqki_index.cpp:570-610) and niqki_cluster (single-linkage clusters: the link and flatten
// kernels over the hit lists of the stored sketches) and niqki_dereplicate (greedy representatives in index order: the
// decide, assign and finish kernels over the same hit lists).  DESIGN.md 4.6b, 4.6c.
#include "nq_handle.h"

#include <algorithm>
#include <string>

namespace nq {

// ---- union-find on the device ------------------------------------------------------------------------------------
// parent[] invariants, true at every moment of a link launch for the values in MEMORY:
//   (1) parent[x] <= x, and parent[x] is a genome of x's component (the component the links made so far define);
//   (2) x is a root while parent[x] == x; a root stops being one only by the compare-and-swap of hook() below, which
//       puts a SMALLER id there; nothing ever writes parent[x] = x again, so "x is not a root" is permanent;
//   (3) chains strictly descend, so they end at a root and there is no cycle, and a root is the smallest id of its tree.
// Writers: hook()'s compare-and-swap (parent[hi]: hi -> lo, lo < hi, lo from the other component: the link itself) and
// the path halving of find() (parent[x]: p -> parent[p] for a non-root x, a value at or above x's root in x's own
// chain).  Both keep (1)-(3); a halving store that lands after a newer one only puts back an older, higher ancestor.
//
// Coherence.  The eight XCD L2s are not coherent for plain loads, so every read of parent[] in the link kernel is an
// agent-scope relaxed atomic load (global_load sc1: past the L1), every halving store an agent-scope relaxed atomic
// store, and the hook an agent-scope compare-and-swap, which executes at the memory side on the real value.  The
// kernel does not rely on the loads being fresh, only on their returning a value parent[x] HELD at some time.  By (1)
// and (2) such a value is still a genome of x's component at or below x, so find() returns a genome r of x's
// component; r may have stopped being a root.  Then:
//   * equal results for t and g prove that t and g are in one component: skipping the pair loses nothing;
//   * different results go to hook(): its compare-and-swap succeeds only if parent[hi] == hi in memory, i.e. hi is a
//     root NOW, and then the two components are one (lo is in the other one, or -- where a stale read hid that they
//     had been joined already -- in the same one, below hi: harmless).  If it fails it returns the real parent[hi],
//     from which the search goes on, so every retry moves strictly down a chain with a value no staleness can
//     repeat.  A stale read therefore costs at most a failed compare-and-swap and a retry, never a link.
// Between launches (init -> link ... link -> flatten) the stream order makes everything visible; the flatten kernel
// only reads parent[] and uses plain loads.
//
// Contention.  One contended word takes 11-13 ns per atomic, and a species of 50 000 genomes is ONE component with
// ~10^9 hits, nearly all of them redundant.  So roots are found with loads and no atomic is issued when they are equal;
// a wavefront works on one query t, whose lanes share the root of t; of the lanes of a step that met a foreign root,
// one per DISTINCT root hooks (the others see the same root or the new one and drop out), so a query issues one
// successful hook per foreign component it meets; all hooks of a call that succeed number exactly N - clusters.

constexpr uint32_t kLinkBlock = 256;   // 4 wavefronts, one query each

__device__ __forceinline__ uint32_t uf_load(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// a genome of x's component that read as a root; halves the path it walks
__device__ __forceinline__ uint32_t uf_find(uint32_t *parent, uint32_t x) {
  for (;;) {
    const uint32_t p = uf_load(parent + x);
    if (p == x) return x;
    const uint32_t gp = uf_load(parent + p);
    if (gp == p) return p;
    __hip_atomic_store(parent + x, gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // x is not a root and never will be
    x = gp;
  }
}

// unites the components of a and b (results of uf_find); returns a genome of the united component that read as its root
__device__ __forceinline__ uint32_t uf_hook(uint32_t *parent, uint32_t a, uint32_t b) {
  while (a != b) {
    const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
    uint32_t seen = hi;
    if (__hip_atomic_compare_exchange_strong(parent + hi, &seen, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
      return lo;
    a = uf_find(parent, seen);   // seen = the real parent[hi] < hi
    b = lo;
  }
  return a;
}

__global__ void cluster_init_kernel(uint32_t *parent, uint32_t n) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g < n) parent[g] = g;
}

__global__ __launch_bounds__(kLinkBlock) void cluster_link_kernel(uint32_t *parent, uint32_t n, const unsigned long long *hit_off,
                                                                  const uint32_t *hit_gids, uint32_t t0, uint32_t nq) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t q = blockIdx.x * (kLinkBlock / 64) + (threadIdx.x >> 6);   // wave-uniform
  if (q >= nq) return;
  const uint32_t t = t0 + q;
  if (t >= n) return;
  const unsigned long long lo = hit_off[q], hi = hit_off[q + 1];
  uint32_t rt = t;
  for (unsigned long long i0 = lo; i0 < hi; i0 += 64) {
    const unsigned long long i = i0 + lane;
    // the relation is symmetric: the pair (t, g) with g > t is linked by query g, g == t is no link
    const uint32_t g = i < hi ? hit_gids[i] : 0xFFFFFFFFu;
    const bool take = g < t;   // (also g < n: t < n)
    if (!__any(take)) continue;
    // (every lane walks from the same rt, normally with the same result; nothing below needs that: a lane compares
    // its rg with its OWN rt, and all lanes take `joined` after a hook)
    rt = uf_find(parent, rt);
    uint32_t rg = take ? uf_find(parent, g) : rt;
    // one hook per distinct foreign root of this step
    for (;;) {
      const unsigned long long foreign = __ballot(rg != rt);
      if (!foreign) break;
      const int leader = __ffsll((long long)foreign) - 1;
      const uint32_t r = (uint32_t)__shfl((int)rg, leader);
      uint32_t joined = 0;
      if ((int)lane == leader) joined = uf_hook(parent, rt, r);
      joined = (uint32_t)__shfl((int)joined, leader);
      if (rg == r || rg == rt) rg = joined;
      rt = joined;
    }
  }
}

// labels[g] = the root of g's tree = the smallest id of its component; the roots are counted per wavefront
__global__ void cluster_flatten_kernel(const uint32_t *parent, uint32_t n, uint32_t *labels, uint32_t *n_roots) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  bool root = false;
  if (g < n) {
    uint32_t x = g, p = parent[x];
    while (p != x) { x = p; p = parent[x]; }
    labels[g] = x;
    root = x == g;
  }
  const unsigned long long m = __ballot(root);
  if (m && (threadIdx.x & 63u) == (uint32_t)(__ffsll((long long)m) - 1)) atomicAdd(n_roots, (uint32_t)__popcll(m));
}

// ---- greedy representatives on the device (niqki_dereplicate) ---------------------------------------
// state[g]: kUndecided -> kRep | kCovered, once, never back.  Genome t is a representative iff no representative g < t
// is linked to it.  A wavefront decides t from the states of t's hits g < t:
//   some g is a representative                -> t is covered   (final: g stays a representative)
//   else no g is undecided (all are covered)  -> t is a representative   (final: covered genomes stay covered)
//   else                                      -> t waits for the next round.
// Both decisions rest on FINAL states only, so a read that returns an older value of state[g] -- which can only be
// kUndecided where memory already holds a decision -- can make t wait one round more and can never change what t
// becomes.  No wave ever waits for another one inside a round.  The lowest undecided genome of a batch has no
// undecided hit below it (earlier batches are decided before this one starts), so every round decides at least that
// one and a batch of n needs at most n rounds; a path in index order takes them all.
//
// Rounds of a batch.  Two launches over the whole batch, one wavefront per query, waves of decided queries leave at
// once: they read state[] with plain loads and see exactly what earlier launches of the stream wrote (round 1 makes
// the heads of groups representatives, round 2 covers everything linked to one -- the shape of near-identical
// genomes).  What is left goes to ONE workgroup of 16 waves that runs all remaining rounds by itself, a workgroup
// barrier between rounds and no host synchronisation: wave w takes the queries [64 w, 64 w + 64) (+ 1024 k) of the
// batch, reads their 64 states in one load and decides the undecided ones in index order, so a run of dependent
// genomes inside its 64 is settled in one round.  Here a round may see decisions of its own launch: every access to
// state[] in that kernel is an agent-scope relaxed atomic (global_load / global_store sc1: past the L1, which is never
// refreshed), and by the argument above a value that is stale all the same only delays.
// A round of the finisher with nothing to decide costs one state load per wave and the barrier.
//
// best[g] = max over the representatives r linked to g of (count(g, r) << 32 | ~r): the largest count, among equal
// counts the smallest r.  After a batch is decided, the wave of every representative t of the batch walks t's whole
// list once more and issues one agent-scope 64-bit atomicMax per hit g != t -- members before and after t alike.
// Representatives are pairwise unlinked, so a genome receives one atomic per representative it is linked to and no
// word is hot.  A covered genome has at least one linked representative below it, so its best[] is set when the last
// batch is through.

enum : uint8_t { kUndecided = 0, kRep = 1, kCovered = 2 };
constexpr uint32_t kFinisherBlock = 1024;

// kFresh: state[] through agent-scope atomics (the finisher); otherwise plain loads of what earlier launches wrote
template <bool kFresh>
__device__ __forceinline__ uint8_t derep_decide(const uint8_t *state, const unsigned long long *hit_off, const uint32_t *hit_gids,
                                                uint32_t q, uint32_t t, uint32_t lane) {
  const unsigned long long lo = hit_off[q], hi = hit_off[q + 1];
  bool waits = false;
  for (unsigned long long i0 = lo; i0 < hi; i0 += 64) {
    const unsigned long long i = i0 + lane;
    const uint32_t g = i < hi ? hit_gids[i] : 0xFFFFFFFFu;
    uint8_t s = kCovered;   // the relation is symmetric: hits g > t are decided after t; g == t is no link
    if (g < t) s = kFresh ? __hip_atomic_load(state + g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : state[g];
    if (__any(s == kRep)) return kCovered;
    waits |= __any(s == kUndecided) != 0;
  }
  return waits ? kUndecided : kRep;
}

__global__ __launch_bounds__(kLinkBlock) void derep_round_kernel(uint8_t *state, uint32_t n, const unsigned long long *hit_off,
                                                                 const uint32_t *hit_gids, uint32_t t0, uint32_t nq, uint32_t *left) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t q = blockIdx.x * (kLinkBlock / 64) + (threadIdx.x >> 6);   // wave-uniform
  if (q >= nq) return;
  const uint32_t t = t0 + q;
  if (t >= n || state[t] != kUndecided) return;
  const uint8_t s = derep_decide<false>(state, hit_off, hit_gids, q, t, lane);
  if (lane == 0) {
    if (s != kUndecided) state[t] = s;
    else *left = 1;   // (every wave that waits stores the same word)
  }
}

// info[0]: the largest round count of a batch so far; info[1], info[2]: rounds 1 and 2 of this batch left something
__global__ __launch_bounds__(kFinisherBlock) void derep_finisher_kernel(uint8_t *state, uint32_t n, const unsigned long long *hit_off,
                                                                        const uint32_t *hit_gids, uint32_t t0, uint32_t nq, uint32_t *info) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t rounds = 0;
  for (;;) {
    bool left = false;
    for (uint32_t base = wave * 64; base < nq; base += kFinisherBlock) {
      const uint32_t q = base + lane;
      const bool mine = q < nq && t0 + q < n;
      const uint8_t s = mine ? __hip_atomic_load(state + t0 + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : (uint8_t)kCovered;
      unsigned long long todo = __ballot(s == kUndecided);
      while (todo) {   // in index order: a decision is seen by the next one of this wave where the load is fresh
        const uint32_t b = (uint32_t)__ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const uint8_t d = derep_decide<true>(state, hit_off, hit_gids, base + b, t0 + base + b, lane);
        if (d == kUndecided) left = true;
        else if (lane == 0) __hip_atomic_store(state + t0 + base + b, d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    // (the stores are write-through; one that has not landed when another wave reads only delays that decision a round)
    if (!__syncthreads_or(left)) break;
    rounds += 1;
  }
  if (threadIdx.x == 0) {
    // round 1 always had work, round 2 if round 1 left something, and if round 2 did, every pass of the loop above
    const uint32_t all = 1 + (info[1] ? 1 : 0) + (info[2] ? 1 + rounds : 0);
    if (all > info[0]) info[0] = all;
    info[1] = 0;
    info[2] = 0;
  }
}

__global__ __launch_bounds__(kLinkBlock) void derep_assign_kernel(const uint8_t *state, unsigned long long *best, uint32_t n,
                                                                  const unsigned long long *hit_off, const uint32_t *hit_counts,
                                                                  const uint32_t *hit_gids, uint32_t t0, uint32_t nq) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t q = blockIdx.x * (kLinkBlock / 64) + (threadIdx.x >> 6);   // wave-uniform
  if (q >= nq) return;
  const uint32_t t = t0 + q;
  if (t >= n || state[t] != kRep) return;
  const unsigned long long lo = hit_off[q], hi = hit_off[q + 1];
  for (unsigned long long i = lo + lane; i < hi; i += 64) {
    const uint32_t g = hit_gids[i];
    if (g == t || g >= n) continue;
    const unsigned long long v = ((unsigned long long)hit_counts[i] << 32) | (uint32_t)~t;
    __hip_atomic_fetch_max(best + g, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// labels / label_counts (may be null) from state[] and best[]; the representatives are counted per wavefront
__global__ void derep_finish_kernel(const uint8_t *state, const unsigned long long *best, uint32_t n, uint32_t *labels,
                                    uint32_t *label_counts, uint32_t *n_reps) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  bool rep = false;
  if (g < n) {
    rep = state[g] == kRep;
    const unsigned long long b = best[g];
    labels[g] = rep ? g : ~(uint32_t)b;
    if (label_counts) label_counts[g] = rep ? 0u : (uint32_t)(b >> 32);
  }
  const unsigned long long m = __ballot(rep);
  if (m && (threadIdx.x & 63u) == (uint32_t)(__ffsll((long long)m) - 1)) atomicAdd(n_reps, (uint32_t)__popcll(m));
}

hipError_t launch_cluster_init(uint32_t *parent, uint32_t n, hipStream_t stream) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(cluster_init_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, parent, n);
  return hipGetLastError();
}

hipError_t launch_cluster_link(uint32_t *parent, uint32_t n, const unsigned long long *hit_off, const uint32_t *hit_gids,
                               uint32_t t0, uint32_t nq, hipStream_t stream) {
  if (!nq || !n) return hipSuccess;
  const uint32_t per = kLinkBlock / 64;
  hipLaunchKernelGGL(cluster_link_kernel, dim3((nq + per - 1) / per), dim3(kLinkBlock), 0, stream, parent, n, hit_off, hit_gids, t0, nq);
  return hipGetLastError();
}

hipError_t launch_cluster_flatten(const uint32_t *parent, uint32_t n, uint32_t *labels, uint32_t *n_roots, hipStream_t stream) {
  hipError_t e = hipMemsetAsync(n_roots, 0, 4, stream);
  if (e != hipSuccess || !n) return e;
  hipLaunchKernelGGL(cluster_flatten_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, parent, n, labels, n_roots);
  return hipGetLastError();
}

hipError_t launch_derep_decide(uint8_t *state, uint32_t n, const unsigned long long *hit_off, const uint32_t *hit_gids, uint32_t t0,
                               uint32_t nq, uint32_t *info, hipStream_t stream) {
  if (!nq || !n) return hipSuccess;
  const uint32_t per = kLinkBlock / 64;
  for (uint32_t round = 1; round <= 2; ++round)
    hipLaunchKernelGGL(derep_round_kernel, dim3((nq + per - 1) / per), dim3(kLinkBlock), 0, stream, state, n, hit_off, hit_gids, t0, nq,
                       info + round);
  hipLaunchKernelGGL(derep_finisher_kernel, dim3(1), dim3(kFinisherBlock), 0, stream, state, n, hit_off, hit_gids, t0, nq, info);
  return hipGetLastError();
}

hipError_t launch_derep_assign(const uint8_t *state, unsigned long long *best, uint32_t n, const unsigned long long *hit_off,
                               const uint32_t *hit_counts, const uint32_t *hit_gids, uint32_t t0, uint32_t nq, hipStream_t stream) {
  if (!nq || !n) return hipSuccess;
  const uint32_t per = kLinkBlock / 64;
  hipLaunchKernelGGL(derep_assign_kernel, dim3((nq + per - 1) / per), dim3(kLinkBlock), 0, stream, state, best, n, hit_off, hit_counts,
                     hit_gids, t0, nq);
  return hipGetLastError();
}

hipError_t launch_derep_finish(const uint8_t *state, const unsigned long long *best, uint32_t n, uint32_t *labels, uint32_t *label_counts,
                               uint32_t *n_reps, hipStream_t stream) {
  hipError_t e = hipMemsetAsync(n_reps, 0, 4, stream);
  if (e != hipSuccess || !n) return e;
  hipLaunchKernelGGL(derep_finish_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, state, best, n, labels, label_counts, n_reps);
  return hipGetLastError();
}

}  // namespace nq

namespace nqi {

bool whole_range(const niqki_index *ix) {
  const uint32_t b = first_slot(ix), e = ix->resident_bytes ? ix->full_end : ix->d.slot_end;
  return b == 0 && e == ix->d.F;
}

// the stored sketches of genomes [t0, t0 + n) as query sketches in device memory: from the store, or -- paged handle --
// zero-copy from the page-locked host store, as niqki_matrix_range reads them
static int read_stored(niqki_index *ix, uint32_t t0, uint32_t n, int32_t *dst) {
  if (!n) return NIQKI_OK;
  if (!ix->resident_bytes) {
    NQ_HIP(ix, nq::launch_store_read(ix->d, ix->store, ix->cap, t0, n, dst, ix->stream));
    return NIQKI_OK;
  }
  nq::Derived d = ix->d;
  d.slot_begin = ix->full_begin;
  d.slot_end = ix->full_end;
  void *dp = nullptr;
  NQ_HIP(ix, hipHostGetDevicePointer(&dp, ix->host_store, 0));
  NQ_HIP(ix, nq::launch_store_read(d, (const uint16_t *)dp, ix->host_cap, t0, n, dst, ix->stream));
  return NIQKI_OK;
}

// counter planes of n query rows in ws_counts (the rows the hit-list form falls back on, or the rows themselves)
static int count_rows(niqki_index *ix, uint32_t n, uint64_t stride, uint16_t **c1, uint16_t **c2) {
  const size_t plane = std::max<size_t>((size_t)n * stride * 2, 2);
  int rc = ensure(ix, ix->ws_counts, plane * (two_planes(ix) ? 2 : 1));
  if (rc) return rc;
  *c1 = (uint16_t *)ix->ws_counts.p;
  *c2 = two_planes(ix) ? (uint16_t *)((char *)ix->ws_counts.p + plane) : nullptr;
  return NIQKI_OK;
}

namespace {

// One self-join with a consumer of the hit buffers: niqki_cluster (the link kernel) or niqki_dereplicate (decide +
// assign).  The batches go in index order and a halved batch finishes its first half before its second: the
// dereplication relies on that (a batch's earlier genomes are all decided), clustering does not care.
struct SelfJoin {
  niqki_index *ix;
  const char *who;
  bool derep;
  uint64_t stride, room;
  uint32_t *parent = nullptr;               // niqki_cluster
  uint8_t *state = nullptr;                 // niqki_dereplicate ...
  unsigned long long *best = nullptr;
  uint32_t *info = nullptr;
  uint64_t *splits, *pairs;                 // the call's stats
  double *ms;                               // read, gather + hits, then the consumer's phases
  hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
};

// genomes [t0, t0 + n): hits at the threshold into the fixed hit buffers, then the consumer's kernels; a batch whose
// hits exceed the room is halved.  The total is known only after the gather and the count, so a split loses that work:
// the following batches start from the size that fitted and stay there (the batch size never grows back within a call).
int self_join_batch(SelfJoin &r, uint32_t t0, uint32_t n, uint32_t *fitted) {
  niqki_index *ix = r.ix;
  int rc;
  uint16_t *c1, *c2;
  if ((rc = ensure(ix, ix->ws_misc, (size_t)n * ix->d.F * 4))) return rc;
  if ((rc = count_rows(ix, n, r.stride, &c1, &c2))) return rc;
  if ((rc = ensure(ix, ix->ws_hitoff, (size_t)(n + 1) * 8))) return rc;
  if (ix->prof) NQ_HIP(ix, hipEventRecord(r.ev[0], ix->stream));
  if ((rc = read_stored(ix, t0, n, (int32_t *)ix->ws_misc.p))) return rc;
  if (ix->prof) NQ_HIP(ix, hipEventRecord(r.ev[1], ix->stream));
  uint64_t total = 0;
  rc = query_hits_dev(ix, (const int32_t *)ix->ws_misc.p, n, c1, c2, r.stride, (unsigned long long *)ix->ws_hitoff.p,
                      (uint32_t *)ix->ws_hc.p, (uint32_t *)ix->ws_hg.p, r.room, true, &total);
  if (rc == NIQKI_E_CAPACITY) {
    if (n == 1) return fail(ix, NIQKI_E_STATE, std::string(r.who) + ": one query's hits exceed the genome count");   // (room >= N)
    *r.splits += 1;
    const uint32_t h = n / 2;
    uint32_t f1 = 0, f2 = 0;
    if ((rc = self_join_batch(r, t0, h, &f1))) return rc;
    if ((rc = self_join_batch(r, t0 + h, n - h, &f2))) return rc;
    *fitted = std::max(1u, std::min(f1, f2));
    return NIQKI_OK;
  }
  if (rc) return rc;
  if (ix->prof) NQ_HIP(ix, hipEventRecord(r.ev[2], ix->stream));
  const unsigned long long *off = (const unsigned long long *)ix->ws_hitoff.p;
  const uint32_t *hc = (const uint32_t *)ix->ws_hc.p, *hg = (const uint32_t *)ix->ws_hg.p;
  int last = 3;
  if (!r.derep) {
    NQ_HIP(ix, nq::launch_cluster_link(r.parent, ix->n_genomes, off, hg, t0, n, ix->stream));
  } else {
    NQ_HIP(ix, nq::launch_derep_decide(r.state, ix->n_genomes, off, hg, t0, n, r.info, ix->stream));
    if (ix->prof) NQ_HIP(ix, hipEventRecord(r.ev[3], ix->stream));
    NQ_HIP(ix, nq::launch_derep_assign(r.state, r.best, ix->n_genomes, off, hc, hg, t0, n, ix->stream));
    last = 4;
  }
  if (ix->prof) {
    NQ_HIP(ix, hipEventRecord(r.ev[last], ix->stream));
    NQ_HIP(ix, hipEventSynchronize(r.ev[last]));
    for (int k = 0; k < last; ++k) {
      float ms = 0;
      NQ_HIP(ix, hipEventElapsedTime(&ms, r.ev[k], r.ev[k + 1]));
      r.ms[k] += ms;
    }
    *r.pairs += total;
  }
  *fitted = n;
  return NIQKI_OK;
}

// the hit buffers, the events, then the batches of genomes [0, n_run) in index order
int self_join_batches(SelfJoin &r, uint32_t n_run) {
  niqki_index *ix = r.ix;
  const uint32_t N = ix->n_genomes;
  r.stride = NIQKI_ROW_STRIDE(N);
  // hit_counts + hit_gids and the two scratch arrays of the same size the hit kernels order them in: 16 bytes a hit;
  // never below N, the hits of one query
  r.room = std::max<uint64_t>(((uint64_t)std::max<uint32_t>(ix->cluster_ws_mib, 1) << 20) / 16, N);
  int rc;
  if ((rc = ensure(ix, ix->ws_hc, (size_t)r.room * 4))) return rc;
  if ((rc = ensure(ix, ix->ws_hg, (size_t)r.room * 4))) return rc;
  uint32_t qb = std::max<uint32_t>(ix->query_batch, 1);
  for (uint32_t t0 = 0; t0 < n_run && !rc;) {
    const uint32_t n = std::min(qb, n_run - t0);
    uint32_t fitted = n;
    rc = self_join_batch(r, t0, n, &fitted);
    if (fitted < n) qb = fitted;   // a split batch: do not gather the following ones twice
    t0 += n;
  }
  return rc;
}

int cluster_run(niqki_index *ix, uint32_t *labels, uint32_t *n_clusters, int mem) {
  const uint32_t N = ix->n_genomes;
  int rc = build_if_needed(ix);
  if (rc) return rc;
  SelfJoin r;
  r.ix = ix;
  r.who = "niqki_cluster";
  r.derep = false;
  r.splits = &ix->cluster_splits;
  r.pairs = &ix->cluster_pairs;
  r.ms = ix->cluster_ms;
  // parent[N], labels[N] (device copy of a host result), the root count
  if ((rc = ensure(ix, ix->ws_parent, ((size_t)N * 2 + 1) * 4))) return rc;
  r.parent = (uint32_t *)ix->ws_parent.p;
  uint32_t *d_labels = mem == NIQKI_MEM_DEVICE ? labels : r.parent + N, *d_roots = r.parent + 2 * (size_t)N;
  hipError_t e0 = hipSuccess;   // (no early return from here on: the events are destroyed below)
  if (ix->prof) for (int k = 0; k < 4; ++k) if (e0 == hipSuccess) e0 = hipEventCreate(&r.ev[k]);
  if (e0 == hipSuccess) e0 = nq::launch_cluster_init(r.parent, N, ix->stream);
  if (e0 != hipSuccess) rc = fail(ix, NIQKI_E_HIP, std::string("niqki_cluster: ") + hipGetErrorString(e0));
  if (!rc) rc = self_join_batches(r, N);
  if (!rc) {
    hipError_t e = hipSuccess;
    if (ix->prof) e = hipEventRecord(r.ev[0], ix->stream);
    if (e == hipSuccess) e = nq::launch_cluster_flatten(r.parent, N, d_labels, d_roots, ix->stream);
    if (e == hipSuccess && ix->prof) e = hipEventRecord(r.ev[1], ix->stream);
    uint32_t roots = 0;
    if (e == hipSuccess && mem != NIQKI_MEM_DEVICE) e = hipMemcpyAsync(labels, d_labels, (size_t)N * 4, hipMemcpyDeviceToHost, ix->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&roots, d_roots, 4, hipMemcpyDeviceToHost, ix->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ix->stream);
    if (e == hipSuccess && ix->prof) {
      float ms = 0;
      e = hipEventElapsedTime(&ms, r.ev[0], r.ev[1]);
      ix->cluster_ms[3] = ms;
    }
    if (e != hipSuccess) rc = fail(ix, NIQKI_E_HIP, std::string("niqki_cluster: ") + hipGetErrorString(e));
    else if (n_clusters) *n_clusters = roots;
  }
  for (auto &e : r.ev) if (e) (void)hipEventDestroy(e);
  return rc;
}

// threshold 0 links every pair, so genome 0 is the only representative: only ITS list is made (at min_score 0 it holds
// every genome with its count), the other genomes start as covered
int derep_run(niqki_index *ix, uint32_t threshold, uint32_t *labels, uint32_t *label_counts, uint32_t *n_reps, int mem) {
  const uint32_t N = ix->n_genomes;
  int rc = build_if_needed(ix);
  if (rc) return rc;
  SelfJoin r;
  r.ix = ix;
  r.who = "niqki_dereplicate";
  r.derep = true;
  r.splits = &ix->derep_splits;
  r.pairs = &ix->derep_pairs;
  r.ms = ix->derep_ms;
  // best[N] (8 bytes), labels[N] and label_counts[N] (device copies of host results), info[4], state[N]
  const bool dev = mem == NIQKI_MEM_DEVICE;
  if ((rc = ensure(ix, ix->ws_parent, (size_t)N * 17 + 16))) return rc;
  r.best = (unsigned long long *)ix->ws_parent.p;
  uint32_t *own_labels = (uint32_t *)(r.best + N), *own_counts = own_labels + N;
  r.info = own_counts + N;   // [0] rounds, [1] [2] flags of a batch's first two rounds, [3] the representative count
  r.state = (uint8_t *)(r.info + 4);
  uint32_t *d_labels = dev ? labels : own_labels, *d_counts = !label_counts ? nullptr : dev ? label_counts : own_counts;
  hipError_t e = hipSuccess;   // (no early return from here on: the events are destroyed below)
  if (ix->prof) for (auto &v : r.ev) if (e == hipSuccess) e = hipEventCreate(&v);
  if (e == hipSuccess) e = hipMemsetAsync(r.best, 0, (size_t)N * 8, ix->stream);
  if (e == hipSuccess) e = hipMemsetAsync(r.info, 0, 16, ix->stream);
  if (e == hipSuccess) e = hipMemsetAsync(r.state, threshold ? nq::kUndecided : nq::kCovered, N, ix->stream);
  if (e == hipSuccess && !threshold) e = hipMemsetAsync(r.state, nq::kUndecided, 1, ix->stream);
  if (e != hipSuccess) rc = fail(ix, NIQKI_E_HIP, std::string("niqki_dereplicate: ") + hipGetErrorString(e));
  if (!rc) rc = self_join_batches(r, threshold ? N : 1);
  if (!rc) {
    uint32_t out[4] = {0, 0, 0, 0};
    e = nq::launch_derep_finish(r.state, r.best, N, d_labels, d_counts, r.info + 3, ix->stream);
    if (e == hipSuccess && !dev) e = hipMemcpyAsync(labels, d_labels, (size_t)N * 4, hipMemcpyDeviceToHost, ix->stream);
    if (e == hipSuccess && !dev && label_counts) e = hipMemcpyAsync(label_counts, d_counts, (size_t)N * 4, hipMemcpyDeviceToHost, ix->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out, r.info, 16, hipMemcpyDeviceToHost, ix->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ix->stream);
    if (e != hipSuccess) rc = fail(ix, NIQKI_E_HIP, std::string("niqki_dereplicate: ") + hipGetErrorString(e));
    else {
      ix->derep_rounds = out[0];
      if (n_reps) *n_reps = out[3];
    }
  }
  for (auto &v : r.ev) if (v) (void)hipEventDestroy(v);
  return rc;
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
  const uint32_t nq = end - begin, N = ix->built_n;
  const uint64_t stride = NIQKI_ROW_STRIDE(N);
  if (mem == NIQKI_MEM_DEVICE) {
    uint16_t *c1, *c2;
    if ((rc = ensure(ix, ix->ws_misc, std::max<size_t>((size_t)nq * ix->d.F * 4, 4)))) return rc;
    if ((rc = count_rows(ix, nq, stride, &c1, &c2))) return rc;
    if ((rc = read_stored(ix, begin, nq, (int32_t *)ix->ws_misc.p))) return rc;
    return query_hits_dev(ix, (const int32_t *)ix->ws_misc.p, nq, c1, c2, stride, (unsigned long long *)hit_off, hit_counts,
                          hit_gids, capacity, false, nullptr);
  }
  // batches of query_batch stored sketches through the host path of niqki_query; hit_off is made of the batches'
  // own offsets, which stay true totals beyond the capacity
  const uint32_t qb = std::max<uint32_t>(ix->query_batch, 1);
  uint64_t base = 0;
  bool overflow = false;
  hit_off[0] = 0;
  for (uint32_t q0 = 0; q0 < nq; q0 += qb) {
    const uint32_t n = std::min(qb, nq - q0);
    if ((rc = ensure(ix, ix->ws_misc, (size_t)n * ix->d.F * 4))) return rc;
    if ((rc = read_stored(ix, begin + q0, n, (int32_t *)ix->ws_misc.p))) return rc;
    const bool room = !overflow && base <= capacity;
    rc = query_to_host(ix, (const int32_t *)ix->ws_misc.p, true, n, hit_off + q0, room ? hit_counts + base : nullptr,
                       room ? hit_gids + base : nullptr, room ? capacity - base : 0);
    if (rc == NIQKI_E_CAPACITY) overflow = true;
    else if (rc) return rc;
    for (uint32_t i = 1; i <= n; ++i) hit_off[q0 + i] += base;
    hit_off[q0] = base;
    base = hit_off[q0 + n];
  }
  return overflow ? NIQKI_E_CAPACITY : NIQKI_OK;
}

int niqki_cluster(niqki_index *ix, uint32_t threshold, uint32_t *labels, uint32_t *n_clusters, int mem) {
  if (!ix || (!labels && ix->n_genomes)) return NIQKI_E_INVALID;
  if (!whole_range(ix)) return fail(ix, NIQKI_E_STATE, "niqki_cluster: a slot-range shard sees partial counts; the self-join needs a whole-range handle");
  NQ_HIP(ix, hipSetDevice(ix->device));
  const uint32_t N = ix->n_genomes;
  ix->cluster_splits = 0;
  ix->cluster_pairs = 0;
  for (double &m : ix->cluster_ms) m = 0;
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
  // the query path with the call's threshold and no top-k; the handle's own values come back whatever happens
  const uint32_t ms = ix->d.min_score, pms = ix->p.min_score, k = ix->p.top_k;
  ix->d.min_score = threshold;
  ix->p.min_score = threshold;
  ix->p.top_k = 0;
  const int rc = cluster_run(ix, labels, n_clusters, mem);
  ix->d.min_score = ms;
  ix->p.min_score = pms;
  ix->p.top_k = k;
  return rc;
}

int niqki_dereplicate(niqki_index *ix, uint32_t threshold, uint32_t *labels, uint32_t *label_counts, uint32_t *n_representatives,
                      int mem) {
  if (!ix || (!labels && ix->n_genomes)) return NIQKI_E_INVALID;
  if (!whole_range(ix)) return fail(ix, NIQKI_E_STATE, "niqki_dereplicate: a slot-range shard sees partial counts; the self-join needs a whole-range handle");
  NQ_HIP(ix, hipSetDevice(ix->device));
  ix->derep_rounds = 0;
  ix->derep_splits = 0;
  ix->derep_pairs = 0;
  for (double &m : ix->derep_ms) m = 0;
  if (ix->n_genomes == 0) {
    if (n_representatives) *n_representatives = 0;
    return NIQKI_OK;
  }
  // the query path with the call's threshold and no top-k; the handle's own values come back whatever happens
  const uint32_t ms = ix->d.min_score, pms = ix->p.min_score, k = ix->p.top_k;
  ix->d.min_score = threshold;
  ix->p.min_score = threshold;
  ix->p.top_k = 0;
  const int rc = derep_run(ix, threshold, labels, label_counts, n_representatives, mem);
  ix->d.min_score = ms;
  ix->p.min_score = pms;
  ix->p.top_k = k;
  return rc;
}

}  // extern "C"
