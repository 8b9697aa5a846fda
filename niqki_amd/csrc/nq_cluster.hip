// nq_cluster.hip -- the self-join of an index: niqki_neighbors_range (the hits of the stored sketches, the sparse form
// of Index::query_range, src/niqki_index.cpp:570-610) and niqki_cluster (single-linkage clusters: the link and flatten
// kernels over the hit lists of the stored sketches) and niqki_dereplicate (greedy representatives in index order: the
// decide, assign and finish kernels over the same hit lists) and niqki_linkage (the single-linkage forest: Boruvka
// rounds over the same hit lists).  DESIGN.md 4.6b, 4.6c, 4.6g.
#include "nq_handle.h"
#include "nq_linkage_key.h"

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
//
// Given genomes (niqki_dereplicate_from).  state[g] = kRep from the start for g < first and only the
// lists of the genomes [first, n) are made; the decide rounds above run unchanged (a given genome is a decided
// representative like any other).  The given representatives have no lists of their own to walk, so after the assign
// step the wave of EVERY query t of the batch takes the hits g < first of t's own list: counts are symmetric, so
// count(t, g) << 32 | ~g is the offer g would have made.  The wave reduces its offers to their maximum and lane 0
// issues the one agent-scope 64-bit atomicMax on best[t] -- the same operation, on the same word, as the offers of
// the batch's new representatives; best[] is only ever written by such atomics and read by the finish kernel of a
// later launch.  An offer to a t that turned out a representative is ignored by the finish kernel like any other.

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

// the offers of the given representatives g < first to the queries of the batch, read off the queries' own lists
__global__ __launch_bounds__(kLinkBlock) void derep_given_kernel(unsigned long long *best, uint32_t n, uint32_t first,
                                                                 const unsigned long long *hit_off, const uint32_t *hit_counts,
                                                                 const uint32_t *hit_gids, uint32_t t0, uint32_t nq) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t q = blockIdx.x * (kLinkBlock / 64) + (threadIdx.x >> 6);   // wave-uniform
  if (q >= nq) return;
  const uint32_t t = t0 + q;
  if (t >= n) return;
  const unsigned long long lo = hit_off[q], hi = hit_off[q + 1];
  unsigned long long v = 0;
  for (unsigned long long i = lo + lane; i < hi; i += 64) {
    const uint32_t g = hit_gids[i];
    if (g >= first || g == t) continue;
    const unsigned long long o = ((unsigned long long)hit_counts[i] << 32) | (uint32_t)~g;
    v = o > v ? o : v;
  }
  for (int d = 32; d; d >>= 1) {
    const unsigned long long o = (unsigned long long)__shfl_xor((long long)v, d);
    v = o > v ? o : v;
  }
  if (lane == 0 && v) __hip_atomic_fetch_max(best + t, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
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

// ---- single-linkage forest on the device (niqki_linkage) -------------------------------------------
// The maximum spanning forest of the co-occurrence graph under the edge order of nq_linkage_key.h IS the complete
// single-linkage hierarchy.  MST(A u B) = MST(MST(A) u B): an edge once dropped is the last of a cycle and stays
// dropped.  So the device keeps a forest of at most n - 1 keys, and per batch of the self-join computes the forest of
// (old forest u the batch's pairs g < t) into the other half of a double buffer, by Boruvka rounds:
//   offer   every edge whose endpoints lie in different components offers its key to both components with a 64-bit
//           atomic maximum on best[component].  Two launches: the old forest, one thread per edge; the hit lists, one
//           wavefront per query t.
//   hook    every component c with an offer takes the component at the other end of its best edge as its parent and
//           records the edge into the new forest.  The order is strict, so the picks of a round can only cycle as a
//           mutual pick of the SAME edge (a longer cycle would need strictly ascending keys all the way round; two
//           components that pick each other through different edges would each hold both edges and pick the larger).
//           In a mutual pick the smaller component id stays root and the other one records the edge: once.
//   jump    comp[g] = the root of g's chain, best[g] = 0.
// comp[g] names g's component by its root; between rounds every comp[g] is a root.  A round whose hook kernel found no
// offer ends the batch: the `any` words (one per round, zeroed by the init kernel) carry that to the launches of the
// following rounds, which return at once; the host enqueues ceil(log2 n) + 1 rounds -- the components with an offer at
// least halve per round -- and never synchronises.
//
// Coherence.  The atomics on best[] execute at the memory side on the real value.  Everything else is read in a LATER
// launch than it was written (stream order makes it visible), with three exceptions, all harmless:
//   * the relaxed agent-scope load of best[] before an offer: best[] only grows within a round, so a stale value costs
//     a needless atomic and never loses an offer;
//   * the hook kernel reads comp[lo] / comp[hi] of its best edge while other threads of the same launch store new
//     parents.  A new parent is stored with bit 31 set (ids have 23 bits), and only a ROOT x, comp[x] == x, is ever
//     given one, so a flagged value decodes to x itself: fresh or stale, the reader gets the value of before the launch;
//   * the jump kernel walks chains while other threads store roots.  A word holds its old value (a flagged parent, or
//     the root of the round before, itself flagged or final) or the final root; every one of them leads to the final
//     root of the chain, the only unflagged x with comp[x] == x on it.  These accesses are agent-scope relaxed atomics
//     like those of the link kernel; nothing relies on their being fresh.

constexpr uint32_t kHookFlag = 0x80000000u;
// (info: [0] old forest size, [1] new forest size, [2] most rounds, [3] error; from kLinkageInfoHead on the `any` words)

__device__ __forceinline__ unsigned long long best_load(const unsigned long long *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void best_offer(unsigned long long *best, uint32_t c, unsigned long long key) {
  if (key > best_load(best + c)) __hip_atomic_fetch_max(best + c, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void linkage_init_kernel(uint32_t *comp, unsigned long long *best, uint32_t n, uint32_t *info, uint32_t rounds) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g < n) {
    comp[g] = g;
    best[g] = 0;
  }
  if (g == 0) info[1] = 0;
  if (g < rounds) info[kLinkageInfoHead + g] = 0;   // (the launch has at least 256 threads)
}

// go: the `any` word of the round before (null in the first round)
__global__ void linkage_offer_forest_kernel(const uint32_t *comp, unsigned long long *best, const unsigned long long *forest,
                                            const uint32_t *info, uint32_t n, const uint32_t *go) {
  if (go && !*go) return;
  const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= info[0] || e >= n) return;
  const unsigned long long key = forest[e];
  const uint32_t lo = linkage_lo(key), hi = linkage_hi(key);
  if (lo >= n || hi >= n) return;
  const uint32_t cl = comp[lo], ch = comp[hi];
  if (cl == ch) return;
  best_offer(best, cl, key);
  best_offer(best, ch, key);
}

__global__ __launch_bounds__(kLinkBlock) void linkage_offer_hits_kernel(const uint32_t *comp, unsigned long long *best, uint32_t n,
                                                                        const unsigned long long *hit_off, const uint32_t *hit_counts,
                                                                        const uint32_t *hit_gids, uint32_t t0, uint32_t nq,
                                                                        const uint32_t *go) {
  if (go && !*go) return;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t q = blockIdx.x * (kLinkBlock / 64) + (threadIdx.x >> 6);   // wave-uniform
  if (q >= nq) return;
  const uint32_t t = t0 + q;
  if (t >= n) return;
  const unsigned long long lo = hit_off[q], hi = hit_off[q + 1];
  const uint32_t ct = comp[t];
  unsigned long long mine = 0;
  for (unsigned long long i = lo + lane; i < hi; i += 64) {
    // the pair (t, g) with g > t is query g's, g == t is no edge
    const uint32_t g = hit_gids[i];
    if (g >= t) continue;
    const uint32_t cg = comp[g];
    if (cg == ct) continue;
    const unsigned long long key = linkage_pack(hit_counts[i], g, t);
    mine = key > mine ? key : mine;
    best_offer(best, cg, key);
  }
  for (int d = 32; d; d >>= 1) {
    const unsigned long long o = (unsigned long long)__shfl_xor((long long)mine, d);
    mine = o > mine ? o : mine;
  }
  if (lane == 0 && mine) best_offer(best, ct, mine);
}

// mine: the `any` word of this round
__global__ void linkage_hook_kernel(uint32_t *comp, const unsigned long long *best, uint32_t n, unsigned long long *forest,
                                    uint32_t *info, const uint32_t *go, uint32_t *mine) {
  if (go && !*go) return;
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  unsigned long long key = 0;
  bool hooks = false;
  if (c < n) {
    key = best[c];   // (nonzero only where c is a root: offers go to comp[] values)
    if (key) {
      const uint32_t lo = linkage_lo(key), hi = linkage_hi(key);
      uint32_t cl = uf_load(comp + lo), ch = uf_load(comp + hi);
      if (cl & kHookFlag) cl = lo;   // hooked in this launch: lo was its own root before it
      if (ch & kHookFlag) ch = hi;
      const uint32_t other = cl == c ? ch : cl;
      hooks = !(best[other] == key && c < other);   // a mutual pick: the smaller id stays root
      if (hooks) __hip_atomic_store(comp + c, other | kHookFlag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  if (__any(key != 0) && (threadIdx.x & 63u) == 0) *mine = 1;   // (every wave with an offer stores the same word)
  // the recorded edges of a wavefront take consecutive places: one atomic a wavefront
  const unsigned long long m = __ballot(hooks);
  if (!m) return;
  const uint32_t lane = threadIdx.x & 63u;
  const int leader = __ffsll((long long)m) - 1;
  uint32_t base = 0;
  if ((int)lane == leader) base = atomicAdd(info + 1, (uint32_t)__popcll(m));
  base = (uint32_t)__shfl((int)base, leader);
  if (hooks) {
    const uint32_t at = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    if (at < n) forest[at] = key;
    else info[3] = 1;   // (a forest has fewer than n edges)
  }
}

__global__ void linkage_jump_kernel(uint32_t *comp, unsigned long long *best, uint32_t n, const uint32_t *go) {
  if (go && !*go) return;
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n) return;
  best[g] = 0;
  uint32_t r = g;
  for (;;) {
    const uint32_t v = uf_load(comp + r);
    if (v == r) break;
    r = v & ~kHookFlag;
  }
  if (r != g) __hip_atomic_store(comp + g, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the batch is through: the new forest becomes the old one (the host swaps the buffers), the rounds that hooked
__global__ void linkage_end_kernel(uint32_t *info, uint32_t rounds) {
  uint32_t r = 0;
  for (uint32_t k = 0; k < rounds; ++k) r += info[kLinkageInfoHead + k] ? 1u : 0u;
  if (rounds && info[kLinkageInfoHead + rounds - 1]) info[3] = 1;   // the last round still had offers
  if (r > info[2]) info[2] = r;
  info[0] = info[1];
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

hipError_t launch_derep_given(unsigned long long *best, uint32_t n, uint32_t first, const unsigned long long *hit_off,
                              const uint32_t *hit_counts, const uint32_t *hit_gids, uint32_t t0, uint32_t nq, hipStream_t stream) {
  if (!nq || !n || !first) return hipSuccess;
  const uint32_t per = kLinkBlock / 64;
  hipLaunchKernelGGL(derep_given_kernel, dim3((nq + per - 1) / per), dim3(kLinkBlock), 0, stream, best, n, first, hit_off, hit_counts,
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

uint32_t linkage_rounds(uint32_t n) {
  uint32_t lg = 0;
  while ((1ull << lg) < n) lg += 1;
  return lg + 1;
}

hipError_t launch_linkage_batch(uint32_t *comp, unsigned long long *best, const unsigned long long *forest_old,
                                unsigned long long *forest_new, uint32_t *info, uint32_t n, const unsigned long long *hit_off,
                                const uint32_t *hit_counts, const uint32_t *hit_gids, uint32_t t0, uint32_t nq, hipStream_t stream) {
  if (!n) return hipSuccess;
  const uint32_t rounds = linkage_rounds(n), per = kLinkBlock / 64;
  const dim3 over_n((n + 255) / 256), block(256);
  hipLaunchKernelGGL(linkage_init_kernel, over_n, block, 0, stream, comp, best, n, info, rounds);
  for (uint32_t r = 0; r < rounds; ++r) {
    const uint32_t *go = r ? info + kLinkageInfoHead + r - 1 : nullptr;
    hipLaunchKernelGGL(linkage_offer_forest_kernel, over_n, block, 0, stream, comp, best, forest_old, info, n, go);
    if (nq)
      hipLaunchKernelGGL(linkage_offer_hits_kernel, dim3((nq + per - 1) / per), dim3(kLinkBlock), 0, stream, comp, best, n, hit_off,
                         hit_counts, hit_gids, t0, nq, go);
    hipLaunchKernelGGL(linkage_hook_kernel, over_n, block, 0, stream, comp, best, n, forest_new, info, go, info + kLinkageInfoHead + r);
    hipLaunchKernelGGL(linkage_jump_kernel, over_n, block, 0, stream, comp, best, n, go);
  }
  hipLaunchKernelGGL(linkage_end_kernel, dim3(1), dim3(1), 0, stream, info, rounds);
  return hipGetLastError();
}

}  // namespace nq
