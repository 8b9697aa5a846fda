// nq_group.hip -- one index sharded by sketch-slot range over several GPUs (include/niqki_hip.h,
// niqki_group_*).  Rank r of G owns slots [F*r/G, F*(r+1)/G) of EVERY genome; the hit count of a
// genome is a sum over slots (src/niqki_index.cpp:652-661 runs over all of them), so a query batch
// needs exactly one exchange of partial results:
//
//   1. every rank has sketched its share of the batch (`per` queries)            no communication
//   2. slice exchange: a rank needs only ITS slots of every query -> one all-to-all of int16
//      slices (2*F/G bytes per query and peer)                                    slice_pack / unpack
//   3. gather over the local slots for ALL G*per queries                          gather_kernel
//        dense   into u16 counter rows, one per query
//        sparse  without counter rows: per query the kernel leaves the CANDIDATES (genomes whose
//                partial count reaches thr = ceil(min_score / G): ids only, at most cand_cap kept)
//                and the SURVIVORS (partial count >= max(1, thr / 2): {id, count}, at most surv_cap)
//   4. cross-shard sum of the partial counts, scattered by query:
//        dense   reduce-scatter of the u16 counters as packed pairs in u32 words -- a count never
//                exceeds F <= 2^15, so the halves cannot carry (RCCL has no 16-bit integer type)
//        sparse  a genome whose summed count reaches min_score has a partial count of at least thr
//                on some rank: ranks all-gather their candidate ids with the list sizes (one blob
//                per rank, cand_blob_ints), each looks its own partial counts of the union up --
//                in its survivor list, or, for an id that is weak here, counted exactly from the
//                sketch store (surv_lookup_kernel) -- and these values are reduce-scattered.
//                Exact; a candidate or survivor list of any rank that holds more than its capacity
//                (blob_overflow_kernel: the same words on every rank) makes every rank redo the
//                batch densely in niqki_group_query_end.
//   5. every rank thresholds + orders the hits of its own `per` queries: from counter rows
//      (hits_* kernels, nq_hits.hip) or, sparse, from the candidates' sums alone -- distinct ids,
//      sorted in LDS, written behind a prefix sum (cand_hits_kernel, _scan_kernel, _write_kernel)
//
// HOW the bytes of steps 2 and 4 cross ranks (rccl / local / ipc) is nq_group_transport.hip, reached only through
// namespace nqg of nq_group.h: reserve, before_write, all_to_all, all_gather, reduce_scatter_u32.
#include "nq_group.h"

#include <algorithm>
#include <cstring>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

namespace nq {

// ---- exchange kernels ----------------------------------------------------------------------
// first slot of rank r (niqki_group_slot_range)
__host__ __device__ inline uint32_t cut(uint32_t F, uint32_t r, uint32_t G) { return (uint32_t)(((uint64_t)F * r) / G); }

// [per][F] int32 sketches -> [G][per][w_max] int16 slices (slot slice of destination g; cells that
// are empty or outside [0, R) -- never indexed or queried, src/niqki_index.cpp:364,:654 -- travel as -1)
// (dst_stride: int16 cells between two destinations' parts, >= per * w_max)
__global__ __launch_bounds__(256) void slice_pack_kernel(const int32_t *sk, uint32_t per, uint32_t F, uint32_t R, uint32_t G,
                                                        uint32_t w_max, int16_t *out, uint64_t dst_stride) {
  const uint32_t q = blockIdx.x, g = blockIdx.y;
  const uint32_t b = cut(F, g, G), w = cut(F, g + 1, G) - b;
  const int32_t *row = sk + (uint64_t)q * F + b;
  int16_t *dst = out + (uint64_t)g * dst_stride + (uint64_t)q * w_max;
  for (uint32_t j = threadIdx.x; j < w_max; j += 256) {
    int32_t x = j < w ? row[j] : -1;
    dst[j] = (x >= 0 && (uint32_t)x < R) ? (int16_t)x : (int16_t)-1;
  }
}

// [nq][w_max] int16 slices of MY slots -> [nq][f_local] int32 sketch rows for the query kernels
// (row q = source rank q / per, its query q % per; src_stride: int16 cells between two sources' parts)
__global__ __launch_bounds__(256) void slice_unpack_kernel(const int16_t *in, uint32_t w_max, uint32_t f_local, int32_t *out, uint32_t per,
                                                          uint64_t src_stride) {
  const uint32_t q = blockIdx.x;
  const int16_t *src = in + (uint64_t)(q / per) * src_stride + (uint64_t)(q % per) * w_max;
  for (uint32_t j = threadIdx.x; j < f_local; j += 256) out[(uint64_t)q * f_local + j] = src[j];
}

// A rank's candidates travel as one blob: nq lists of C ids, the nq list sizes, the nq sizes of its survivor
// lists (one all-gather).
__host__ __device__ inline uint64_t cand_blob_ints(uint32_t nq, uint32_t C) { return (uint64_t)nq * C + 2ull * nq; }

// ---- sparse exchange without counter rows ---------------------------------------------------------
// The ids a query's ranks proposed, m per query: id(q, i) = p[(i / C) * blob + q * C + i % C]
// (the all-gathered blobs: C ids per rank; a flat [nq][m] array: C = m).
struct IdView {
  const int32_t *p;
  uint64_t blob;
  uint32_t C;
  __device__ int32_t at(uint32_t q, uint32_t i) const { return p[(uint64_t)(i / C) * blob + (uint64_t)q * C + i % C]; }
};
__device__ inline uint32_t id_hash(uint32_t id) { return (id * 2654435761u) >> 7; }
constexpr uint32_t kSurvMax = 4096;       // survivors per query a lookup can index (LDS table of 2x)
constexpr uint32_t kCandMax = 4096;       // ids per query cand_hits_kernel can order in LDS

// mine[q][i] = this shard's partial count of id(q, i) (0 for -1): from the shard's survivor list of the
// query (every genome with a partial count >= surv_thr, indexed here by an LDS hash table) or, for an id
// that is not among them -- another rank's candidate that is weak here --, counted exactly as the slots
// in which the genome's stored sketch equals the query's (the identity behind the matrix path, DESIGN.md
// 4.6): f_local strided 2-byte reads per such id, rare by construction.  A survivor list that holds more than
// SC entries is read up to SC (the rest of its ids are counted from the store like any other): the overflow itself
// is blob_overflow_kernel's to report.
// CT: uint16_t, or uint32_t where the cross-shard sums can pass 2^16 - 1 (S = 16)
template <typename CT>
__global__ __launch_bounds__(256) void surv_lookup_kernel(const int2 *surv, const int32_t *surv_n, uint32_t SC, uint32_t T, uint32_t m,
                                                         IdView ids, const int32_t *sk, uint32_t q_stride, uint32_t q_off,
                                                         uint32_t f_local, const uint16_t *store, uint64_t store_cap, uint32_t R,
                                                         CT *mine) {
  extern __shared__ __align__(8) int lds_tab[];
  int2 *tab = (int2 *)lds_tab;                  // T x {id, count}
  uint32_t *missing = (uint32_t *)(tab + T);    // one bit per position i < m <= kCandMax
  __shared__ uint32_t acc;
  const uint32_t q = blockIdx.x, tid = threadIdx.x, mw = (m + 31) / 32;
  for (uint32_t i = tid; i < T; i += 256) tab[i] = make_int2(-1, 0);
  for (uint32_t i = tid; i < mw; i += 256) missing[i] = 0;
  __syncthreads();
  const uint32_t ns_all = (uint32_t)surv_n[q], ns = ns_all < SC ? ns_all : SC;
  for (uint32_t i = tid; i < ns; i += 256) {
    const int2 e = surv[(uint64_t)q * SC + i];
    uint32_t h = id_hash((uint32_t)e.x) & (T - 1);
    while (atomicCAS(&tab[h].x, -1, e.x) != -1) h = (h + 1) & (T - 1);   // (ids of one list are distinct)
    tab[h].y = e.y;
  }
  __syncthreads();
  for (uint32_t i = tid; i < m; i += 256) {
    const int32_t id = ids.at(q, i);
    uint32_t c = 0;
    if (id >= 0) {
      uint32_t h = id_hash((uint32_t)id) & (T - 1);
      bool found = false;
      for (int2 e = tab[h]; e.x != -1; h = (h + 1) & (T - 1), e = tab[h])
        if (e.x == id) { c = (uint32_t)e.y; found = true; break; }
      if (!found) atomicOr(&missing[i >> 5], 1u << (i & 31));
    }
    mine[(uint64_t)q * m + i] = (CT)c;
  }
  __syncthreads();
  // ids this shard holds no survivor entry for: counted exactly from the sketch store, one after the other
  const int32_t *row = sk + (uint64_t)q * q_stride + q_off;
  for (uint32_t w = 0; w < mw; ++w) {
    for (uint32_t bits = missing[w]; bits; bits &= bits - 1) {   // (uniform: every thread reads the same word)
      const uint32_t i = w * 32 + (uint32_t)__builtin_ctz(bits);
      const uint32_t id = (uint32_t)ids.at(q, i);
      if (tid == 0) acc = 0;
      __syncthreads();
      uint32_t c = 0;
      for (uint32_t s_ = tid; s_ < f_local; s_ += 256) {
        const int32_t fp = row[s_];
        c += (fp >= 0 && (uint32_t)fp < R && store[(uint64_t)s_ * store_cap + id] == (uint16_t)fp) ? 1u : 0u;
      }
      if (c) atomicAdd(&acc, c);
      __syncthreads();
      if (tid == 0) mine[(uint64_t)q * m + i] = (CT)acc;
      __syncthreads();
    }
  }
}

// The hits of one query from its candidates alone: ids id(first_q + ql, i) with summed counts tot[ql][i]
// (the same id may appear under several ranks, with the same sum): distinct ids whose sum reaches min_score,
// ordered like greater<pair<count, gid>> (src/niqki_index.cpp:685), as 64-bit keys count << 32 | gid.
template <typename CT>
__global__ __launch_bounds__(256) void cand_hits_kernel(const CT *tot, uint32_t first_q, uint32_t m, IdView ids, uint32_t min_score,
                                                       uint32_t T, uint32_t P, unsigned long long *keys, uint32_t *n_out) {
  extern __shared__ __align__(8) int lds_tab[];
  unsigned long long *list = (unsigned long long *)lds_tab;   // P keys
  int32_t *set = (int32_t *)(list + P);                        // T ids
  __shared__ uint32_t cnt;
  const uint32_t ql = blockIdx.x, q = first_q + ql, tid = threadIdx.x;
  for (uint32_t i = tid; i < T; i += 256) set[i] = -1;
  for (uint32_t i = tid; i < P; i += 256) list[i] = 0ull;
  if (tid == 0) cnt = 0;
  __syncthreads();
  for (uint32_t i = tid; i < m; i += 256) {
    const int32_t id = ids.at(q, i);
    if (id < 0) continue;
    uint32_t h = id_hash((uint32_t)id) & (T - 1);
    for (;;) {
      const int32_t prev = atomicCAS(&set[h], -1, id);
      if (prev == -1) {   // first of its copies
        const uint32_t c = tot[(uint64_t)ql * m + i];
        if (c >= min_score) list[atomicAdd(&cnt, 1u)] = ((unsigned long long)c << 32) | (uint32_t)id;
        break;
      }
      if (prev == id) break;
      h = (h + 1) & (T - 1);
    }
  }
  __syncthreads();
  const uint32_t n = cnt;
  // bitonic sort, descending (empty places hold 0 and end up last; a real key is never 0: count >= 1 unless
  // min_score is 0, and then gid 0 with count 0 keeps its place among the n first by the write below)
  for (uint32_t k = 2; k <= P; k <<= 1)
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      for (uint32_t i = tid; i < P; i += 256) {
        const uint32_t l = i ^ j;
        if (l > i) {
          const unsigned long long x = list[i], y = list[l];
          const bool desc = (i & k) == 0;
          if ((x < y) == desc) { list[i] = y; list[l] = x; }
        }
      }
      __syncthreads();
    }
  for (uint32_t i = tid; i < n; i += 256) keys[(uint64_t)ql * m + i] = list[i];
  if (tid == 0) n_out[ql] = n;
}

// S = 16 groups, dense exchange: a shard's counters (<= 2^15 each) as u32 words for the sum, and the sums
// (<= 2^16) back as two u16 planes lo = min(sum, 2^15), hi = sum - lo for the hit kernels' 32-bit form
__global__ __launch_bounds__(256) void widen_rows_kernel(const uint16_t *in, uint64_t n, uint32_t *out) {
  const uint64_t step = (uint64_t)gridDim.x * 256;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += step) out[i] = in[i];
}
__global__ __launch_bounds__(256) void split_sums_kernel(const uint32_t *in, uint64_t n, uint16_t *lo, uint16_t *hi) {
  const uint64_t step = (uint64_t)gridDim.x * 256;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += step) {
    const uint32_t v = in[i], l = v < 32768u ? v : 32768u;
    lo[i] = (uint16_t)l;
    hi[i] = (uint16_t)(v - l);
  }
}

// flag |= some rank's candidate or survivor list of some query holds more than its capacity
__global__ __launch_bounds__(256) void blob_overflow_kernel(const int32_t *cand_all, uint64_t blob, uint32_t nq, uint32_t G, uint32_t C,
                                                           uint32_t SC, uint32_t *flag) {
  const uint32_t q = blockIdx.x * 256 + threadIdx.x;
  if (q >= nq) return;
  bool over = false;
  for (uint32_t g = 0; g < G; ++g) {
    const int32_t *tail = cand_all + g * blob + (uint64_t)nq * C;
    over |= (uint32_t)tail[q] > C || (uint32_t)tail[nq + q] > SC;
  }
  if (over) atomicOr(flag, 1u);
}

// hit_off[0..nq] = exclusive prefix of n (one workgroup)
__global__ __launch_bounds__(1024) void cand_hits_scan_kernel(const uint32_t *n, uint32_t nq, unsigned long long *hit_off) {
  __shared__ unsigned long long part[1024];
  const uint32_t tid = threadIdx.x, per_t = (nq + 1023) / 1024;
  unsigned long long s = 0;
  for (uint32_t i = tid * per_t; i < (tid + 1) * per_t && i < nq; ++i) s += n[i];
  part[tid] = s;
  __syncthreads();
  for (uint32_t d = 1; d < 1024; d <<= 1) {
    const unsigned long long v = tid >= d ? part[tid - d] : 0ull;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  unsigned long long run = tid ? part[tid - 1] : 0ull;
  for (uint32_t i = tid * per_t; i < (tid + 1) * per_t && i < nq; ++i) { hit_off[i] = run; run += n[i]; }
  if (tid == 1023) hit_off[nq] = part[1023];
}
__global__ __launch_bounds__(256) void cand_hits_write_kernel(const unsigned long long *keys, const uint32_t *n, uint32_t m,
                                                             const unsigned long long *hit_off, uint32_t *hc, uint32_t *hg,
                                                             unsigned long long capacity) {
  const uint32_t ql = blockIdx.x;
  const unsigned long long base = hit_off[ql];
  for (uint32_t i = threadIdx.x; i < n[ql]; i += 256) {
    if (base + i >= capacity) break;
    const unsigned long long k = keys[(uint64_t)ql * m + i];
    hc[base + i] = (uint32_t)(k >> 32);
    hg[base + i] = (uint32_t)k;
  }
}

// hc / hg[0 .. min(*total, capacity)) = the head of the lists in staging buffers (total: hit_off[per], on the device)
__global__ __launch_bounds__(256) void hits_head_kernel(const unsigned long long *total, unsigned long long capacity, const uint32_t *sc,
                                                       const uint32_t *sg, uint32_t *hc, uint32_t *hg) {
  const unsigned long long n = *total < capacity ? *total : capacity, step = (unsigned long long)gridDim.x * 256;
  for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n; i += step) {
    hc[i] = sc[i];
    hg[i] = sg[i];
  }
}

}  // namespace nq

namespace {

using nqi::Buf;
using Ws = niqki_group::Ws;

// f(l, shard, workspace) for every local rank, with the rank's device current; the first failure ends the walk
template <typename F>
int each_rank(niqki_group *g, F &&f) {
  for (uint32_t l = 0; l < g->n_local; ++l) {
    NQ_GH(g, hipSetDevice(g->sh[l]->device));
    const int rc = f(l, g->sh[l], g->ws[l]);
    if (rc) return rc;
  }
  return NIQKI_OK;
}

// bytes of one destination's slices of `per` queries (16-byte granular for the pull kernel)
size_t slice_bytes(uint32_t per, uint32_t w_max) { return (((size_t)per * w_max * 2) + 15) & ~(size_t)15; }
// option "exchange" as a batch takes it: top-k batches are dense (the sparse candidate exchange does not know the
// boundary; the dense form ends in nqi::hits_dev on the summed rows, which does)
int exchange_of(const niqki_group *g) { return g->sh[0]->p.top_k ? 2 : g->exchange; }
// the decisions and sizes of one query batch (niqki_group_plan_batch: also what the CPU test of the protocol uses)
void plan_batch(uint32_t G, uint32_t S, uint32_t min_score, int exchange, uint32_t per, uint32_t N, uint32_t C, niqki_group_plan *o) {
  const uint32_t F = 1u << S, nq_ = G * per;
  bool sparse = exchange == 1 || (exchange == 0 && min_score >= 4 * G);
  if (min_score < G || N == 0) sparse = false;                    // ceil(min_score / G) must be >= 1
  if ((uint64_t)G * C > nq::kCandMax) sparse = false;             // (cand_hits_kernel orders a query's candidates in LDS)
  o->sparse = sparse ? 1u : 0u;
  o->cand_threshold = (min_score + G - 1) / G;
  o->surv_threshold = std::max(1u, o->cand_threshold / 2);
  o->slice_slots = (F + G - 1) / G;
  o->slice_bytes = slice_bytes(per, o->slice_slots);
  o->cand_blob_bytes = (((size_t)nq::cand_blob_ints(nq_, C) * 4) + 15) & ~(size_t)15;
  o->row_stride = NIQKI_ROW_STRIDE(N);
  const bool wide = S > 15;                                       // cross-shard sums reach 2^16: they travel as u32
  o->sum_words = sparse ? (wide ? (uint64_t)per * G * C : (uint64_t)per * G * C / 2)
                        : (wide ? (uint64_t)per * o->row_stride : (uint64_t)per * (o->row_stride / 2));
}
// ... of a batch of this group: every size below comes from here
niqki_group_plan plan_of(const niqki_group *g, int exchange, uint32_t per, uint32_t N) {
  niqki_group_plan plan;
  plan_batch(g->world, g->sh[0]->d.S, g->sh[0]->d.min_score, exchange, per, N, g->cand_cap, &plan);
  return plan;
}

// exchange buffer sizes of a batch (ipc: made before the first of them is used); query: counts travel too
int reserve_batch(niqki_group *g, const niqki_group_plan &plan, uint32_t per, bool query) {
  size_t need[kXbufs] = {};
  need[kSend] = plan.slice_bytes * g->world;
  if (query && plan.sparse) {   // no counter rows (they are made only if a batch has to be redone densely)
    need[kCand] = plan.cand_blob_bytes;
    need[kMine] = (size_t)plan.sum_words * 4 * g->world;   // (one part of sum_words u32 words per rank)
  } else if (query) {
    need[kCounts] = std::max<size_t>((size_t)g->world * per * plan.row_stride * (g->wide ? 4 : 2), 4);
  }
  return nqg::reserve(g, need);
}

// steps 1-3 shared by insert and query: local sketches -> compact rows of all world*per sketches
// restricted to each rank's slots (ws.allsk, stride f_local)
int exchange_slices(niqki_group *g, const niqki_group_plan &plan, const int32_t *const *local_sketches, uint32_t per) {
  const uint32_t G = g->world, F = g->sh[0]->d.F, R = g->sh[0]->d.R, w_max = plan.slice_slots;
  const size_t bytes = plan.slice_bytes;
  int rc = nqg::before_write(g, kSend);
  if (!rc) rc = each_rank(g, [&](uint32_t l, niqki_index *ix, Ws &w) -> int {
    NQ_G(g, l, nqi::ensure(ix, w.xbuf[kSend], bytes * G));
    NQ_G(g, l, nqi::ensure(ix, w.recv, bytes * G));
    nqi::Span sp(ix, NIQKI_KC_EXCHANGE);
    hipLaunchKernelGGL(nq::slice_pack_kernel, dim3(per, G), dim3(256), 0, ix->stream, local_sketches[l], per, F, R, G, w_max,
                       (int16_t *)w.xbuf[kSend].p, (uint64_t)(bytes / 2));
    NQ_GH(g, hipGetLastError());
    return NIQKI_OK;
  });
  if (rc) return rc;
  {
    nqi::Span sp(g->sh[0], NIQKI_KC_EXCHANGE);
    if ((rc = nqg::all_to_all(g, kSend, &Ws::recv, bytes))) return rc;
  }
  return each_rank(g, [&](uint32_t l, niqki_index *ix, Ws &w) -> int {
    const uint32_t f_local = ix->d.slot_end - ix->d.slot_begin;
    NQ_G(g, l, nqi::ensure(ix, w.allsk, (size_t)G * per * f_local * 4));
    nqi::Span sp(ix, NIQKI_KC_EXCHANGE);
    hipLaunchKernelGGL(nq::slice_unpack_kernel, dim3(G * per), dim3(256), 0, ix->stream, (const int16_t *)w.recv.p, w_max,
                       f_local, (int32_t *)w.allsk.p, per, (uint64_t)(bytes / 2));
    NQ_GH(g, hipGetLastError());
    return NIQKI_OK;
  });
}

}  // namespace

extern "C" {

void niqki_group_slot_range(uint32_t rank, uint32_t world, uint32_t S, uint32_t *slot_begin, uint32_t *slot_end) {
  const uint32_t F = 1u << S;
  if (slot_begin) *slot_begin = nq::cut(F, rank, world);
  if (slot_end) *slot_end = nq::cut(F, rank + 1, world);
}

int niqki_group_new_id(uint8_t id[NIQKI_GROUP_ID_BYTES]) {
  if (!id) return NIQKI_E_INVALID;
  return nqg::new_id(id);
}

int niqki_group_create(niqki_index *const *shards, uint32_t n_local, uint32_t first_rank, uint32_t world, const uint8_t *id,
                       niqki_group **out) {
  if (!shards || !out || n_local == 0 || world == 0 || world > kMaxWorld || first_rank + n_local > world) return NIQKI_E_INVALID;
  *out = nullptr;
  niqki_group *g = new (std::nothrow) niqki_group();
  if (!g) return NIQKI_E_NOMEM;
  g->world = world; g->n_local = n_local; g->first = first_rank;
  g->wide = shards[0] && shards[0]->d.S > 15;
  g->sh.assign(shards, shards + n_local);
  g->ws.resize(n_local);
  auto bail = [&](int code, const std::string &why) {
    if (g->sh[0]) g->sh[0]->err = why;   // readable through niqki_last_error(shards[0])
    niqki_group_destroy(g);
    return code;
  };
  const uint32_t S = shards[0] ? shards[0]->d.S : 0;
  bool shared_device = false;
  for (uint32_t l = 0; l < n_local; ++l) {
    niqki_index *ix = shards[l];
    if (!ix) { delete g; return NIQKI_E_INVALID; }
    uint32_t b, e;
    niqki_group_slot_range(first_rank + l, world, S, &b, &e);
    if (ix->d.S != S || ix->d.slot_begin != b || ix->d.slot_end != e)
      return bail(NIQKI_E_INVALID, "shard " + std::to_string(first_rank + l) + " must own slots [" + std::to_string(b) + ", " +
                                       std::to_string(e) + ") (niqki_group_slot_range)");
    if (ix->resident_bytes) return bail(NIQKI_E_INVALID, "a paged index (resident_bytes) cannot be a shard of a group");
    if (ix->d.S > 15 && world < 2)
      return bail(NIQKI_E_INVALID, "an S = 16 group needs at least two shards (a shard counts at most 2^15 slots in u16)");
    if (ix->d.K != shards[0]->d.K || ix->d.W != shards[0]->d.W || ix->d.min_score != shards[0]->d.min_score ||
        ix->p.top_k != shards[0]->p.top_k || ix->n_genomes != shards[0]->n_genomes)
      return bail(NIQKI_E_INVALID, "the shards of a group must agree in K, W, min_score, top_k and genome count");
    for (uint32_t m = 0; m < l; ++m) shared_device |= shards[m]->device == ix->device;
  }
  if (hipSetDevice(shards[0]->device) != hipSuccess || hipHostMalloc((void **)&g->host_flags, 64, hipHostMallocDefault) != hipSuccess ||
      hipEventCreateWithFlags(&g->ev_flags, hipEventDisableTiming) != hipSuccess)
    return bail(NIQKI_E_HIP, "pinned flag words / event could not be made");
  g->host_flags[0] = g->host_flags[1] = 0;
  const int rc = nqg::open(g, id, shared_device);
  if (rc) return bail(rc, g->err);
  *out = g;
  return NIQKI_OK;
}

void niqki_group_destroy(niqki_group *g) {
  if (!g) return;
  for (uint32_t l = 0; l < g->n_local && l < g->ws.size(); ++l) {
    if (g->sh[l]) {
      (void)hipSetDevice(g->sh[l]->device);
      (void)hipStreamSynchronize(g->sh[l]->stream);
    }
  }
  nqg::close(g);   // (ipc: drops the views of its arena from ws[0].xbuf)
  for (auto &w : g->ws)
    for (Buf *b : w.all())
      if (b->p) (void)hipFree(b->p);
  if (g->host_flags) (void)hipHostFree(g->host_flags);
  if (g->ev_flags) (void)hipEventDestroy(g->ev_flags);
  delete g;
}

const char *niqki_group_last_error(const niqki_group *g) { return g ? g->err.c_str() : ""; }

int niqki_group_plan_batch(uint32_t world, uint32_t S, uint32_t min_score, int exchange_option, uint32_t per, uint32_t n_genomes,
                           uint32_t cand_cap, niqki_group_plan *out) {
  if (!out || world == 0 || world > kMaxWorld || S == 0 || S > 16 || exchange_option < 0 || exchange_option > 2) return NIQKI_E_INVALID;
  plan_batch(world, S, min_score, exchange_option, per, n_genomes, cand_cap, out);
  return NIQKI_OK;
}

int niqki_group_set_option(niqki_group *g, const char *key, int64_t value) {
  if (!g || !key) return NIQKI_E_INVALID;
  if (!std::strcmp(key, "exchange")) {
    if (value < 0 || value > 2) return gfail(g, NIQKI_E_INVALID, "exchange: 0 = choose, 1 = sparse, 2 = dense");
    g->exchange = (int)value;
    return NIQKI_OK;
  }
  if (!std::strcmp(key, "cand_cap")) {
    if (value < 2 || value > 65536 || (value & 1)) return gfail(g, NIQKI_E_INVALID, "cand_cap must be even, in 2..65536");
    g->cand_cap = (uint32_t)value;
    return NIQKI_OK;
  }
  if (!std::strcmp(key, "surv_cap")) {
    if (value < 2 || value > (int64_t)nq::kSurvMax) return gfail(g, NIQKI_E_INVALID, "surv_cap must be in 2..4096");
    g->surv_cap = (uint32_t)value;
    return NIQKI_OK;
  }
  return gfail(g, NIQKI_E_INVALID, std::string("unknown group option ") + key);
}

int niqki_group_get_stat(const niqki_group *g, const char *key, uint64_t *value) {
  if (!g || !key || !value) return NIQKI_E_INVALID;
  if (!std::strcmp(key, "overflows")) { *value = g->overflows; return NIQKI_OK; }
  if (!std::strcmp(key, "rccl")) { *value = g->transport == niqki_group::kRccl ? 1 : 0; return NIQKI_OK; }
  if (!std::strcmp(key, "transport")) { *value = (uint64_t)g->transport; return NIQKI_OK; }   // 0 local, 1 rccl, 2 ipc
  if (!std::strcmp(key, "ipc_words_kind")) { *value = nqg::ipc_words_kind(g); return NIQKI_OK; }
  if (!std::strcmp(key, "ipc_arena_fine")) { *value = nqg::ipc_arena_fine(g); return NIQKI_OK; }
  if (!std::strcmp(key, "ranks_seen")) return nqg::ranks_seen(g, value);
  if (!std::strcmp(key, "sparse")) {
    *value = plan_of(g, exchange_of(g), 1, std::max(1u, g->sh[0]->n_genomes)).sparse;
    return NIQKI_OK;
  }
  return NIQKI_E_INVALID;
}

int niqki_group_insert(niqki_group *g, const int32_t *const *local_sketches, uint32_t per, uint32_t n_total) {
  if (!g || !local_sketches) return NIQKI_E_INVALID;
  if (g->pend.active) return gfail(g, NIQKI_E_STATE, "a query batch is in flight (niqki_group_query_end)");
  if ((uint64_t)n_total > (uint64_t)per * g->world) return gfail(g, NIQKI_E_INVALID, "n_total exceeds world * per");
  if (per == 0) return NIQKI_OK;
  const niqki_group_plan plan = plan_of(g, 2, per, 0);   // (only the slices travel)
  int rc = reserve_batch(g, plan, per, false);
  if (rc) return rc;
  if ((rc = exchange_slices(g, plan, local_sketches, per))) return rc;
  return each_rank(g, [&](uint32_t l, niqki_index *ix, Ws &w) -> int {
    // rows are rank major = batch order: the first n_total of them are the batch
    NQ_G(g, l, nqi::insert_dev(ix, (const int32_t *)w.allsk.p, ix->d.slot_end - ix->d.slot_begin, 0, n_total));
    return NIQKI_OK;
  });
}

namespace {

uint32_t pow2_at_least(uint32_t x) {
  uint32_t p = 1;
  while (p < x) p <<= 1;
  return p;
}

// this shard's partial counts of the ids a query's ranks proposed (nq::surv_lookup_kernel)
// (wide: `mine` holds uint32_t values)
hipError_t launch_surv_lookup(niqki_index *ix, const int2 *surv, const int32_t *surv_n, uint32_t SC, uint32_t nq_, uint32_t m,
                              const nq::IdView &ids, const int32_t *sk, uint32_t q_stride, uint32_t q_off, void *mine,
                              bool wide = false) {
  if (nq_ == 0 || m == 0) return hipSuccess;
  const uint32_t T = pow2_at_least(2 * std::max(SC, 1u));
  const size_t lds = (size_t)T * 8 + (size_t)((m + 31) / 32) * 4;
  const uint32_t f_local = ix->d.slot_end - ix->d.slot_begin;
  auto launch = [&](auto *out) -> hipError_t {   // out: CT *
    const auto kernel = nq::surv_lookup_kernel<std::remove_pointer_t<decltype(out)>>;
    hipError_t e = hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, dim3(nq_), dim3(256), lds, ix->stream, surv, surv_n, SC, T, m, ids, sk, q_stride, q_off, f_local,
                       (const uint16_t *)ix->store, (uint64_t)ix->cap, ix->d.R, out);
    return hipGetLastError();
  };
  return wide ? launch((uint32_t *)mine) : launch((uint16_t *)mine);
}

// hits of `per` queries (first_q ..) from candidate ids and their summed counts; keys / nhit: scratch
int hits_from_candidates(niqki_index *ix, const void *tot, uint32_t first_q, uint32_t per, uint32_t m, const nq::IdView &ids,
                         uint32_t min_score, Buf &keys, Buf &nhit, unsigned long long *hit_off, uint32_t *hc, uint32_t *hg,
                         uint64_t capacity, bool wide = false) {
  if (per == 0) return NIQKI_OK;
  if (m > nq::kCandMax) return nqi::fail(ix, NIQKI_E_INVALID, "too many candidate ids per query");
  int rc = nqi::ensure(ix, keys, std::max<size_t>((size_t)per * m * 8, 8));
  if (!rc) rc = nqi::ensure(ix, nhit, (size_t)per * 4);
  if (rc) return rc;
  const uint32_t P = pow2_at_least(std::max(m, 2u)), T = 2 * P;
  const size_t lds = (size_t)P * 8 + (size_t)T * 4;
  nqi::Span sp(ix, NIQKI_KC_HITS);
  auto launch = [&](const auto *sums) -> int {   // sums: const CT *
    const auto kernel = nq::cand_hits_kernel<std::remove_const_t<std::remove_pointer_t<decltype(sums)>>>;
    NQ_HIP(ix, hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kernel, dim3(per), dim3(256), lds, ix->stream, sums, first_q, m, ids, min_score, T, P,
                       (unsigned long long *)keys.p, (uint32_t *)nhit.p);
    return NIQKI_OK;
  };
  if ((rc = wide ? launch((const uint32_t *)tot) : launch((const uint16_t *)tot))) return rc;
  hipLaunchKernelGGL(nq::cand_hits_scan_kernel, dim3(1), dim3(1024), 0, ix->stream, (const uint32_t *)nhit.p, per, hit_off);
  hipLaunchKernelGGL(nq::cand_hits_write_kernel, dim3(per), dim3(256), 0, ix->stream, (const unsigned long long *)keys.p,
                     (const uint32_t *)nhit.p, m, (const unsigned long long *)hit_off, hc, hg, (unsigned long long)capacity);
  NQ_HIP(ix, hipGetLastError());
  return NIQKI_OK;
}

// Where rank l's hit lists of the batch in flight are made: the caller's arrays or, for host results, the library's
// staging buffers (copied out by query_end).
int hit_out(niqki_group *g, uint32_t l, nqi::HitOut &out) {
  auto &pd = g->pend;
  auto &w = g->ws[l];
  out = nqi::HitOut{(unsigned long long *)pd.hit_off[l], pd.hit_counts[l], pd.hit_gids[l], pd.capacity};
  if (!pd.host) return NIQKI_OK;
  NQ_G(g, l, nqi::ensure(g->sh[l], w.hitoff, (size_t)(pd.per + 1) * 8));
  NQ_G(g, l, nqi::ensure(g->sh[l], w.hc, (size_t)std::max<uint64_t>(pd.capacity, 1) * 4));
  NQ_G(g, l, nqi::ensure(g->sh[l], w.hg, (size_t)std::max<uint64_t>(pd.capacity, 1) * 4));
  out = nqi::HitOut{(unsigned long long *)w.hitoff.p, (uint32_t *)w.hc.p, (uint32_t *)w.hg.p, pd.capacity};
  return NIQKI_OK;
}

// 3 (dense form): counter rows of all queries over the local slots
int gather_rows(niqki_group *g, uint32_t per, const niqki_group_plan &plan) {
  const uint32_t nq_ = g->world * per, N = g->pend.N;
  const uint64_t stride = plan.row_stride;
  const int rc = nqg::before_write(g, kCounts);
  if (rc) return rc;
  return each_rank(g, [&](uint32_t l, niqki_index *ix, Ws &w) -> int {
    const size_t cells = std::max<size_t>((size_t)nq_ * stride, 2);
    NQ_G(g, l, nqi::ensure(ix, w.xbuf[kCounts], cells * (g->wide ? 4 : 2)));
    Buf &rows = g->wide ? w.rows16 : w.xbuf[kCounts];   // S = 16: u16 rows of the shard first, widened for the sum
    if (g->wide) NQ_G(g, l, nqi::ensure(ix, w.rows16, cells * 2));
    if (N == 0) NQ_GH(g, hipMemsetAsync(rows.p, 0, cells * 2, ix->stream));
    NQ_G(g, l, nqi::counts_dev(ix, (const int32_t *)w.allsk.p, ix->d.slot_end - ix->d.slot_begin, 0, nq_, (uint16_t *)rows.p,
                               stride, nullptr, nullptr));
    if (g->wide) {
      hipLaunchKernelGGL(nq::widen_rows_kernel, dim3(4096), dim3(256), 0, ix->stream, (const uint16_t *)w.rows16.p,
                         (uint64_t)nq_ * stride, (uint32_t *)w.xbuf[kCounts].p);
      NQ_GH(g, hipGetLastError());
    }
    return NIQKI_OK;
  });
}

// 4b of a batch whose partial hit vectors (ws.xbuf[kCounts]) are complete: dense reduce-scatter into ws.red
int finish_dense(niqki_group *g, uint32_t per, const niqki_group_plan &plan) {
  const uint64_t stride = plan.row_stride;
  const size_t cells = std::max<size_t>((size_t)per * stride, 2);
  int rc = each_rank(g, [&](uint32_t l, niqki_index *ix, Ws &w) -> int {
    NQ_G(g, l, nqi::ensure(ix, w.red, cells * 2 * (g->wide ? 2 : 1)));   // (S = 16: two planes)
    if (g->wide) NQ_G(g, l, nqi::ensure(ix, w.sum32, cells * 4));
    return NIQKI_OK;
  });
  if (rc) return rc;
  nqi::Span sp(g->sh[0], NIQKI_KC_EXCHANGE);
  if (!g->wide) return nqg::reduce_scatter_u32(g, kCounts, &Ws::red, (size_t)plan.sum_words);
  if ((rc = nqg::reduce_scatter_u32(g, kCounts, &Ws::sum32, (size_t)plan.sum_words))) return rc;
  return each_rank(g, [&](uint32_t, niqki_index *ix, Ws &w) -> int {
    hipLaunchKernelGGL(nq::split_sums_kernel, dim3(4096), dim3(256), 0, ix->stream, (const uint32_t *)w.sum32.p, (uint64_t)per * stride,
                       (uint16_t *)w.red.p, (uint16_t *)w.red.p + cells);
    NQ_GH(g, hipGetLastError());
    return NIQKI_OK;
  });
}

// 5. threshold + order of this rank's queries from ws.red into the caller's device buffers or the
// library's staging buffers (host results: copied out by query_end)
int run_hits(niqki_group *g, uint32_t per, const niqki_group_plan &plan) {
  auto &pd = g->pend;
  const uint32_t N = pd.N;
  const uint64_t stride = plan.row_stride;
  return each_rank(g, [&](uint32_t l, niqki_index *ix, Ws &w) -> int {
    const uint16_t *plane2 = g->wide ? (const uint16_t *)w.red.p + std::max<size_t>((size_t)per * stride, 2) : nullptr;
    nqi::HitOut out;
    const int rc = hit_out(g, l, out);
    if (rc) return rc;
    if (!pd.host && pd.capacity) {
      // Device outputs are final as they stand: where the batch holds more than `capacity` hits the caller keeps the
      // first `capacity` of them, so the list that crosses that border must be the HEAD of the query's list.  The hit
      // kernels leave out a crossing list's entries past the border BEFORE they order it (its smallest gids, not its
      // last entries): the lists are made in staging buffers with room for one more whole list and their head copied.
      const uint64_t room = pd.capacity + N;
      NQ_G(g, l, nqi::ensure(ix, w.hc, (size_t)room * 4));
      NQ_G(g, l, nqi::ensure(ix, w.hg, (size_t)room * 4));
      out = nqi::HitOut{(unsigned long long *)pd.hit_off[l], (uint32_t *)w.hc.p, (uint32_t *)w.hg.p, room};
    }
    NQ_G(g, l, nqi::hits_dev(ix, (const uint16_t *)w.red.p, plane2, per, stride, 0, N, out));
    if (!pd.host && pd.capacity) {
      const uint32_t blocks = (uint32_t)std::min<uint64_t>((pd.capacity + 255) / 256, 1024);
      hipLaunchKernelGGL(nq::hits_head_kernel, dim3(blocks), dim3(256), 0, ix->stream, (const unsigned long long *)pd.hit_off[l] + per,
                         (unsigned long long)pd.capacity, (const uint32_t *)w.hc.p, (const uint32_t *)w.hg.p, pd.hit_counts[l],
                         pd.hit_gids[l]);
      NQ_GH(g, hipGetLastError());
    }
    return NIQKI_OK;
  });
}

// 3 (sparse form): gather over the local slots WITHOUT counter rows.  What leaves the kernel is, per query, the
// candidates (partial count >= ceil(min_score / G): their ids travel) and the survivors (partial count >= half of
// that, with their counts: what the other ranks' candidates are looked up in)
int gather_candidates(niqki_group *g, uint32_t per, const niqki_group_plan &plan) {
  const uint32_t G = g->world, nq_ = G * per, C = g->cand_cap, SC = g->surv_cap;
  const size_t blob = plan.cand_blob_bytes, sum_bytes = (size_t)plan.sum_words * 4;
  const int rc = nqg::before_write(g, kCand);
  if (rc) return rc;
  return each_rank(g, [&](uint32_t l, niqki_index *ix, Ws &w) -> int {
    NQ_G(g, l, nqi::ensure(ix, w.xbuf[kCand], blob));
    NQ_G(g, l, nqi::ensure(ix, w.surv, (size_t)nq_ * SC * 8));
    NQ_G(g, l, nqi::ensure(ix, w.cand_all, (size_t)G * blob));
    NQ_G(g, l, nqi::ensure(ix, w.xbuf[kMine], sum_bytes * G));
    NQ_G(g, l, nqi::ensure(ix, w.tot, sum_bytes));
    NQ_G(g, l, nqi::ensure(ix, w.flag, 4));
    nq::CandOut co;
    co.cand = (int32_t *)w.xbuf[kCand].p;
    co.n = (int32_t *)w.xbuf[kCand].p + (size_t)nq_ * C;
    co.thr = plan.cand_threshold;
    co.cap = C;
    co.surv = (int2 *)w.surv.p;
    co.surv_n = co.n + nq_;
    co.surv_thr = plan.surv_threshold;
    co.surv_cap = SC;
    NQ_G(g, l, nqi::counts_dev(ix, (const int32_t *)w.allsk.p, ix->d.slot_end - ix->d.slot_begin, 0, nq_, nullptr, plan.row_stride,
                               nullptr, &co));
    return NIQKI_OK;
  });
}

// 4 (sparse form): the candidates of all ranks, my partial counts of them, their sums (ws.tot)
int sum_candidates(niqki_group *g, uint32_t per, const niqki_group_plan &plan) {
  const uint32_t G = g->world, nq_ = G * per, C = g->cand_cap, SC = g->surv_cap;
  const size_t blob = plan.cand_blob_bytes;
  int rc;
  {
    nqi::Span sp(g->sh[0], NIQKI_KC_EXCHANGE);
    if ((rc = nqg::all_gather(g, kCand, &Ws::cand_all, blob))) return rc;
  }
  if ((rc = nqg::before_write(g, kMine))) return rc;
  rc = each_rank(g, [&](uint32_t, niqki_index *ix, Ws &w) -> int {
    nqi::Span sp(ix, NIQKI_KC_EXCHANGE);
    NQ_GH(g, hipMemsetAsync(w.flag.p, 0, 4, ix->stream));
    const nq::IdView ids{(const int32_t *)w.cand_all.p, (uint64_t)(blob / 4), C};
    NQ_GH(g, launch_surv_lookup(ix, (const int2 *)w.surv.p, (const int32_t *)w.xbuf[kCand].p + (size_t)nq_ * C + nq_, SC, nq_, G * C, ids,
                                (const int32_t *)w.allsk.p, ix->d.slot_end - ix->d.slot_begin, 0, w.xbuf[kMine].p, g->wide));
    // a candidate list of ANY rank that overflowed (same words on every rank: all decide alike)
    hipLaunchKernelGGL(nq::blob_overflow_kernel, dim3((nq_ + 255) / 256), dim3(256), 0, ix->stream, (const int32_t *)w.cand_all.p,
                       (uint64_t)(blob / 4), nq_, G, C, SC, (uint32_t *)w.flag.p);
    NQ_GH(g, hipGetLastError());
    return NIQKI_OK;
  });
  if (rc) return rc;
  nqi::Span sp(g->sh[0], NIQKI_KC_EXCHANGE);
  return nqg::reduce_scatter_u32(g, kMine, &Ws::tot, (size_t)plan.sum_words);
}

// 5 (sparse form).  The overflow word stays on the device: the hits are made from the candidates' sums right away,
// and query_end -- the one place the host waits -- redoes the batch densely in the (rare) case that a list overflowed.
int hits_of_candidates(niqki_group *g, uint32_t per, const niqki_group_plan &plan) {
  const uint32_t G = g->world, C = g->cand_cap, min_score = g->sh[0]->d.min_score;
  return each_rank(g, [&](uint32_t l, niqki_index *ix, Ws &w) -> int {
    nqi::HitOut out;
    const int rc = hit_out(g, l, out);
    if (rc) return rc;
    const nq::IdView ids{(const int32_t *)w.cand_all.p, (uint64_t)(plan.cand_blob_bytes / 4), C};
    NQ_G(g, l, hits_from_candidates(ix, w.tot.p, (g->first + l) * per, per, G * C, ids, min_score, w.keys, w.nhit, out.off, out.counts,
                                    out.gids, out.capacity, g->wide));
    return NIQKI_OK;
  });
}

// A batch counts as in flight only if begin went through: whatever way begin fails, query_end finds no batch.
struct InFlight {
  niqki_group::Pending &pd;
  bool keep = false;
  explicit InFlight(niqki_group::Pending &p) : pd(p) { pd.active = true; }
  ~InFlight() { pd.active = keep; }
};

}  // namespace

int niqki_group_query_begin(niqki_group *g, const int32_t *const *local_sketches, uint32_t per, uint64_t *const *hit_off,
                            uint32_t *const *hit_counts, uint32_t *const *hit_gids, uint64_t capacity, int mem) {
  if (!g || !local_sketches || !hit_off) return NIQKI_E_INVALID;
  if (g->pend.active) return gfail(g, NIQKI_E_STATE, "a query batch is already in flight (niqki_group_query_end)");
  int rc = each_rank(g, [&](uint32_t l, niqki_index *ix, Ws &) -> int {
    NQ_G(g, l, nqi::build_if_needed(ix));
    if (ix->built_n != g->sh[0]->built_n) return gfail(g, NIQKI_E_STATE, "the shards hold different numbers of genomes");
    return NIQKI_OK;
  });
  if (rc) return rc;
  const uint32_t N = g->sh[0]->built_n;
  const niqki_group_plan plan = plan_of(g, exchange_of(g), per, N);
  auto &pd = g->pend;
  pd.per = per; pd.N = N; pd.capacity = capacity; pd.host = mem != NIQKI_MEM_DEVICE;
  pd.off_v.assign(hit_off, hit_off + g->n_local);
  pd.hc_v.assign(hit_counts, hit_counts + g->n_local);
  pd.hg_v.assign(hit_gids, hit_gids + g->n_local);
  pd.hit_off = pd.off_v.data(); pd.hit_counts = pd.hc_v.data(); pd.hit_gids = pd.hg_v.data();
  pd.sparse = per != 0 && plan.sparse != 0;
  InFlight batch(pd);
  if (per == 0) { batch.keep = true; return NIQKI_OK; }
  if ((rc = reserve_batch(g, plan, per, true))) return rc;
  if ((rc = exchange_slices(g, plan, local_sketches, per))) return rc;
  if (pd.sparse) {
    if ((rc = gather_candidates(g, per, plan))) return rc;
    if ((rc = sum_candidates(g, per, plan))) return rc;
    if ((rc = hits_of_candidates(g, per, plan))) return rc;
  } else {
    if ((rc = gather_rows(g, per, plan))) return rc;
    if ((rc = finish_dense(g, per, plan))) return rc;
    if ((rc = run_hits(g, per, plan))) return rc;
  }
  // the two words query_end looks at, on their way to pinned memory behind everything above
  NQ_GH(g, hipSetDevice(g->sh[0]->device));
  g->host_flags[0] = g->host_flags[1] = 0;
  if (pd.sparse) NQ_GH(g, hipMemcpyAsync(&g->host_flags[0], g->ws[0].flag.p, 4, hipMemcpyDeviceToHost, g->sh[0]->stream));
  if (const uint32_t *timeout = nqg::timeout_flag(g))
    NQ_GH(g, hipMemcpyAsync(&g->host_flags[1], timeout, 4, hipMemcpyDeviceToHost, g->sh[0]->stream));
  NQ_GH(g, hipEventRecord(g->ev_flags, g->sh[0]->stream));
  batch.keep = true;
  return NIQKI_OK;
}

int niqki_group_query_end(niqki_group *g) {
  if (!g) return NIQKI_E_INVALID;
  auto &pd = g->pend;
  if (!pd.active) return gfail(g, NIQKI_E_STATE, "no query batch in flight");
  pd.active = false;
  const uint32_t per = pd.per;
  if (per == 0) return NIQKI_OK;
  NQ_GH(g, hipSetDevice(g->sh[0]->device));
  NQ_GH(g, hipEventSynchronize(g->ev_flags));
  if (g->host_flags[1]) return gfail(g, NIQKI_E_HIP, "a peer of the group did not answer in time (ipc transport)");
  int rc;
  if (pd.sparse && g->host_flags[0]) {
    // a list overflowed on some rank: the batch again with counter rows (the sketch slices are still in ws.allsk)
    ++g->overflows;
    const niqki_group_plan dense = plan_of(g, 2, per, pd.N);
    if ((rc = reserve_batch(g, dense, per, true))) return rc;
    if ((rc = gather_rows(g, per, dense))) return rc;
    if ((rc = finish_dense(g, per, dense))) return rc;
    if ((rc = run_hits(g, per, dense))) return rc;
  }
  if (!pd.host) return NIQKI_OK;
  return each_rank(g, [&](uint32_t l, niqki_index *ix, Ws &w) -> int {
    NQ_GH(g, hipMemcpyAsync(pd.hit_off[l], w.hitoff.p, (size_t)(per + 1) * 8, hipMemcpyDeviceToHost, ix->stream));
    NQ_GH(g, hipStreamSynchronize(ix->stream));
    const uint64_t total = pd.hit_off[l][per];
    if (total > pd.capacity) return gfail(g, NIQKI_E_CAPACITY, "hit capacity too small; hit_off holds the sizes needed");
    if (total) {
      NQ_GH(g, hipMemcpyAsync(pd.hit_counts[l], w.hc.p, (size_t)total * 4, hipMemcpyDeviceToHost, ix->stream));
      NQ_GH(g, hipMemcpyAsync(pd.hit_gids[l], w.hg.p, (size_t)total * 4, hipMemcpyDeviceToHost, ix->stream));
      NQ_GH(g, hipStreamSynchronize(ix->stream));
    }
    return NIQKI_OK;
  });
}

int niqki_group_query(niqki_group *g, const int32_t *const *local_sketches, uint32_t per, uint64_t *const *hit_off,
                      uint32_t *const *hit_counts, uint32_t *const *hit_gids, uint64_t capacity, int mem) {
  const int rc = niqki_group_query_begin(g, local_sketches, per, hit_off, hit_counts, hit_gids, capacity, mem);
  return rc ? rc : niqki_group_query_end(g);   // (a begin that failed has left no batch in flight)
}

// ---- the row-free sparse exchange step by step (what a shard of a group runs; device memory only) ----
int niqki_query_survivors(niqki_index *ix, const int32_t *sketches, uint32_t nq, uint32_t cand_threshold, uint32_t surv_threshold,
                          uint32_t cand_cap, uint32_t surv_cap, int32_t *cand, int32_t *n_cand, int32_t *surv, int32_t *n_surv,
                          int mem) {
  if (!ix || (nq && (!sketches || !cand || !n_cand || !surv || !n_surv)) || !cand_cap || !surv_cap) return NIQKI_E_INVALID;
  if (mem != NIQKI_MEM_DEVICE) return nqi::fail(ix, NIQKI_E_INVALID, "niqki_query_survivors is device-memory only");
  NQ_HIP(ix, hipSetDevice(ix->device));
  nq::CandOut co;
  co.cand = cand; co.n = n_cand; co.thr = cand_threshold; co.cap = cand_cap;
  co.surv = (int2 *)surv; co.surv_n = n_surv; co.surv_thr = surv_threshold; co.surv_cap = surv_cap;
  return nqi::counts_dev(ix, sketches, ix->d.F, ix->resident_bytes ? ix->full_begin : ix->d.slot_begin, nq, nullptr, 0, nullptr, &co);
}

int niqki_survivor_counts(niqki_index *ix, const int32_t *sketches, uint32_t nq, const int32_t *ids, uint32_t m, const int32_t *surv,
                          const int32_t *n_surv, uint32_t surv_cap, uint16_t *counts, int mem) {
  if (!ix || (nq && m && (!sketches || !ids || !surv || !n_surv || !counts))) return NIQKI_E_INVALID;
  if (mem != NIQKI_MEM_DEVICE) return nqi::fail(ix, NIQKI_E_INVALID, "niqki_survivor_counts is device-memory only");
  if (ix->resident_bytes) return nqi::fail(ix, NIQKI_E_STATE, "not on a paged index (the sketch store is in host memory)");
  if (m > nq::kCandMax || surv_cap > nq::kSurvMax || !surv_cap) return nqi::fail(ix, NIQKI_E_INVALID, "at most 4096 ids per query and 4096 survivors");
  NQ_HIP(ix, hipSetDevice(ix->device));
  const nq::IdView view{ids, 0, std::max(m, 1u)};
  NQ_HIP(ix, launch_surv_lookup(ix, (const int2 *)surv, n_surv, surv_cap, nq, m, view, sketches, ix->d.F, ix->d.slot_begin, counts));
  return NIQKI_OK;
}

int niqki_hits_from_candidates(niqki_index *ix, const int32_t *ids, const uint16_t *totals, uint32_t nq, uint32_t m, uint64_t *hit_off,
                               uint32_t *hit_counts, uint32_t *hit_gids, uint64_t capacity, int mem) {
  if (!ix || !hit_off || (nq && m && (!ids || !totals))) return NIQKI_E_INVALID;
  if (mem != NIQKI_MEM_DEVICE) return nqi::fail(ix, NIQKI_E_INVALID, "niqki_hits_from_candidates is device-memory only");
  NQ_HIP(ix, hipSetDevice(ix->device));
  if (nq == 0 || m == 0) {
    NQ_HIP(ix, hipMemsetAsync(hit_off, 0, (size_t)(nq + 1) * 8, ix->stream));
    return NIQKI_OK;
  }
  const nq::IdView view{ids, 0, m};
  return hits_from_candidates(ix, totals, 0, nq, m, view, ix->d.min_score, ix->ws_tc, ix->ws_tg, (unsigned long long *)hit_off,
                              hit_counts, hit_gids, capacity);
}

namespace {
// per local rank: `per` sketch rows = the first n_entry[l] sketches of the shard's staged batch
// (niqki_stage_raw on that shard), the rest empty sketches (-1)
int staged_rows(niqki_group *g, uint32_t per, const uint32_t *n_entry, std::vector<const int32_t *> &rows) {
  rows.assign(g->n_local, nullptr);
  return each_rank(g, [&](uint32_t l, niqki_index *ix, Ws &w) -> int {
    const uint32_t n = n_entry ? n_entry[l] : 0;
    if (n > per) return gfail(g, NIQKI_E_INVALID, "a rank's staged entries exceed `per`");
    const size_t row = (size_t)ix->d.F * 4;
    NQ_G(g, l, nqi::ensure(ix, w.stpad, std::max<size_t>((size_t)per * row, 4)));
    if (n) {
      if (!ix->staged.valid || ix->staged.n_entry < n) return gfail(g, NIQKI_E_STATE, "rank " + std::to_string(g->first + l) + " has no staged batch of that size");
      NQ_G(g, l, nqi::staged_sketch_ws(ix));
      NQ_GH(g, hipMemcpyAsync(w.stpad.p, ix->ws_stsk.p, (size_t)n * row, hipMemcpyDeviceToDevice, ix->stream));
    }
    if (n < per) NQ_GH(g, hipMemsetAsync((char *)w.stpad.p + (size_t)n * row, 0xFF, (size_t)(per - n) * row, ix->stream));
    rows[l] = (const int32_t *)w.stpad.p;
    return NIQKI_OK;
  });
}
}  // namespace

int niqki_group_staged_insert(niqki_group *g, uint32_t per, const uint32_t *n_entry) {
  if (!g || !n_entry) return NIQKI_E_INVALID;
  if (g->n_local != g->world) return gfail(g, NIQKI_E_STATE, "staged group calls need all ranks in one process");
  std::vector<const int32_t *> rows;
  int rc = staged_rows(g, per, n_entry, rows);
  if (rc) return rc;
  if (per == 0) return NIQKI_OK;
  if ((rc = exchange_slices(g, plan_of(g, 2, per, 0), rows.data(), per))) return rc;   // (all ranks in one process: nothing to reserve)
  return each_rank(g, [&](uint32_t l, niqki_index *ix, Ws &w) -> int {
    const uint32_t f_local = ix->d.slot_end - ix->d.slot_begin;
    // ids follow the entries: rank after rank, each rank's valid rows
    for (uint32_t s = 0; s < g->world; ++s)
      NQ_G(g, l, nqi::insert_dev(ix, (const int32_t *)w.allsk.p + (size_t)s * per * f_local, f_local, 0, n_entry[s]));
    return NIQKI_OK;
  });
}

int niqki_group_staged_query(niqki_group *g, uint32_t per, const uint32_t *n_entry, uint64_t *const *hit_off,
                             uint32_t *const *hit_counts, uint32_t *const *hit_gids, uint64_t capacity, int mem) {
  if (!g || !n_entry) return NIQKI_E_INVALID;
  if (g->n_local != g->world) return gfail(g, NIQKI_E_STATE, "staged group calls need all ranks in one process");
  std::vector<const int32_t *> rows;
  int rc = staged_rows(g, per, n_entry, rows);
  if (rc) return rc;
  return niqki_group_query(g, rows.data(), per, hit_off, hit_counts, hit_gids, capacity, mem);
}

}  // extern "C"
