// nq_api_unite.hip -- niqki_unite behind the C ABI: one entry per label.  The host numbers the labels by first appearance
// and lists every label's members (one-off work, as niqki_set_labels does its own); store_unite_kernel (nq_unite.hip,
// launch shape in nq_unite_blocks.h) takes the per-label minimum of every row of the sketch store into a new, smaller
// store, and every index segment is dropped, so the next use builds ONE main segment over the labels' sketches.  A paged
// handle's store is page-locked host memory: the host takes the minima row by row in place.  DESIGN.md 4.6h.
#include "nq_handle.h"

#include <algorithm>
#include <chrono>
#include <string>
#include <unordered_map>
#include <vector>

namespace nqi {

namespace {

// labels -> every genome's label number (by first appearance), and the members of every label: off[L + 1], then the
// genome ids sorted by (label number, genome id)
struct Groups {
  std::vector<uint32_t> ids, off, members;
  uint32_t n_labels = 0;
};

void group_labels(const uint32_t *labels, uint32_t n, Groups &g) {
  std::unordered_map<uint32_t, uint32_t> number;
  number.reserve(n);
  g.ids.resize(n);
  for (uint32_t i = 0; i < n; ++i) g.ids[i] = number.emplace(labels[i], (uint32_t)number.size()).first->second;
  g.n_labels = (uint32_t)number.size();
  g.off.assign((size_t)g.n_labels + 1, 0);
  for (uint32_t i = 0; i < n; ++i) ++g.off[g.ids[i] + 1];
  for (uint32_t l = 0; l < g.n_labels; ++l) g.off[l + 1] += g.off[l];
  std::vector<uint32_t> at(g.off.begin(), g.off.end() - 1);
  g.members.resize(n);
  for (uint32_t i = 0; i < n; ++i) g.members[at[g.ids[i]]++] = i;
}

// paged handle: every row of the host store, forward and in place.  Label l's members are all at or above column l (l
// labels have a smaller first member), and column l itself belongs to a label numbered at most l, which is read
// before it is written.
void unite_host_store(niqki_index *ix, const Groups &g) {
  const uint32_t f_all = ix->full_end - ix->full_begin;
  for (uint32_t s = 0; s < f_all; ++s) {
    uint16_t *row = ix->host_store + (size_t)s * ix->host_cap;
    for (uint32_t l = 0; l < g.n_labels; ++l) {
      uint16_t m = nq::kEmpty16;
      for (uint32_t j = g.off[l]; j < g.off[l + 1]; ++j) m = row[g.members[j]] < m ? row[g.members[j]] : m;
      row[l] = m;
    }
  }
}

double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

int unite_run(niqki_index *ix, const uint32_t *labels, uint32_t *new_ids, uint32_t *n_labels, int mem) {
  const uint32_t N = ix->n_genomes;
  const bool dev = mem == NIQKI_MEM_DEVICE;
  ix->unite_ms[0] = ix->unite_ms[1] = 0;
  const auto t0 = std::chrono::steady_clock::now();
  std::vector<uint32_t> h_lab;
  if (dev) {
    h_lab.resize(N);
    NQ_HIP(ix, hipMemcpyAsync(h_lab.data(), labels, (size_t)N * 4, hipMemcpyDeviceToHost, ix->stream));
    NQ_HIP(ix, hipStreamSynchronize(ix->stream));   // the one synchronisation of a device call's inputs
    labels = h_lab.data();
  }
  Groups g;
  group_labels(labels, N, g);
  const uint32_t L = g.n_labels;
  if (new_ids) {
    if (dev) NQ_HIP(ix, hipMemcpyAsync(new_ids, g.ids.data(), (size_t)N * 4, hipMemcpyHostToDevice, ix->stream));
    else std::copy(g.ids.begin(), g.ids.end(), new_ids);
  }
  if (n_labels) *n_labels = L;
  drop_labels(ix);     // (also when every label is distinct, so that the call's effect does not depend on the labels)
  drop_taxonomy(ix);
  drop_sizes(ix);
  if (L == N) {        // all distinct: the handle, a built index included, stays as it is
    if (dev && new_ids) NQ_HIP(ix, hipStreamSynchronize(ix->stream));   // (g.ids leaves scope)
    if (ix->prof) ix->unite_ms[0] = ms_since(t0);
    return NIQKI_OK;
  }

  if (ix->resident_bytes) {
    if (dev && new_ids) NQ_HIP(ix, hipStreamSynchronize(ix->stream));
    if (ix->prof) ix->unite_ms[0] = ms_since(t0);
    const auto t1 = std::chrono::steady_clock::now();
    NQ_HIP(ix, hipStreamSynchronize(ix->stream));   // a page copy that still reads the host store
    release_segments(ix);
    unite_host_store(ix, g);
    host_store_rewritten(ix, L);
    if (ix->prof) ix->unite_ms[1] = ms_since(t1);
    return NIQKI_OK;
  }

  // off[L + 1] and the members on the device, then the new store (on failure the genome set is unchanged)
  const size_t off_bytes = ((size_t)L + 2) / 2 * 8;
  int rc = ensure(ix, ix->ws_parent, off_bytes + (size_t)N * 4);
  if (rc) return rc;
  uint32_t *d_off = (uint32_t *)ix->ws_parent.p, *d_mem = (uint32_t *)((uint8_t *)ix->ws_parent.p + off_bytes);
  NQ_HIP(ix, hipMemcpyAsync(d_off, g.off.data(), ((size_t)L + 1) * 4, hipMemcpyHostToDevice, ix->stream));
  NQ_HIP(ix, hipMemcpyAsync(d_mem, g.members.data(), (size_t)N * 4, hipMemcpyHostToDevice, ix->stream));
  const uint32_t f_local = ix->d.slot_end - ix->d.slot_begin;
  const uint64_t cap = nq::retain_cap(L);
  uint16_t *ns = nullptr;
  if (hipMalloc((void **)&ns, (size_t)f_local * cap * 2) != hipSuccess) {
    (void)hipStreamSynchronize(ix->stream);   // (the copies read g)
    return fail(ix, NIQKI_E_NOMEM, "niqki_unite: sketch store allocation failed");
  }
  hipEvent_t ev[2] = {nullptr, nullptr};
  if (ix->prof) {
    (void)hipStreamSynchronize(ix->stream);   // the preparation ends with its copies
    ix->unite_ms[0] = ms_since(t0);
    for (auto &e : ev)
      if (hipEventCreate(&e) != hipSuccess) e = nullptr;
  }
  if (ev[0]) (void)hipEventRecord(ev[0], ix->stream);
  hipError_t e;
  {
    Span sp(ix, NIQKI_KC_BUILD);
    e = nq::launch_store_unite(ix->store, ix->cap, ns, cap, f_local, L, d_off, d_mem, ix->stream);
  }
  if (ev[1]) (void)hipEventRecord(ev[1], ix->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ix->stream);   // the call's synchronisation: the old store goes, g leaves scope
  float ms = 0;
  if (e == hipSuccess && ev[0] && ev[1] && hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) ix->unite_ms[1] = ms;
  for (auto &x : ev) if (x) (void)hipEventDestroy(x);
  if (e != hipSuccess) {
    (void)hipFree(ns);
    return fail(ix, NIQKI_E_HIP, std::string("niqki_unite: minimum pass: ") + hipGetErrorString(e));
  }
  release_segments(ix);
  return adopt_store(ix, ns, cap, L);
}

}  // namespace

}  // namespace nqi

using namespace nqi;

extern "C" {

int niqki_unite(niqki_index *ix, const uint32_t *labels, uint32_t n, uint32_t *new_ids, uint32_t *n_labels, int mem) {
  if (!ix) return NIQKI_E_INVALID;
  if (n != ix->n_genomes) return fail(ix, NIQKI_E_INVALID, "niqki_unite: " + std::to_string(n) + " labels for " + std::to_string(ix->n_genomes) + " genomes");
  if (!labels && n) return NIQKI_E_INVALID;
  if (!whole_range(ix)) return fail(ix, NIQKI_E_STATE, "niqki_unite: a slot-range shard holds part of every sketch; unite genomes on a whole-range handle");
  if (ix->append.active) return fail(ix, NIQKI_E_STATE, "niqki_unite: an append is pending: finish it or call niqki_append_cancel first");
  NQ_HIP(ix, hipSetDevice(ix->device));
  if (n == 0) {
    if (n_labels) *n_labels = 0;
    return NIQKI_OK;
  }
  return unite_run(ix, labels, new_ids, n_labels, mem);
}

}  // extern "C"
