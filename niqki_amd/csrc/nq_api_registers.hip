// nq_api_registers.hip -- niqki_registers / niqki_sketch_registers / niqki_staged_registers behind the C ABI: the
// histograms of the HyperLogLog registers that the top H bits of the cells are (niqki_hip.h).  The store pass and the
// row pass are nq_registers.hip; a paged handle's store is page-locked host memory, so the host counts it in place, as
// niqki_unite takes its minima there.  Nothing here is floating point: the estimate is the caller's
// (niqki_amd/host/size_estimate.h).  DESIGN.md 4.6j.
#include "nq_handle.h"

#include <algorithm>
#include <string>
#include <vector>

namespace nqi {

namespace {

// what every call of the family refuses, in this order
int registers_refusal(niqki_index *ix, const char *who) {
  const nq::Derived &d = ix->d;
  if (d.H > 6) return fail(ix, NIQKI_E_INVALID, std::string(who) + ": H = " + std::to_string(d.H) + ", register histograms take H <= 6 (65 bins)");
  if (d.mask_m != (1u << d.M) - 1u || d.max_rem != (1u << d.H) - 1u)
    return fail(ix, NIQKI_E_STATE, std::string(who) + ": niqki_select_best_H changed H after construction, the top H bits of a cell are no register; "
                                                      "create the index with the H it should have");
  if (!whole_range(ix)) return fail(ix, NIQKI_E_STATE, std::string(who) + ": a slot-range shard holds part of every sketch; read registers on a whole-range handle");
  return NIQKI_OK;
}

// paged handle: columns [begin, end) of every row of the host store
void host_store_registers(const niqki_index *ix, uint32_t begin, uint32_t end, uint32_t *hist) {
  const uint32_t f_all = ix->full_end - ix->full_begin, n_reg = 1u << ix->d.H, B = n_reg + 1u;
  for (uint32_t s = 0; s < f_all; ++s) {
    const uint16_t *row = ix->host_store + (size_t)s * ix->host_cap;
    for (uint32_t g = begin; g < end; ++g) ++hist[(size_t)(g - begin) * B + (row[g] < ix->d.R ? row[g] >> ix->d.M : n_reg)];
  }
}

// One pass into `hist` (n x B words in `mem`): preset, launch, and for a host call the one crossing.  which: 0 the
// store pass, 1 the row pass (the slot of registers_ms).
template <class Launch>
int registers_pass(niqki_index *ix, uint64_t n, uint32_t *hist, int mem, int which, Launch launch) {
  const size_t bytes = (size_t)n * ((1u << ix->d.H) + 1u) * 4;
  uint32_t *d_hist = hist;
  if (mem != NIQKI_MEM_DEVICE) {
    int rc = ensure(ix, ix->ws_reg, bytes);
    if (rc) return rc;
    d_hist = (uint32_t *)ix->ws_reg.p;
  }
  ix->registers_ms[which] = 0;
  PhaseTimer ev(ix, 2, ix->registers_ms);
  int rc = ev.create();
  if (rc) return rc;
  NQ_HIP(ix, hipMemsetAsync(d_hist, 0, bytes, ix->stream));
  if ((rc = ev.mark(0))) return rc;
  NQ_HIP(ix, launch(d_hist));
  if ((rc = ev.mark(1))) return rc;
  if (mem != NIQKI_MEM_DEVICE) {
    NQ_HIP(ix, hipMemcpyAsync(hist, d_hist, bytes, hipMemcpyDeviceToHost, ix->stream));
    NQ_HIP(ix, hipStreamSynchronize(ix->stream));
  }
  return ev.add(0, 1, which);   // (synchronises, while profiling is on only)
}

int row_registers(niqki_index *ix, const int32_t *d_sk, uint32_t n, uint32_t *hist, int mem) {
  return registers_pass(ix, n, hist, mem, 1, [&](uint32_t *d_hist) { return nq::launch_row_registers(ix->d, d_sk, n, d_hist, ix->stream); });
}

}  // namespace

}  // namespace nqi

using namespace nqi;

extern "C" {

int niqki_registers(niqki_index *ix, uint32_t begin, uint32_t end, uint32_t *hist, int mem) {
  if (!ix) return NIQKI_E_INVALID;
  if (begin > end || end > ix->n_genomes)
    return fail(ix, NIQKI_E_INVALID, "niqki_registers: genomes [" + std::to_string(begin) + ", " + std::to_string(end) + ") of " + std::to_string(ix->n_genomes));
  int rc = registers_refusal(ix, "niqki_registers");
  if (rc) return rc;
  if (begin == end) return NIQKI_OK;
  if (!hist) return NIQKI_E_INVALID;
  NQ_HIP(ix, hipSetDevice(ix->device));
  if (ix->resident_bytes) {
    const size_t words = (size_t)(end - begin) * ((1u << ix->d.H) + 1u);
    std::vector<uint32_t> h;
    uint32_t *dst = hist;
    if (mem == NIQKI_MEM_DEVICE) {
      h.assign(words, 0);
      dst = h.data();
    } else {
      std::fill(hist, hist + words, 0u);
    }
    ix->registers_ms[0] = 0;
    NQ_HIP(ix, hipStreamSynchronize(ix->stream));   // (an insert's rows on their way into the host store)
    host_store_registers(ix, begin, end, dst);
    if (mem == NIQKI_MEM_DEVICE) {
      NQ_HIP(ix, hipMemcpyAsync(hist, dst, words * 4, hipMemcpyHostToDevice, ix->stream));
      NQ_HIP(ix, hipStreamSynchronize(ix->stream));   // (h leaves scope)
    }
    return NIQKI_OK;
  }
  return registers_pass(ix, end - begin, hist, mem, 0, [&](uint32_t *d_hist) {
    return nq::launch_store_registers(ix->d, ix->store, ix->cap, ix->d.slot_end - ix->d.slot_begin, begin, end, d_hist, ix->stream);
  });
}

int niqki_sketch_registers(niqki_index *ix, const int32_t *sketches, uint32_t n, uint32_t *hist, int mem) {
  if (!ix) return NIQKI_E_INVALID;
  int rc = registers_refusal(ix, "niqki_sketch_registers");
  if (rc) return rc;
  if (n == 0) return NIQKI_OK;
  if (!sketches || !hist) return NIQKI_E_INVALID;
  NQ_HIP(ix, hipSetDevice(ix->device));
  const int32_t *d_sk = sketches;
  if (mem != NIQKI_MEM_DEVICE) {
    const size_t bytes = (size_t)n * ix->d.F * 4;
    if ((rc = ensure(ix, ix->ws_sk, bytes))) return rc;
    NQ_HIP(ix, hipMemcpyAsync(ix->ws_sk.p, sketches, bytes, hipMemcpyHostToDevice, ix->stream));
    d_sk = (const int32_t *)ix->ws_sk.p;
  }
  return row_registers(ix, d_sk, n, hist, mem);
}

int niqki_staged_registers(niqki_index *ix, uint32_t *hist, int mem) {
  if (!ix) return NIQKI_E_INVALID;
  int rc = registers_refusal(ix, "niqki_staged_registers");
  if (rc) return rc;
  NQ_HIP(ix, hipSetDevice(ix->device));
  if ((rc = staged_sketch_ws(ix))) return rc;
  // (the staged sketches are only read: niqki_staged_query answers as before)
  if (ix->staged.n_entry == 0) return NIQKI_OK;
  if (!hist) return NIQKI_E_INVALID;
  return row_registers(ix, (const int32_t *)ix->ws_stsk.p, ix->staged.n_entry, hist, mem);
}

}  // extern "C"
