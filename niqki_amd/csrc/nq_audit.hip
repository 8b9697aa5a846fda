// nq_audit.hip -- the kernel of niqki_audit (nq_api_audit.hip): per indexed genome g the ordered hit list of its own
// stored sketch, read against the labelling of niqki_set_labels: the first entry under g's label, the first under
// another one, the vote of the first k entries, and the verdict the two counts give -- g's own entry left out of all
// of them (niqki_hip.h has the definition).  Counts, threshold, order and ties come from the query path; nothing here
// counts or orders hits.  Every loop is bounded: the vote by k + 1 lanes, the scan by its list.  None waits for
// another thread, and the only atomic is the one on the info word.  DESIGN.md 4.6i.
#include "../../include/niqki_hip.h"
#include "nq_common.h"
#include "nq_kernels.h"

#include <hip/hip_runtime.h>

#include <algorithm>

namespace nq {

namespace {

constexpr uint32_t kAuditBlock = 256;
constexpr uint32_t kAuditWaves = kAuditBlock / 64;
constexpr uint32_t kAuditNoGid = 0xFFFFFFFFu;

// the rule of niqki_hip.h (NIQKI_AUDIT_*), stated here and nowhere else
__device__ __forceinline__ uint32_t audit_verdict(uint32_t own, uint32_t other) {
  if (own == 0 && other == 0) return NIQKI_AUDIT_ALONE;
  if (own > other) return NIQKI_AUDIT_AGREES;
  if (own == other) return NIQKI_AUDIT_TIED;
  return own ? NIQKI_AUDIT_MISPLACED : NIQKI_AUDIT_STRAY;
}

// A 256-thread workgroup takes four lists at a time, a wavefront each.  The wavefront walks its list 64 entries a
// step; lane i holds entry base + i with its gid, count and label.  H' is the list without the entry whose gid is the
// genome itself: a ballot finds that lane, and an entry's place in H' is its lane less the self lanes before it.
__global__ __launch_bounds__(kAuditBlock) void audit_kernel(AuditArgs a) {
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;   // the lanes before this one
  uint32_t bad = 0;
  for (uint32_t q0 = blockIdx.x * kAuditWaves; q0 < a.nq; q0 += gridDim.x * kAuditWaves) {   // (uniform over the workgroup)
    const uint32_t q = q0 + w;
    if (q >= a.nq) continue;   // (uniform over the wavefront; the kernel has no barrier)
    const uint32_t g = a.t0 + q;
    if (g >= a.n_genomes) {    // never: the host launches lists of indexed genomes
      bad += lane == 0 ? 1u : 0u;
      continue;
    }
    const unsigned long long h0 = a.hit_off[q], h1 = a.hit_off[q + 1];
    uint32_t len = 0;
    if (h1 > h0 && h1 - h0 <= a.n_genomes) len = (uint32_t)(h1 - h0);
    else if (h1 > h0) bad += lane == 0 ? 1u : 0u;   // never a list longer than the genome count; the host ends the call
    const uint32_t *counts = a.hit_counts + h0, *gids = a.hit_gids + h0;
    const uint32_t mine = a.labels[g];
    uint32_t own_c = 0, own_g = kAuditNoGid, oth_c = 0, oth_g = kAuditNoGid, vote_g = kAuditNoGid, vote_n = 0;
    bool own_found = false, oth_found = false;
    for (uint32_t base = 0; base < len; base += 64) {   // (base, len and the two flags are the wavefront's)
      const uint32_t i = base + lane;
      uint32_t gid = kAuditNoGid, cnt = 0, lab = 0;
      bool entry = false;   // an entry of H'
      if (i < len) {
        gid = gids[i];
        cnt = counts[i];
        if (gid >= a.n_genomes) {
          bad += 1;
        } else if (gid != g) {
          lab = a.labels[gid];
          entry = true;
        }
      }
      const unsigned long long in = __ballot(entry);
      if (base == 0) {
        // The vote: V is the first k entries of H'.  k <= 63 and at most one entry is g's own, so V lies in the first
        // k + 1 lanes of this step.  Lane by lane in list order, every lane compares its label with that lane's; one
        // popcount is the label's number of entries in V.  A larger number wins; among equal numbers the label met
        // first stays, because its first entry was the earlier lane.
        const unsigned long long v = __ballot(entry && (uint32_t)__popcll(in & below) < a.k);
        const bool in_v = (v >> lane) & 1ull;
        const uint32_t lanes = min(min(a.k + 1u, 64u), len);
        uint32_t win = 64;
        for (uint32_t j = 0; j < lanes; ++j) {
          if (!((v >> j) & 1ull)) continue;   // (v is the wavefront's: g's own lane, or a bad entry)
          const uint32_t lab_j = (uint32_t)__shfl((int)lab, (int)j, 64);
          const uint32_t n = (uint32_t)__popcll(__ballot(in_v && lab == lab_j));
          if (n > vote_n) {
            vote_n = n;
            win = j;
          }
        }
        if (win < 64) vote_g = (uint32_t)__shfl((int)gid, (int)win, 64);
      }
      // the first entry under g's label and the first under another one, where this step holds them
      const unsigned long long own_m = __ballot(entry && lab == mine), oth_m = in & ~own_m;
      if (!own_found && own_m) {
        const int at = __ffsll((long long)own_m) - 1;
        own_c = (uint32_t)__shfl((int)cnt, at, 64);
        own_g = (uint32_t)__shfl((int)gid, at, 64);
        own_found = true;
      }
      if (!oth_found && oth_m) {
        const int at = __ffsll((long long)oth_m) - 1;
        oth_c = (uint32_t)__shfl((int)cnt, at, 64);
        oth_g = (uint32_t)__shfl((int)gid, at, 64);
        oth_found = true;
      }
      if (own_found && oth_found) break;
    }
    if (lane == 0) {
      if (a.verdict) a.verdict[g] = audit_verdict(own_c, oth_c);
      if (a.own_count) a.own_count[g] = own_c;
      if (a.own_gid) a.own_gid[g] = own_g;
      if (a.other_count) a.other_count[g] = oth_c;
      if (a.other_gid) a.other_gid[g] = oth_g;
      if (a.vote_gid) a.vote_gid[g] = vote_g;
      if (a.vote_n) a.vote_n[g] = vote_n;
    }
  }
  if (bad) atomicAdd(a.info + kAuditInfoBad, bad);
}

}  // namespace

hipError_t launch_audit(const AuditArgs &a, hipStream_t stream) {
  if (a.nq == 0) return hipSuccess;
  // four lists a workgroup and turn; no more workgroups than keep every compute unit full
  const uint32_t blocks = std::min<uint32_t>((a.nq + kAuditWaves - 1) / kAuditWaves, 256u * 8u);
  hipLaunchKernelGGL(audit_kernel, dim3(blocks), dim3(kAuditBlock), 0, stream, a);
  return hipGetLastError();
}

}  // namespace nq
