// size_estimate.h -- a sketch's number of distinct k-mers from its register histogram (niqki_registers,
// niqki_sketch_registers, niqki_staged_registers), and the containment of two sketches from their co-occurrence count
// and their sizes.  Plain host arithmetic, no engine call: everything the device delivers is an integer.  Mirrored
// operation for operation in niqki_amd/size_estimate.py; DESIGN.md 4.6j.
//
// The top H bits of a cell are r = max(0, 2^H - 1 - leading zeros of the k-mer's hash), and a slot keeps the smallest
// fingerprint it has seen, so the most leading zeros: a HyperLogLog register whose rank is 2^H - r.  hist[r] counts the
// valid cells with register r, hist[2^H] the cells that are not valid (an empty register, rank 0).
//   Z = hist[2^H] + sum over r of hist[r] * 2^-(2^H - r)     (summed in ascending r; every term is exact)
//   E = alpha * F^2 / Z,  alpha = 0.7213 / (1 + 1.079 / F), the standard constants 0.673, 0.697, 0.709 at F = 16, 32, 64
// Range.  The store holds DENSIFIED sketches: an empty slot took a neighbour's cell, so a genome with fewer than about
// 8 F k-mers looks larger than it is (1024 k-mers at F = 4096 estimate as 10 237) -- `below`, whatever E says; the
// empty count before densification is in neither the store nor the dump format.  A register saturates at r = 0: with
// more than an eighth of them there the estimate runs low (bias under 2 % up to a share of 0.22, -5 % at 0.39 with
// H = 3, S = 10) -- `above`.  H < 2 or S < 4 hold too little to say: always `below`.
#pragma once
#include <cmath>
#include <cstdint>

namespace nqsize {

enum Status { OK = 0, BELOW = 1, ABOVE = 2 };

inline const char *status_text(Status s) { return s == OK ? "ok" : s == BELOW ? "below" : "above"; }

struct Estimate {
  double kmers;
  Status status;
};

// hist: NIQKI_REGISTER_BINS(H) = 2^H + 1 counts that sum to F = 2^S; H <= 6
inline Estimate estimate(const uint32_t *hist, uint32_t S, uint32_t H) {
  const uint32_t n_reg = 1u << H;
  const double F = (double)(1u << S);
  double Z = (double)hist[n_reg];
  for (uint32_t r = 0; r < n_reg; ++r) Z += std::ldexp((double)hist[r], -(int)(n_reg - r));
  if (!(Z > 0)) return {0.0, BELOW};
  const double alpha = S >= 7 ? 0.7213 / (1.0 + 1.079 / F) : S == 6 ? 0.709 : S == 5 ? 0.697 : 0.673;
  const double E = alpha * F * F / Z;
  if (H < 2 || S < 4 || E < 8.0 * F) return {E, BELOW};
  if ((uint64_t)hist[0] * 8u > (uint64_t)1 << S) return {E, ABOVE};
  return {E, OK};
}

struct Containment {
  bool defined;      // both sizes ok
  double jaccard;    // count / F
  double cq, cg;     // the share of the query's k-mers found in the genome, of the genome's found in the query
};

// count: slots in which the two sketches agree; q, g: the two estimates
inline Containment containment(uint32_t count, uint32_t S, const Estimate &q, const Estimate &g) {
  Containment c{q.status == OK && g.status == OK, (double)count / (double)(1u << S), 0.0, 0.0};
  if (!c.defined) return c;
  const double I = c.jaccard * (q.kmers + g.kmers) / (1.0 + c.jaccard);   // |A n B| = J (|A| + |B|) / (1 + J)
  c.cq = I / q.kmers < 1.0 ? I / q.kmers : 1.0;
  c.cg = I / g.kmers < 1.0 ? I / g.kmers : 1.0;
  return c;
}

}  // namespace nqsize
