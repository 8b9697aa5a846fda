// nq_sketch_lines.h -- chunk geometry of the line-aligned sketch loop (nq_sketch.hip, roll_records_lines).
//
// A record's k-mer i is hashed when base i + K - 1 comes in: its HASH BYTE.  The hash bytes of a record part are
// dealt to the lanes of a workgroup in whole 128-byte lines of the address space (a line = the bytes with the same
// address >> 7), one contiguous run of lines per lane: no two lanes' hash steps share a line, every chunk boundary
// but the record's own two ends is a line boundary, and a lane fetches each of its lines once, whole.  The sketch is a
// per-slot minimum over k-mers, so any partition gives the same bits.
//
// Lines are balanced per SIMD, not per lane (wave w runs on SIMD w % 4 and a wave steps as long as its longest
// lane): m lines over B lanes is m / B each, and the m % B extra lines go to the four SIMDs in shares that differ
// by at most one, each SIMD filling its waves one after the other (so the fewest waves run an extra line).
//
// Host and device share this code: the kernel calls it per record, tests/test_sketch_lines_geometry.py compiles it
// with g++ and checks the partition and the load bounds.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define NQ_HD __host__ __device__ __forceinline__
#else
#define NQ_HD inline
#endif

namespace nq {

constexpr uint32_t kLineLog2 = 7;                 // 128-byte lines: the L2's line and the fabric's request size
constexpr uint64_t kLineBytes = 1ull << kLineLog2;
constexpr uint32_t kLineWarmBytes = 32;           // a warm-up loads exactly this many bytes
constexpr uint32_t kLineFastKMax = 31;            // largest K of the line loop (a warm-up's K - 1 bases fit its 32 bytes)

struct LaneLines {
  uint64_t line0;        // first line (address >> 7) of the lane's run
  uint32_t n_lines;      // lines in the run (0: the lane has no part in this record)
  uint64_t first_kmer;   // index in the record of the first k-mer the lane hashes
  uint64_t count;        // k-mers the lane hashes
  uint64_t hash_lo;      // addresses of the lane's hash bytes: [hash_lo, hash_hi)
  uint64_t hash_hi;
  uint64_t warm_start;   // address of the 32 bytes the lane's warm-up loads
  uint32_t warm_fast;    // 1: 30 plain rolling steps from warm_start; 0: K - 1 steps with the record's prefix rules
};

// ---- every address the kernel loads from is one of these (the CPU test walks them all against the buffer) ----
// Warm-up: 32 bytes.  A wave takes the fast form only if all its lanes with lines can; beside a lane that cannot, a
// fast lane runs the K - 1 steps as well, over the last K - 1 of its 30 bases.
NQ_HD uint64_t warm_load(const LaneLines &g, uint32_t K, bool wave_fast) {
  return (g.warm_fast && !wave_fast) ? g.warm_start + (30u - (K - 1u)) : g.warm_start;
}
// ... and, in the K - 1-step form, the record's first 32 bytes (the prefix rules) for a lane that starts inside the prefix
NQ_HD bool reads_prefix(const LaneLines &g, uint32_t K) { return g.first_kmer < K - 1u; }
// Round rd (0 .. the wave's longest run): the 128 bytes at this address -- the lane's line, or the record's first
// bytes where it has none in this round (its lanes still take part in the wave's loads; the bytes are not used)
NQ_HD uint64_t round_line(const LaneLines &g, uint32_t rd, uint64_t rec_addr) {
  return rd < g.n_lines ? (g.line0 + rd) << kLineLog2 : rec_addr;
}
// ... fetched whole if all of it lies inside the buffer [buf_lo, buf_hi) (and the same holds for the wave's other lanes),
// else as eight 16-byte pieces, piece x from this address: x itself, or the nearest 16 bytes inside the buffer (which holds
// its 64-byte pad at least).  The piece is then moved back by the difference; bytes from outside are never hash bytes.
NQ_HD bool line_inside(uint64_t line, uint64_t buf_lo, uint64_t buf_hi) { return line >= buf_lo && line + kLineBytes <= buf_hi; }
NQ_HD uint64_t clamp_piece(uint64_t x, uint64_t buf_lo, uint64_t buf_hi) {
  return x < buf_lo ? buf_lo : x + 16u > buf_hi ? buf_hi - 16u : x;
}

// The share of lane l of wave w of m lines over a workgroup of `block` lanes (a multiple of 256): lines [start, start + n).
NQ_HD void deal_lines(uint64_t m, uint32_t block, uint32_t w, uint32_t l, uint64_t &start, uint32_t &n) {
  const uint64_t q = m / block;
  const uint32_t r = (uint32_t)(m % block);
  uint32_t before = 0, mine = 0;
  for (uint32_t v = 0; v <= w; ++v) {
    const uint32_t s = v & 3u, j = v >> 2;               // wave v is the j-th wave of SIMD s
    const uint32_t es = r / 4u + (s < r % 4u ? 1u : 0u);   // the SIMD's extra lines
    const uint32_t x = es > 64u * j ? (es - 64u * j < 64u ? es - 64u * j : 64u) : 0u;
    if (v < w) before += x; else mine = x;
  }
  start = q * (64u * w + l) + before + (l < mine ? l : mine);
  n = (uint32_t)q + (l < mine ? 1u : 0u);
}

// seqs: address of the buffer; [b0, b1): the record's offsets in it (b1 - b0 > K).
NQ_HD LaneLines lane_lines(uint64_t seqs, uint64_t b0, uint64_t b1, uint32_t K,
                           uint32_t splits, uint32_t part, uint32_t block, uint32_t wave, uint32_t lane) {
  LaneLines g;
  const uint64_t A0 = seqs + b0, len = b1 - b0;
  const uint64_t H0 = A0 + K - 1u, H1 = A0 + len - 1u;   // hash bytes of the record (its last k-mer is skipped)
  const uint64_t La = H0 >> kLineLog2, Lb = (H1 + kLineBytes - 1u) >> kLineLog2, n = Lb - La;
  const uint64_t pa = La + n * part / splits, pb = La + n * (part + 1u) / splits;
  uint64_t start;
  deal_lines(pb - pa, block, wave, lane, start, g.n_lines);
  g.line0 = pa + start;
  if (g.n_lines == 0) {
    g.first_kmer = g.count = 0;
    g.hash_lo = g.hash_hi = H0;
    g.warm_start = A0;   // (it warms up on the record's first bytes, for nothing)
    g.warm_fast = 0;
    return g;
  }
  const uint64_t c0 = g.line0 << kLineLog2, c1 = (g.line0 + g.n_lines) << kLineLog2;
  g.hash_lo = c0 > H0 ? c0 : H0;
  g.hash_hi = c1 < H1 ? c1 : H1;
  g.first_kmer = g.hash_lo - H0;
  g.count = g.hash_hi - g.hash_lo;
  // warm-up: the K - 1 bases before the first hash byte.  The fast form takes 30 steps whatever K (K <= 31: it
  // starts 31 - K bases further back) and needs all 30 behind the record's K - 1 prefix positions, that is
  // position first_kmer + K - 1 - 30 >= K - 1
  g.warm_fast = (K <= kLineFastKMax && g.first_kmer >= 30u) ? 1u : 0u;
  g.warm_start = g.warm_fast ? g.hash_lo - 30u : g.hash_lo - (K - 1u);
  return g;
}

// ---- leveling a SIMD's four waves ----
// The issue arbiter serves a SIMD's waves by priority, then age: left alone, the oldest wave of a SIMD runs ahead and
// the youngest ends the workgroup alone, at a rate one wave cannot keep up (a lane is one dependent chain).  So every
// wave publishes how far it is through the entry, on a scale all waves share, and takes the top priority while it is
// the one furthest behind on its SIMD.  Nothing waits on these words: a stale one costs a priority, never a result.
//
// PROGRESS: the hash bytes of the entry (all parts') in the records the wave is through plus the line rounds it is
// through in the current one, a round of a part standing for block * splits lines of the record; in steps of
// 2^shift bytes, 32 to 63 of them over the entry's n hash bytes.  Wave-uniform, never falls, and after the last
// record it is n >> shift for every wave.
constexpr uint32_t kLevelDone = 0xFFFFFFFFu;   // the word of a wave that has left the loop
constexpr uint32_t kLevelWords = 16;           // one word per wave of the 1024-lane workgroup
NQ_HD uint32_t level_shift(uint64_t n) { return n >= 64u ? 58u - (uint32_t)__builtin_clzll(n) : 0u; }
// the bytes of a record that `rounds` line rounds of a part stand for
NQ_HD uint64_t level_round_bytes(uint32_t rounds, uint32_t block, uint32_t splits) { return ((uint64_t)rounds * block * splits) << kLineLog2; }
// rec_n: the current record's hash bytes; rounds: line rounds of it the wave is through (a wave without lines in a
// record never gets here: the record goes into done_recs at once)
NQ_HD uint32_t level_progress(uint64_t done_recs, uint64_t rec_n, uint32_t rounds, uint32_t block, uint32_t splits, uint32_t shift) {
  const uint64_t in = level_round_bytes(rounds, block, splits);
  return (uint32_t)((done_recs + (in < rec_n ? in : rec_n)) >> shift);
}
// The bytes into the current record (rounds * block * splits lines) at which the progress leaves p, the value
// level_progress() has now: the next step boundary.  All ones: none before the record's end.
NQ_HD uint64_t level_next(uint64_t done_recs, uint64_t rec_n, uint32_t p, uint32_t shift) {
  const uint64_t t = (((uint64_t)p + 1u) << shift) - done_recs;
  return t > rec_n ? ~0ull : t;
}
// the word of wave w among the sixteen: the four waves of SIMD w % 4 side by side
NQ_HD uint32_t level_word(uint32_t w) { return (w & 3u) * 4u + (w >> 2); }
// THE RULE: 3 for the wave (or waves) at the least progress among those of the SIMD still in the loop, one level
// less per step of lead, down to 0.  simd[]: the SIMD's four words, this wave's among them (kLevelDone is the
// largest word, so a wave that has left is never the least); mine: this wave's progress (not kLevelDone).
NQ_HD uint32_t level_prio(uint32_t mine, const uint32_t simd[4]) {
  uint32_t least = mine;
  for (int i = 0; i < 4; ++i) least = simd[i] < least ? simd[i] : least;
  const uint32_t lead = mine - least;
  return lead < 3u ? 3u - lead : 0u;
}

}  // namespace nq
