"""Leveling of a SIMD's four waves in the line-aligned sketch loop (niqki_amd/csrc/nq_sketch_lines.h), on the CPU: the
priority rule level_prio() over random progress words, and the progress scale level_progress() walked along the rounds
the kernel runs for lane_lines() geometries.  The header is the code the kernel runs, compiled here with g++."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r"""
#include <algorithm>
#include <cstdio>
#include <cstdint>
#include <vector>
#include "nq_sketch_lines.h"

static uint64_t rng_state = 0x2545F4914F6CDD1Dull;
static uint64_t rnd() {
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
#define FAIL(...) do { printf("FAIL case %d: ", cs); printf(__VA_ARGS__); printf("\n"); return 1; } while (0)

// ---- the rule ----
static int rule() {
  for (int cs = 0; cs < 200000; ++cs) {
    // words close together (leads of 0..5 steps), far apart, or anything; some waves have left the loop
    uint32_t w[4];
    const uint32_t base = cs % 3 == 0 ? (uint32_t)rnd() % 0xFFFFFFF0u : (uint32_t)(rnd() % 64);
    for (int i = 0; i < 4; ++i) {
      w[i] = cs % 3 == 2 ? (uint32_t)(rnd() % 0xFFFFFFFFull) : base + (uint32_t)(rnd() % (cs % 2 ? 6 : 2));
      if (rnd() % 4 == 0) w[i] = nq::kLevelDone;
    }
    uint32_t least = nq::kLevelDone;
    for (int i = 0; i < 4; ++i) least = std::min(least, w[i]);
    uint32_t pr[4];
    int running = 0;
    for (int i = 0; i < 4; ++i) {
      if (w[i] == nq::kLevelDone) continue;
      ++running;
      pr[i] = nq::level_prio(w[i], w);
      if (pr[i] > 3u) FAIL("priority %u", pr[i]);
      if (w[i] == least && pr[i] != 3u) FAIL("a wave at the least progress gets %u", pr[i]);
      const uint32_t lead = w[i] - least;
      if (pr[i] != (lead < 3u ? 3u - lead : 0u)) FAIL("lead %u gets %u", lead, pr[i]);
      // the order of the other three words does not matter
      uint32_t o[4] = {w[0], w[1], w[2], w[3]};
      std::sort(o, o + 4);
      do {
        if (nq::level_prio(w[i], o) != pr[i]) FAIL("depends on the order of the words");
      } while (std::next_permutation(o, o + 4));
    }
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 4; ++j)
        if (w[i] != nq::kLevelDone && w[j] != nq::kLevelDone && w[i] > w[j] && pr[i] > pr[j]) FAIL("the wave further ahead gets the higher priority");
    if (running == 1)
      for (int i = 0; i < 4; ++i)
        if (w[i] != nq::kLevelDone && pr[i] != 3u) FAIL("a wave alone gets %u", pr[i]);
  }
  // a wave alone on its SIMD, whatever its progress, and whatever word it reads for itself (a stale one included)
  for (int cs = 0; cs < 1000; ++cs) {
    const uint32_t mine = (uint32_t)(rnd() % 0xFFFFFFFFull);
    uint32_t w[4] = {nq::kLevelDone, nq::kLevelDone, nq::kLevelDone, nq::kLevelDone};
    if (nq::level_prio(mine, w) != 3u) FAIL("alone, own word not seen");
    w[rnd() % 4] = mine;
    if (nq::level_prio(mine, w) != 3u) FAIL("alone");
  }
  return 0;
}

// ---- progress along the rounds of the kernel's loop ----
// The walk is the kernel's: per record with k-mers, a wave that has lines runs nl_max rounds (its longest lane's run) and
// looks at its progress at the head of every round; then the record counts as done, as it does at once for a wave
// without lines in it.
static int progress() {
  const uint32_t block = 1024;
  const uint32_t split_set[] = {1, 2, 3, 32};
  const uint64_t len_set[] = {40, 130, 3000, 131072 + 97, 200001, (1ull << 21) + 5, (1ull << 21) + 77, 5000000, (1ull << 22) + 640 + 31};
  for (int cs = 0; cs < 40; ++cs) {
    const uint32_t K = 17 + (uint32_t)(rnd() % 15);
    const uint64_t seqs = 0x7f0000000000ull + (rnd() % 4096) * 128 + rnd() % 128;
    const uint32_t splits = cs < 4 ? 1u : split_set[rnd() % 4];
    const uint32_t n_rec = cs == 0 ? 1u : cs == 1 ? 5u : 1 + (uint32_t)(rnd() % 5);
    std::vector<uint64_t> off(n_rec + 1, 0);
    uint64_t n = 0;
    for (uint32_t r = 0; r < n_rec; ++r) {
      uint64_t len = len_set[rnd() % 9] + rnd() % 3;
      if (rnd() % 7 == 0) len = K;   // no k-mer
      if (cs == 1) { const uint64_t fixed[5] = {(1ull << 21) + 5, 40, 3000, 130, (1ull << 21) + 1}; len = fixed[r]; }
      off[r + 1] = off[r] + len;
      if (len > K) n += len - K;
    }
    const uint32_t shift = nq::level_shift(n);
    const uint32_t last = (uint32_t)(n >> shift);
    if (n >= 32 && (last < 32u || last > 63u)) FAIL("%u steps over %llu hash bytes", last, (unsigned long long)n);
    for (uint32_t part = 0; part < splits; ++part) {
      for (uint32_t w = 0; w < 16; ++w) {
        uint64_t done = 0;
        uint32_t p_last = 0;
        for (uint32_t r = 0; r < n_rec; ++r) {
          const uint64_t b0 = off[r], b1 = off[r + 1];
          if (b1 - b0 <= K) continue;
          const uint64_t rec_n = b1 - b0 - K;
          uint32_t nl_max = 0;
          for (uint32_t l = 0; l < 64; ++l) nl_max = std::max(nl_max, nq::lane_lines(seqs, b0, b1, K, splits, part, block, w, l).n_lines);
          uint64_t next = 0;        // (the kernel looks at a record's first round whatever it brings)
          uint32_t p_seen = 0;
          for (uint32_t rd = 0; rd < nl_max; ++rd) {
            // (wave-uniform by construction: no argument is a lane's)
            const uint32_t p = nq::level_progress(done, rec_n, rd, block, splits, shift);
            // the kernel computes the progress only in the rounds level_next() names: it misses no step, and but for a
            // record's first round it looks only where the progress has moved
            if (nq::level_round_bytes(rd, block, splits) >= next) {
              if (rd && p == p_seen) FAIL("a look without a step (wave %u record %u round %u)", w, r, rd);
              p_seen = p;
              next = nq::level_next(done, rec_n, p, shift);
            } else if (p != p_seen) FAIL("step to %u missed (wave %u record %u round %u)", p, w, r, rd);
            if (p < p_last) FAIL("progress falls from %u to %u (wave %u record %u round %u)", p_last, p, w, r, rd);
            if (p > last) FAIL("progress %u beyond the entry's %u", p, last);
            if (p == nq::kLevelDone) FAIL("progress equals the sentinel");
            p_last = p;
          }
          // the rounds of a record never count for more than the record
          if (nl_max && nq::level_progress(done, rec_n, nl_max, block, splits, shift) > (uint32_t)((done + rec_n) >> shift)) FAIL("rounds beyond the record");
          // ... and a wave's rounds (one more than its neighbours' at most) reach the record's end but for the last round's share
          if (nl_max && (((uint64_t)(nl_max + 1) * block * splits) << 7) < rec_n) FAIL("wave %u ends record %u %u rounds in, far from its end", w, r, nl_max);
          done += rec_n;
        }
        const uint32_t p_end = nq::level_progress(done, 0, 0, block, splits, shift);
        if (p_end < p_last) FAIL("progress falls at the end");
        if (p_end != last || done != n) FAIL("ends at %u, not at its maximum %u", p_end, last);
      }
    }
  }
  // the sixteen words: four per SIMD side by side, every word once
  int cs = -1;
  bool used[16] = {};
  for (uint32_t w = 0; w < 16; ++w) {
    const uint32_t x = nq::level_word(w);
    if (x >= nq::kLevelWords || used[x]) FAIL("word of wave %u", w);
    if (x / 4 != (w & 3u)) FAIL("wave %u not in the row of SIMD %u", w, w & 3u);
    used[x] = true;
  }
  return 0;
}

int main() {
  if (rule()) return 1;
  if (progress()) return 1;
  printf("ok\n");
  return 0;
}
"""


def test_level_rule_and_progress(tmp_path):
    """level_prio(): a value in 0..3; 3 for every wave at the least progress among the words that are not the sentinel;
    never more for a wave further ahead than for one less far ahead; sentinels ignored, so a wave alone gets 3; the same
    for every order of the SIMD's words.  level_progress(): along the rounds of lane_lines() geometries (several
    records, records in which most waves have no lines, records without k-mers, splits) it never falls, never passes or
    equals the sentinel, ends at the entry's n >> shift for every wave, and takes no argument that differs between the
    lanes of a wave; the scale has 32 to 63 steps.  level_next() names exactly the rounds in which the progress moves."""
    src = tmp_path / "level.cpp"
    src.write_text(SRC)
    exe = tmp_path / "level"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "niqki_amd", "csrc"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
