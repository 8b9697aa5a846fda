"""Chunk geometry of the line-aligned sketch loop (niqki_amd/csrc/nq_sketch_lines.h), on the CPU: the header is the
code the kernel runs, compiled here with g++ and driven over random buffer addresses, record sets, splits and K."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r"""
#include <cstdio>
#include <cstdint>
#include <vector>
#include "nq_sketch_lines.h"
#include "niqki_hip.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
#define FAIL(...) do { printf("FAIL case %d rec %u part %u tid %u: ", cs, r, part, tid); printf(__VA_ARGS__); printf("\n"); return 1; } while (0)

int main() {
  const uint32_t block = 1024, pad = NIQKI_SEQ_PAD;
  const uint32_t split_set[] = {1, 2, 3, 7, 32};
  // lengths around the sizes where the deal changes: a few lines, one per lane, one per lane and a rest, many
  const uint64_t len_set[] = {0, 40, 127, 128, 129, 300, 4000, 131072 - 31, 131072, 131072 + 97, 200001, 5000000, (1ull << 21) + 63};
  for (int cs = 0; cs < 60; ++cs) {
    const uint32_t K = 17 + (uint32_t)(rnd() % 15);                       // 17..31
    const uint64_t seqs = 0x7f0000000000ull + (rnd() % 4096) * 128 + (cs % 3 == 0 ? rnd() % 128 : (cs % 3 == 1 ? 1 + 60 * (rnd() % 3) : 127));
    const uint32_t splits = split_set[rnd() % 5];
    const uint32_t n_rec = 1 + (uint32_t)(rnd() % 4);
    std::vector<uint64_t> off(n_rec + 1, 0);
    for (uint32_t r = 0; r < n_rec; ++r) {
      uint64_t len = rnd() % 3 == 0 ? K + rnd() % 200 : len_set[rnd() % 13] + rnd() % 3;
      if (cs == 0) len = K + 1;                                          // one k-mer
      off[r + 1] = off[r] + len;
    }
    const uint64_t buf_lo = seqs, buf_hi = seqs + off[n_rec] + pad;
    for (uint32_t r = 0; r < n_rec; ++r) {
      const uint64_t b0 = off[r], b1 = off[r + 1], len = b1 - b0;
      uint32_t part = 0, tid = 0;
      if (len <= K) continue;
      const uint64_t n_kmers = len - K, H0 = seqs + b0 + K - 1;
      uint64_t next_kmer = 0, next_line = H0 >> 7;
      for (part = 0; part < splits; ++part) {
        uint64_t simd_lines[4] = {0, 0, 0, 0}, simd_rounds[4] = {0, 0, 0, 0};
        uint32_t wave_max = 0;
        // the wave's decisions first: its longest run, and whether it takes the fast warm-up
        uint32_t wave_rounds[16]; bool wave_fast[16];
        for (uint32_t w = 0; w < 16; ++w) {
          wave_rounds[w] = 0; wave_fast[w] = true;
          for (uint32_t l = 0; l < 64; ++l) {
            const nq::LaneLines g = nq::lane_lines(seqs, b0, b1, K, splits, part, block, w, l);
            wave_rounds[w] = g.n_lines > wave_rounds[w] ? g.n_lines : wave_rounds[w];
            wave_fast[w] = wave_fast[w] && (g.warm_fast || g.n_lines == 0);
          }
        }
        for (tid = 0; tid < block; ++tid) {
          const nq::LaneLines g = nq::lane_lines(seqs, b0, b1, K, splits, part, block, tid >> 6, tid & 63);
          if ((g.n_lines != 0) != (g.count != 0)) FAIL("lines %u but %llu k-mers", g.n_lines, (unsigned long long)g.count);
          // EVERY load of the lane, as the kernel forms it, against the bound the kernel has: the end of the sketch's own
          // records plus the pad (never laxer than the buffer's; here the record's own end, the tightest it can be)
          const uint64_t lim = seqs + b1 + pad;
          if (lim > buf_hi) FAIL("bound");
          if (wave_rounds[tid >> 6]) {
            const uint64_t w0 = nq::warm_load(g, K, wave_fast[tid >> 6]);
            if (w0 < buf_lo || w0 + 32 > lim) FAIL("warm-up load outside the buffer");
            if (g.n_lines && (w0 < seqs + b0 || w0 + (wave_fast[tid >> 6] ? 30 : K - 1) != g.hash_lo)) FAIL("warm-up bytes do not end at the first hash byte");
            if (!wave_fast[tid >> 6] && nq::reads_prefix(g, K) && seqs + b0 + 32 > lim) FAIL("prefix load outside the buffer");
            for (uint32_t rd = 0; rd < wave_rounds[tid >> 6]; ++rd) {
              const uint64_t line = nq::round_line(g, rd, seqs + b0);
              if (rd < g.n_lines && (line & 127)) FAIL("line not aligned");
              for (uint32_t q = 0; q < 8; ++q) {
                const uint64_t x = line + 16 * q;
                const uint64_t c = nq::line_inside(line, buf_lo, lim) ? x : nq::clamp_piece(x, buf_lo, lim);
                if (c < buf_lo || c + 16 > lim) FAIL("piece %u of round %u loads outside the buffer", q, rd);
                // a hash byte of the lane inside this piece must come from its own address: it is inside the loaded 16 bytes
                if (rd < g.n_lines)
                  for (uint64_t a = x; a < x + 16; ++a)
                    if (a >= g.hash_lo && a < g.hash_hi && (a < c || a >= c + 16)) FAIL("hash byte not loaded");
              }
            }
          }
          if (g.n_lines) {
            if (g.line0 != next_line) FAIL("line run starts at %llu, expected %llu", (unsigned long long)g.line0, (unsigned long long)next_line);
            next_line += g.n_lines;
            if (g.first_kmer != next_kmer) FAIL("first k-mer %llu, expected %llu", (unsigned long long)g.first_kmer, (unsigned long long)next_kmer);
            next_kmer += g.count;
            if (g.hash_lo != H0 + g.first_kmer || g.hash_hi != g.hash_lo + g.count) FAIL("hash bytes do not match the k-mers");
            if ((g.hash_lo >> 7) != g.line0 || ((g.hash_hi - 1) >> 7) != g.line0 + g.n_lines - 1) FAIL("hash bytes outside the lines");
            if (g.warm_fast ? (g.warm_start + 30 != g.hash_lo || g.first_kmer < 30) : (g.warm_start + K - 1 != g.hash_lo)) FAIL("warm-up window");
          }
          simd_lines[(tid >> 6) & 3] += g.n_lines;
          wave_max = g.n_lines > wave_max ? g.n_lines : wave_max;
          if ((tid & 63) == 63) { simd_rounds[(tid >> 6) & 3] += wave_max; wave_max = 0; }
        }
        for (int a = 0; a < 4; ++a)
          for (int b = 0; b < 4; ++b) {
            if (simd_lines[a] > simd_lines[b] + 1) FAIL("SIMD %d has %llu lines, SIMD %d %llu", a, (unsigned long long)simd_lines[a], b, (unsigned long long)simd_lines[b]);
            if (simd_rounds[a] > simd_rounds[b] + 1) FAIL("SIMD %d runs %llu rounds, SIMD %d %llu", a, (unsigned long long)simd_rounds[a], b, (unsigned long long)simd_rounds[b]);
          }
      }
      part = tid = 0;
      if (next_kmer != n_kmers) FAIL("%llu of %llu k-mers dealt", (unsigned long long)next_kmer, (unsigned long long)n_kmers);
    }
  }
  printf("ok\n");
  return 0;
}
"""


def test_lane_geometry_partitions_records_inside_the_buffer(tmp_path):
    """Over random cases: the lanes' k-mer ranges partition each record exactly (in lane order, part by part), every
    lane's lines are one contiguous run, every load the kernel forms from the header's helpers (warm-up, prefix, the
    eight pieces of every round's line, clamped where the line is not inside) lies inside [seqs, seqs + end of the
    record + pad) and holds the lane's hash bytes of that piece, and the
    lines (and the rounds the waves run) of the four SIMDs differ by at most one."""
    src = tmp_path / "geom.cpp"
    src.write_text(SRC)
    exe = tmp_path / "geom"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "niqki_amd", "csrc"),
                           "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
