"""Block arithmetic of the store compaction behind niqki_retain (niqki_amd/csrc/nq_retain_blocks.h), on the CPU: the
header is the code the kernels run.  It is compiled here with g++ into a restatement of the kernel's row loop -- per
block of 4 096 source columns the ranks from the keep words, the image at off + rank, then whole 16-byte pieces and
single elements out along the destination's grid -- and driven over the designed masks of tests/retain_masks.py (the
masks the GPU test runs).  The compacted row must be what plain numpy indexing gives."""
import os
import subprocess

import numpy as np
import pytest

from retain_masks import SIZES, designed_masks, expected_ids

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r"""
#include <cstdio>
#include <cstdint>
#include <vector>
#include "nq_retain_blocks.h"

#define FAIL(...) do { printf("FAIL mask %u block %u: ", mk, b); printf(__VA_ARGS__); printf("\n"); return 1; } while (0)

// in: u32 n, u32 n_masks, then n_masks x n flag bytes.  out: per mask u32 n_kept, n x u32 new ids, n_kept x u16 row
int main(int argc, char **argv) {
  FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
  uint32_t n = 0, n_masks = 0, b = 0;
  if (!in || !out || fread(&n, 4, 1, in) != 1 || fread(&n_masks, 4, 1, in) != 1) return 2;
  std::vector<uint8_t> keep(n);
  std::vector<uint16_t> src((n + 63) / 64 * 64);
  for (uint32_t c = 0; c < src.size(); ++c) src[c] = (uint16_t)(c * 7 + 1);
  const uint32_t n_blocks = (n + nq::kRetainBlock - 1) / nq::kRetainBlock;
  for (uint32_t mk = 0; mk < n_masks; ++mk) {
    if (fread(keep.data(), 1, n, in) != n) return 2;
    // the rank pass: keep words, kept counts, their exclusive prefix
    std::vector<uint64_t> words((size_t)n_blocks * nq::kRetainWords, 0);
    std::vector<uint32_t> blk_dst(n_blocks + 1, 0);
    for (uint32_t c = 0; c < n; ++c)
      if (keep[c]) { words[c >> 6] |= 1ull << (c & 63); blk_dst[c / nq::kRetainBlock + 1] += 1; }
    for (b = 0; b < n_blocks; ++b) blk_dst[b + 1] += blk_dst[b];
    const uint32_t total = blk_dst[n_blocks];
    const uint64_t cap = nq::retain_cap(total);
    const uint64_t least = total < 64 ? 64 : total;
    if (cap % 64 || cap < least || cap >= least + 64) { b = 0; FAIL("capacity %llu for %u", (unsigned long long)cap, total); }
    std::vector<uint16_t> dst(cap, 0);
    std::vector<uint8_t> written(cap, 0), whole(cap / 8, 0);
    std::vector<uint32_t> ids(n, 0xFFFFFFFFu);
    for (b = 0; b < n_blocks; ++b) {
      const uint32_t dst0 = blk_dst[b], kept = blk_dst[b + 1] - dst0;
      const uint64_t *w = words.data() + (size_t)b * nq::kRetainWords;
      uint32_t word_rank[nq::kRetainWords], run = 0;
      for (uint32_t i = 0; i < nq::kRetainWords; ++i) { word_rank[i] = run; run += (uint32_t)__builtin_popcountll(w[i]); }
      if (run != kept) FAIL("kept count");
      for (uint32_t i = 0; i < nq::kRetainBlock && (uint64_t)b * nq::kRetainBlock + i < n; ++i)
        if ((w[i >> 6] >> (i & 63)) & 1) ids[b * nq::kRetainBlock + i] = dst0 + nq::retain_rank(w, word_rank, i);
      if (kept == 0) continue;                          // such a block reads nothing
      const nq::RetainSpan sp = nq::retain_span(dst0, kept);
      if (sp.off != dst0 % 8 || sp.end != sp.off + kept || sp.end > nq::kRetainImage) FAIL("span");
      if (sp.whole_lo > sp.whole_hi || sp.whole_hi > sp.pieces || sp.pieces * 8 > nq::kRetainImage + 7) FAIL("pieces");
      // the image: a thread's group of 8 columns goes to off + rank of its first column, kept elements in order
      std::vector<uint16_t> img(nq::kRetainImage, 0xDEAD);
      std::vector<uint8_t> filled(nq::kRetainImage, 0);
      for (uint32_t j = 0; j < nq::kRetainBlock / 8; ++j) {
        const uint32_t c = j * 8, m = (uint32_t)(w[c >> 6] >> (c & 63)) & 0xFF;
        uint32_t at = sp.off + nq::retain_rank(w, word_rank, c);
        if (m && (uint64_t)b * nq::kRetainBlock + c + 8 > src.size()) FAIL("group %u loads beyond the source's capacity", j);
        for (uint32_t e = 0; e < 8; ++e)
          if ((m >> e) & 1) {
            if (at >= nq::kRetainImage || filled[at]) FAIL("image element %u", at);
            filled[at] = 1;
            img[at++] = src[(size_t)b * nq::kRetainBlock + c + e];
          }
      }
      for (uint32_t i = 0; i < nq::kRetainImage; ++i)
        if (filled[i] != (i >= sp.off && i < sp.end)) FAIL("image fill at %u", i);
      const uint64_t d0 = dst0 - sp.off;                // destination column of image element 0
      if (d0 % 8) FAIL("image not on the destination's grid");
      for (uint32_t p = 0; p < sp.pieces; ++p) {
        if (p >= sp.whole_lo && p < sp.whole_hi) {
          if (d0 + p * 8 + 8 > cap) FAIL("16-byte store beyond the capacity");
          if (whole[(d0 >> 3) + p]++) FAIL("piece stored whole twice");
          for (uint32_t i = p * 8; i < p * 8 + 8; ++i) {
            if (i < sp.off || i >= sp.end) FAIL("whole piece %u leaves the block's range", p);
            if (written[d0 + i]++) FAIL("column written twice");
            dst[d0 + i] = img[i];
          }
        } else {
          uint32_t any = 0;
          for (uint32_t i = p * 8; i < p * 8 + 8; ++i)
            if (i >= sp.off && i < sp.end) {
              if (d0 + i >= total || written[d0 + i]++) FAIL("column written twice or beyond the kept count");
              dst[d0 + i] = img[i];
              any = 1;
            }
          if (!any) FAIL("piece %u holds nothing", p);
          if (whole[(d0 >> 3) + p]) FAIL("ragged elements in a piece another block stored whole");
        }
      }
    }
    b = 0;
    for (uint32_t c = 0; c < cap; ++c)
      if (written[c] != (c < total)) FAIL("column %u written %u times", c, written[c]);
    fwrite(&total, 4, 1, out);
    fwrite(ids.data(), 4, n, out);
    fwrite(dst.data(), 2, total, out);
  }
  fclose(out);
  printf("ok\n");
  return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("retain_blocks")
    src = d / "blocks.cpp"
    src.write_text(SRC)
    exe = d / "blocks"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "niqki_amd", "csrc"), str(src), "-o", str(exe)])
    return str(exe)


@pytest.mark.parametrize("n", SIZES + [4096, 4097, 12289])
def test_row_loop_of_the_header_compacts_like_numpy(driver, tmp_path, n):
    masks = designed_masks(n)
    names = [nm for nm, _ in masks]
    assert len(set(names)) == len(names)
    if n > 8192:   # what the design is there for
        for k in (0, 1, 7, 8, 9):
            assert sorted(int(m[:4096].sum()) % 8 for nm, m in masks if nm.startswith("block%d_" % k)) == list(range(8))
            assert all(int(m[4096:8192].sum()) == k for nm, m in masks if nm.startswith("block%d_" % k))
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([n, len(masks)], np.uint32).tobytes())
        for _, m in masks:
            f.write(m.astype(np.uint8).tobytes())
    r = subprocess.run([driver, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
    buf = open(tmp_path / "out.bin", "rb").read()
    src = (np.arange(n, dtype=np.uint64) * 7 + 1).astype(np.uint16)
    at = 0
    for name, m in masks:
        total = int(np.frombuffer(buf, np.uint32, 1, at)[0])
        ids = np.frombuffer(buf, np.uint32, n, at + 4)
        row = np.frombuffer(buf, np.uint16, total, at + 4 + 4 * n)
        at += 4 + 4 * n + 2 * total
        assert total == int(m.sum()), name
        assert np.array_equal(ids, expected_ids(m)), name
        assert np.array_equal(row, src[m]), name                      # the plain compaction
    assert at == len(buf)
