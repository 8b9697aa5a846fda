// nq_retain_blocks.h -- block arithmetic of the store compaction (nq_index.hip, store_compact_kernel; niqki_retain).
//
// The sketch store is u16 [slot][cap], one column per genome.  Dropping genomes moves the kept columns of every row
// to the front, in order, into a NEW store.  The source columns are cut into blocks of kRetainBlock; the kept columns
// of a block land in ONE contiguous destination range [dst0, dst0 + kept), dst0 = kept columns of the blocks before.
// A workgroup compacts a block's row segment in LDS into an image laid on the DESTINATION's 16-byte grid: image
// element off + r is destination column dst0 + r, off = dst0 & 7, so image piece p (8 elements, 16 bytes) is the
// destination's piece (dst0 >> 3) + p.  Pieces that lie whole inside the range are stored as 16 bytes; the elements of
// the first and last piece, which a neighbouring block shares, as 2 bytes each: no 16-byte piece of the destination is
// ever written whole by two workgroups, and no byte by more than one.
//
// Host and device share this code: the kernels call it, tests/test_retain_blocks.py compiles it with g++ and drives a
// restatement of the kernel's row loop over the designed masks.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define NQ_HD __host__ __device__ __forceinline__
#else
#define NQ_HD inline
#endif

namespace nq {

constexpr uint32_t kRetainBlock = 4096;                  // source columns of a block
constexpr uint32_t kRetainWords = kRetainBlock / 64;     // its keep bits as 64-bit words (bit c & 63 of word c >> 6)
constexpr uint32_t kRetainImage = kRetainBlock + 8;      // elements of a row image: the block's columns + the offset

// What a block's image looks like on the destination's 16-byte grid.
struct RetainSpan {
  uint32_t off;        // image element of the block's first kept column (dst0 & 7)
  uint32_t end;        // one past the image element of its last kept column (off + kept)
  uint32_t pieces;     // 16-byte pieces the image touches: [0, pieces)
  uint32_t whole_lo;   // pieces [whole_lo, whole_hi) lie inside [off, end): 16-byte stores
  uint32_t whole_hi;   // pieces [0, whole_lo) and [whole_hi, pieces) are ragged: their elements inside [off, end), 2 bytes each
};

NQ_HD RetainSpan retain_span(uint64_t dst0, uint32_t kept) {
  RetainSpan s;
  s.off = (uint32_t)(dst0 & 7u);
  s.end = s.off + kept;
  s.pieces = (s.end + 7u) >> 3;
  s.whole_lo = s.off ? 1u : 0u;
  s.whole_hi = s.end >> 3;
  if (s.whole_hi < s.whole_lo) s.whole_hi = s.whole_lo;   // a range inside one piece
  if (kept == 0) s.pieces = s.whole_lo = s.whole_hi = 0;
  return s;
}

// Rank inside the block of column c (0 .. kRetainBlock - 1): kept columns of the block below it.  word_rank[w] = kept
// columns of the words below w (the exclusive prefix of the words' popcounts).
NQ_HD uint32_t retain_rank(const uint64_t *words, const uint32_t *word_rank, uint32_t c) {
  const uint64_t below = words[c >> 6] & ((1ull << (c & 63u)) - 1ull);
  return word_rank[c >> 6] + (uint32_t)__builtin_popcountll(below);
}

// Capacity (columns) of the store that holds n_kept genomes: whole 128-byte lines, never none
NQ_HD uint64_t retain_cap(uint64_t n_kept) { return ((n_kept < 64u ? 64u : n_kept) + 63u) / 64u * 64u; }

}  // namespace nq
