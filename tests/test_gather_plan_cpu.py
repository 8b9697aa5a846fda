"""The query launch rule (niqki_amd/csrc/nq_gather_plan.h), on the CPU: the header is the code counts_segment, launch_lookup
and launch_gather run, compiled here with g++ and asked for the plan of every row of the tables below.  The expectations
are typed in, read off the rule as counts_segment, launch_lookup, gather_shape and launch_gather stated it before the plan
was a value (thresholds 256 / 1024 / 512 / 64 queries, 16384 genomes, 8192 slots, 12288 genomes per tile, 128 MiB, 8 GiB;
the byte counts worked out per row in the comments); nothing here computes them."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r"""
#include <cstdio>
#include <cstring>
#include "nq_gather_plan.h"

// one row per line of stdin:
//   request W f_local n_tiles tile align_log2 padded n_genomes lookup_prepass query_order gather_variant paged aligned
//   pad_at_zero nq hl_cap n
int main() {
  char req[32];
  unsigned W, f_local, n_tiles, tile, align, padded, n_genomes, paged, aligned, pad0, nq, hl_cap, n;
  int prepass, order, variant;
  while (scanf("%31s %u %u %u %u %u %u %u %d %d %d %u %u %u %u %u %u", req, &W, &f_local, &n_tiles, &tile, &align, &padded, &n_genomes,
               &prepass, &order, &variant, &paged, &aligned, &pad0, &nq, &hl_cap, &n) == 17) {
    const nq::GatherFacts f{1u << W, f_local, n_tiles, tile, align, padded != 0, n_genomes};
    const nq::GatherPlan p = nq::gather_plan(f, nq::GatherOptions{prepass, order, variant, paged != 0}, aligned != 0, pad0 != 0, nq, hl_cap);
    if (!strcmp(req, "facts")) {
      printf("%d %d %u\n", (int)nq::launch_lookup_usable(f), (int)nq::lookup_wants_packed(f), nq::lookup_slots(f));
    } else if (!strcmp(req, "plan")) {
      printf("%d %d %d %u %zu %zu %zu %d %d %d %d %u %zu %d\n", (int)p.pre, (int)p.packed_table, (int)p.ordered, p.chunk, p.stash_bytes,
             p.pre_bytes, p.order_bytes, p.shape.block, p.shape.unroll, p.shape.nt, (int)p.shape.pad, nq::gather_shape_code(p.shape),
             p.lds_bytes, (int)nq::gather_shape_exists(p.shape));
    } else if (!strcmp(req, "lookup")) {   // the pre-pass kernel of a launch of n queries and its kernel launches: tiles, pieces per thread
      const nq::LookupForm lf = nq::lookup_form(p, n);
      printf("%d %u %u", (int)lf.rows, lf.slots, lf.step);
      for (unsigned t0 = 0; t0 < n_tiles; t0 += lf.step) {
        const nq::LookupLaunch l = nq::lookup_launch(lf, n_tiles, f.R, t0);
        printf(" %u %u %d", l.nt, l.per, (int)nq::lookup_launch_exists(lf.rows, lf.slots, l.nt, l.per));
      }
      printf("\n");
    } else if (!strcmp(req, "order")) {
      const nq::OrderForm of = nq::order_form(p, n);
      printf("%d %d\n", (int)of.ordered, (int)of.fork);
    } else if (!strcmp(req, "lds")) {   // n: threads per workgroup
      printf("%zu %zu\n", nq::gather_lds_bytes(n, tile, padded != 0, hl_cap), nq::hit_list_lds(tile, hl_cap));
    } else {
      return 2;
    }
  }
  return 0;
}
"""

# ---- views: (W, f_local, n_tiles, tile, align_log2, padded, n_genomes) ----
NS = (12, 32768, 2, 50048, 6, 1, 100000)     # the bench's shape: S = 15, two padded tiles
NS_FLAT = (12, 32768, 2, 50048, 6, 0, 100000)
T1 = (12, 4096, 1, 50048, 6, 1, 50000)       # one tile, S = 12
V3 = (12, 32768, 3, 65408, 6, 1, 190000)
V4 = (12, 32768, 4, 65408, 6, 1, 250000)
V5 = (12, 32768, 5, 65408, 6, 1, 300000)
V16 = (12, 32768, 16, 65408, 6, 1, 1046528)
V17 = (12, 32768, 17, 65408, 6, 1, 1100000)
SMALL = (12, 4096, 1, 12288, 6, 1, 12288)    # a short-read index: the largest tile of the 256-thread shape
SMALL1 = (12, 4096, 1, 12352, 6, 1, 12352)   # ... and the next one


def two_tiles(f_local):
    return (12, f_local, 2, 50048, 6, 1, 100000)


def tiles(n, W=12):
    return (W, 4096, n, 65408, 6, 1, 60000 * n)


# ---- options: (lookup_prepass, query_order, gather_variant, paged); then aligned, pad_at_zero, nq, hl_cap, n ----
DEF = (-1, 1, 0, 0)
PLAIN = (0, 0, 0, 0)    # no pre-pass, no order
PRE = (1, 0, 0, 0)      # pre-pass wherever usable, no order

# stat "last_gather_kernel": BLOCK | UNROLL << 12 | (NT + 1) << 20 | PAD << 24, typed per shape
K1024_16_1_P, K1024_16_2_P, K1024_16_3_P, K1024_16_4_P = 0x1210400, 0x1310400, 0x1410400, 0x1510400
K1024_32_PRE_P, K1024_16_PRE, K1024_8_2_P, K1024_8_2, K1024_32_2_P = 0x1020400, 0x0010400, 0x1308400, 0x0308400, 0x1320400
K512_16_2, K256_16_2, K128_16_2, K256_16_1, K256_16_PRE = 0x0310200, 0x0310100, 0x0310080, 0x0210100, 0x0010100

# LDS bytes: counters (tile + 1) / 2 words [+ 64 dummy words] + 2048 per wave [+ 8 per hit-list key]
L_NS = 25088 * 4 + 16 * 2048              # tile 50048 padded, 1024 threads: 133120
L_NS_FLAT = 25024 * 4 + 16 * 2048         # ... not padded: 132864
L_65408 = 32768 * 4 + 16 * 2048           # 163840: the whole LDS of a workgroup
MIB = 1 << 20

# (view, options, aligned, pad_at_zero, nq, hl_cap) -> (usable, packed form, slots per lookup_kernel workgroup)
FACTS = [
    # f_local not a multiple of 32 (<= 2 tiles) or of 16 (> 2 tiles)
    (((12, 4096, 1, 50048, 6, 1, 50000),), (1, 1, 32)),
    (((12, 4080, 2, 50048, 6, 1, 100000),), (0, 0, 32)),
    (((12, 4080, 3, 50048, 6, 1, 150000),), (1, 0, 16)),     # whole blocks of 16, but no rows of 32 slots
    (((12, 4072, 3, 50048, 6, 1, 150000),), (0, 0, 16)),
    # the packed word's length half: tile <= 65535
    (((12, 4096, 1, 65535, 6, 0, 65535),), (1, 1, 32)),
    (((12, 4096, 1, 65536, 6, 0, 65536),), (0, 0, 32)),
    # ... and its start half: (tile >> align_log2) + R + 1 at 65535 and 65536
    (((15, 4096, 1, 32766, 0, 0, 32766),), (1, 0, 32)),
    (((15, 4096, 1, 32767, 0, 0, 32767),), (0, 0, 32)),
    # the packed form by (W, tiles): a group's row of R * {1, 2} words is 1 or 2 x 4096 words
    ((tiles(1, 12),), (1, 1, 32)),
    ((tiles(2, 12),), (1, 1, 32)),
    ((tiles(3, 12),), (1, 1, 16)),
    ((tiles(1, 13),), (1, 1, 32)),
    ((tiles(2, 11),), (1, 1, 32)),
    ((tiles(1, 10),), (1, 0, 32)),
    ((tiles(1, 11),), (1, 0, 32)),
    ((tiles(3, 11),), (1, 0, 16)),    # the last odd tile's row would be half a piece per thread
    ((tiles(2, 13),), (1, 0, 32)),    # 64 KB per row
]

# -> (pre, packed_table, ordered, chunk, stash bytes, pre-pass bytes, order bytes, BLOCK, UNROLL, NT, PAD, code, LDS bytes)
PLANS = [
    # ---- default pre-pass (-1).  Two tiles, S = 15: 256 KB per query either way; 1023 / 1024 queries; paged ----
    ((NS, DEF, 1, 1, 1023, 0), (0, 0, 1, 4096, 1023 * 256 * 1024, 0, 32768, 1024, 16, 2, 1, K1024_16_2_P, L_NS)),
    ((NS, DEF, 1, 1, 1024, 0), (1, 1, 1, 4096, 0, 256 * MIB, 32768, 1024, 32, -1, 1, K1024_32_PRE_P, L_NS)),
    ((NS, (-1, 1, 0, 1), 1, 1, 1024, 0), (0, 0, 1, 4096, 256 * MIB, 0, 32768, 1024, 16, 2, 1, K1024_16_2_P, L_NS)),
    # five tiles: 255 / 256 queries (stash 4 x 256 KB per query; pre-pass words 5 x 128 KB)
    ((V5, DEF, 1, 1, 255, 0), (0, 0, 1, 4096, 255 * MIB, 0, 32768, 1024, 16, 1, 1, K1024_16_1_P, L_65408)),
    ((V5, DEF, 1, 1, 256, 0), (1, 1, 1, 4096, 0, 160 * MIB, 32768, 1024, 32, -1, 1, K1024_32_PRE_P, L_65408)),
    # three and four tiles: never by default
    ((V3, DEF, 1, 1, 4096, 0), (0, 0, 1, 4096, 2048 * MIB, 0, 32768, 1024, 16, 3, 1, K1024_16_3_P, L_65408)),
    ((V4, DEF, 1, 1, 4096, 0), (0, 0, 1, 4096, 3072 * MIB, 0, 32768, 1024, 16, 4, 1, K1024_16_4_P, L_65408)),
    # forced off, forced on (one query), forced on with misaligned sketches
    ((NS, (0, 1, 0, 0), 1, 1, 4096, 0), (0, 0, 1, 4096, 1024 * MIB, 0, 32768, 1024, 16, 2, 1, K1024_16_2_P, L_NS)),
    ((NS, (1, 1, 0, 0), 1, 1, 1, 0), (1, 1, 0, 4096, 0, 262144, 0, 1024, 32, -1, 1, K1024_32_PRE_P, L_NS)),
    ((NS, (1, 1, 0, 0), 0, 1, 1, 0), (0, 0, 0, 4096, 262144, 0, 0, 1024, 16, 2, 1, K1024_16_2_P, L_NS)),
    # forced on where the table has no packed form (W = 10): lookup_kernel, bit 1 of the stat stays 0
    ((tiles(1, 10), PRE, 1, 1, 4096, 0), (1, 0, 0, 4096, 0, 64 * MIB, 0, 1024, 32, -1, 1, K1024_32_PRE_P, L_65408)),
    # ---- order ----
    ((NS, (0, 0, 0, 0), 1, 1, 4096, 0), (0, 0, 0, 4096, 1024 * MIB, 0, 0, 1024, 16, 2, 1, K1024_16_2_P, L_NS)),
    ((NS, (0, 1, 0, 0), 1, 1, 63, 0), (0, 0, 0, 4096, 63 * 262144, 0, 0, 1024, 16, 2, 1, K1024_16_2_P, L_NS)),
    ((NS, (0, 1, 0, 0), 1, 1, 64, 0), (0, 0, 1, 4096, 16 * MIB, 0, 32768, 1024, 16, 2, 1, K1024_16_2_P, L_NS)),
    # the key's 20 bits: a segment of 2^20 - 2 / 2^20 - 1 genomes (17 tiles: 16 x 256 KB of stash per query)
    (((12, 32768, 17, 65408, 6, 1, 1048574), (0, 1, 0, 0), 1, 1, 64, 0), (0, 0, 1, 4096, 256 * MIB, 0, 32768, 1024, 16, 1, 1, K1024_16_1_P, L_65408)),
    (((12, 32768, 17, 65408, 6, 1, 1048575), (0, 2, 0, 0), 1, 1, 64, 0), (0, 0, 0, 4096, 256 * MIB, 0, 0, 1024, 16, 1, 1, K1024_16_1_P, L_65408)),
    # mode 1: 16383 / 16384 genomes, 4096 / 8192 slots; mode 2 below both (tile 16384: 8192 + 64 counter words)
    (((12, 8192, 1, 16384, 6, 1, 16383), (0, 1, 0, 0), 1, 1, 64, 0), (0, 0, 0, 64, 0, 0, 0, 1024, 16, 1, 1, K1024_16_1_P, 8256 * 4 + 32768)),
    (((12, 8192, 1, 16384, 6, 1, 16384), (0, 1, 0, 0), 1, 1, 64, 0), (0, 0, 1, 4096, 0, 0, 32768, 1024, 16, 1, 1, K1024_16_1_P, 8256 * 4 + 32768)),
    (((12, 4096, 1, 16384, 6, 1, 16384), (0, 1, 0, 0), 1, 1, 64, 0), (0, 0, 0, 64, 0, 0, 0, 1024, 16, 1, 1, K1024_16_1_P, 8256 * 4 + 32768)),
    (((12, 4096, 1, 16384, 6, 1, 1000), (0, 2, 0, 0), 1, 1, 64, 0), (0, 0, 1, 4096, 0, 0, 32768, 1024, 16, 1, 1, K1024_16_1_P, 8256 * 4 + 32768)),
    # ---- chunk ----
    # one tile without pre-pass: the whole call in one launch, no scratch
    ((T1, PLAIN, 1, 1, 100000, 0), (0, 0, 0, 100000, 0, 0, 0, 1024, 16, 1, 1, K1024_16_1_P, L_NS)),
    # stash of 16 / 32 / 64 KB per query: 128 MiB hold 8192 / 4096 / 2048 of them
    ((two_tiles(2048), PLAIN, 1, 1, 10000, 0), (0, 0, 0, 8192, 128 * MIB, 0, 0, 1024, 16, 2, 1, K1024_16_2_P, L_NS)),
    ((two_tiles(4096), PLAIN, 1, 1, 10000, 0), (0, 0, 0, 4096, 128 * MIB, 0, 0, 1024, 16, 2, 1, K1024_16_2_P, L_NS)),
    ((two_tiles(8192), PLAIN, 1, 1, 10000, 0), (0, 0, 0, 4096, 256 * MIB, 0, 0, 1024, 16, 2, 1, K1024_16_2_P, L_NS)),
    # ordered or pre: 4096 even where 8192 stashes would fit
    ((two_tiles(2048), (0, 2, 0, 0), 1, 1, 10000, 0), (0, 0, 1, 4096, 64 * MIB, 0, 32768, 1024, 16, 2, 1, K1024_16_2_P, L_NS)),
    ((two_tiles(2048), PRE, 1, 1, 10000, 0), (1, 1, 0, 4096, 0, 64 * MIB, 0, 1024, 32, -1, 1, K1024_32_PRE_P, L_NS)),
    # the 8 GiB of pre-pass words: S = 15 at 16 tiles is 2 MiB per query, 4096 fit exactly; at 17 tiles 3855 fit, so 3840
    ((V16, PRE, 1, 1, 10000, 0), (1, 1, 0, 4096, 0, 8192 * MIB, 0, 1024, 32, -1, 1, K1024_32_PRE_P, L_65408)),
    ((V17, PRE, 1, 1, 10000, 0), (1, 1, 0, 3840, 0, 3840 * 17 * 131072, 0, 1024, 32, -1, 1, K1024_32_PRE_P, L_65408)),
    # ---- shape ----
    # gather_variant 1 .. 5 (the padded walk: 1024 threads only)
    ((NS, (0, 0, 1, 0), 1, 1, 64, 0), (0, 0, 0, 4096, 16 * MIB, 0, 0, 1024, 8, 2, 1, K1024_8_2_P, L_NS)),
    ((NS, (0, 0, 2, 0), 1, 1, 64, 0), (0, 0, 0, 4096, 16 * MIB, 0, 0, 1024, 32, 2, 1, K1024_32_2_P, L_NS)),
    ((NS, (0, 0, 3, 0), 1, 1, 64, 0), (0, 0, 0, 4096, 16 * MIB, 0, 0, 512, 16, 2, 0, K512_16_2, 25088 * 4 + 8 * 2048)),
    ((NS, (0, 0, 4, 0), 1, 1, 64, 0), (0, 0, 0, 4096, 16 * MIB, 0, 0, 256, 16, 2, 0, K256_16_2, 25088 * 4 + 4 * 2048)),
    ((NS, (0, 0, 5, 0), 1, 1, 64, 0), (0, 0, 0, 4096, 16 * MIB, 0, 0, 128, 16, 2, 0, K128_16_2, 25088 * 4 + 2 * 2048)),
    # variant 0: tiles of 12288 / 12352 genomes
    ((SMALL, PLAIN, 1, 1, 64, 0), (0, 0, 0, 64, 0, 0, 0, 256, 16, 1, 0, K256_16_1, 6208 * 4 + 4 * 2048)),
    ((SMALL1, PLAIN, 1, 1, 64, 0), (0, 0, 0, 64, 0, 0, 0, 1024, 16, 1, 1, K1024_16_1_P, 6240 * 4 + 16 * 2048)),
    # the short-read form: one small tile, hit lists of 64 keys, a batch of 65536 reads (the default takes the pre-pass)
    ((SMALL, DEF, 1, 1, 65536, 64), (1, 1, 0, 4096, 0, 64 * MIB, 0, 256, 16, -1, 0, K256_16_PRE, 6208 * 4 + 4 * 2048 + 512)),
    # not padded with the pre-pass; padded but the kernel's LDS does not start at 0 (the dummy words are still counted)
    ((NS_FLAT, PRE, 1, 1, 64, 0), (1, 1, 0, 4096, 0, 16 * MIB, 0, 1024, 16, -1, 0, K1024_16_PRE, L_NS_FLAT)),
    ((NS, PRE, 1, 0, 64, 0), (1, 1, 0, 4096, 0, 16 * MIB, 0, 1024, 16, -1, 0, K1024_16_PRE, L_NS)),
    ((NS, (0, 0, 1, 0), 1, 0, 64, 0), (0, 0, 0, 4096, 16 * MIB, 0, 0, 1024, 8, 2, 0, K1024_8_2, L_NS)),
    # NT with the pre-pass on one, three and four tiles (two, five: above; without: the rows above, 1 .. 5 tiles)
    ((T1, PRE, 1, 1, 64, 0), (1, 1, 0, 4096, 0, 64 * 16384, 0, 1024, 32, -1, 1, K1024_32_PRE_P, L_NS)),
    ((V3, PRE, 1, 1, 64, 0), (1, 1, 0, 4096, 0, 64 * 3 * 131072, 0, 1024, 32, -1, 1, K1024_32_PRE_P, L_65408)),
    ((V4, PRE, 1, 1, 64, 0), (1, 1, 0, 4096, 0, 64 * 4 * 131072, 0, 1024, 32, -1, 1, K1024_32_PRE_P, L_65408)),
]

# (view, options, aligned, pad_at_zero, nq, hl_cap, n) -> (streamed rows, slots, tiles per launch, then per kernel launch: NT, PER)
LOOKUPS = [
    # with the table: 511 / 512 queries in the launch
    ((NS, PRE, 1, 1, 4096, 0, 511), (0, 32, 4, (2, 0))),
    ((NS, PRE, 1, 1, 4096, 0, 512), (1, 32, 2, (2, 2))),
    # streamed rows, 1 .. 6 tiles: groups of two, a last odd tile alone
    ((tiles(1), PRE, 1, 1, 4096, 0, 4096), (1, 32, 2, (1, 1))),
    ((tiles(2), PRE, 1, 1, 4096, 0, 4096), (1, 32, 2, (2, 2))),
    ((tiles(3), PRE, 1, 1, 4096, 0, 4096), (1, 32, 2, (2, 2), (1, 1))),
    ((tiles(4), PRE, 1, 1, 4096, 0, 4096), (1, 32, 2, (2, 2), (2, 2))),
    ((tiles(5), PRE, 1, 1, 4096, 0, 4096), (1, 32, 2, (2, 2), (2, 2), (1, 1))),
    ((tiles(6), PRE, 1, 1, 4096, 0, 4096), (1, 32, 2, (2, 2), (2, 2), (2, 2))),
    ((tiles(2, 11), PRE, 1, 1, 4096, 0, 4096), (1, 32, 2, (2, 1))),
    ((tiles(1, 13), PRE, 1, 1, 4096, 0, 4096), (1, 32, 2, (1, 2))),
    # random look-ups, 1 .. 6 tiles: blocks of 32 slots up to two tiles, else of 16 and four tiles per launch
    ((tiles(1), PRE, 1, 1, 4096, 0, 100), (0, 32, 4, (1, 0))),
    ((tiles(2), PRE, 1, 1, 4096, 0, 100), (0, 32, 4, (2, 0))),
    ((tiles(3), PRE, 1, 1, 4096, 0, 100), (0, 16, 4, (3, 0))),
    ((tiles(4), PRE, 1, 1, 4096, 0, 100), (0, 16, 4, (4, 0))),
    ((tiles(5), PRE, 1, 1, 4096, 0, 100), (0, 16, 4, (4, 0), (1, 0))),
    ((tiles(6), PRE, 1, 1, 4096, 0, 100), (0, 16, 4, (4, 0), (2, 0))),
    # no packed form (W = 11, three tiles): random look-ups whatever the launch's size
    ((tiles(3, 11), PRE, 1, 1, 4096, 0, 4096), (0, 16, 4, (3, 0))),
]

# (view, options, aligned, pad_at_zero, nq, hl_cap, n) -> (ordered, fork)
ORDERS = [
    ((NS, (1, 1, 0, 0), 1, 1, 4160, 0, 4096), (1, 1)),
    ((NS, (1, 1, 0, 0), 1, 1, 4160, 0, 64), (1, 1)),      # the call's last launch
    ((NS, (1, 1, 0, 0), 1, 1, 4159, 0, 63), (0, 0)),
    ((NS, (0, 1, 0, 0), 1, 1, 4160, 0, 64), (1, 0)),      # no pre-pass to run beside
    ((NS, (1, 0, 0, 0), 1, 1, 4160, 0, 4096), (0, 0)),
]

# (tile, padded, hl_cap, threads) -> (LDS bytes, hit_list_lds(tile, hl_cap))
LDS = [
    ((12288, 0, 0, 128), (6144 * 4 + 2 * 2048, 6208 * 4 + 16 * 2048)),
    ((12288, 1, 64, 256), (6208 * 4 + 4 * 2048 + 512, 6208 * 4 + 16 * 2048 + 512)),
    ((50048, 0, 0, 512), (25024 * 4 + 8 * 2048, L_NS)),
    ((50048, 1, 0, 1024), (L_NS, L_NS)),
    ((50048, 0, 2048, 1024), (L_NS_FLAT + 16384, L_NS + 16384)),
    ((50048, 1, 2048, 1024), (149504, 149504)),       # hit_list_lds IS the 1024-thread padded value
    ((50049, 1, 4, 1024), (25089 * 4 + 32768 + 32, 25089 * 4 + 32768 + 32)),   # an odd tile: (tile + 1) / 2 words
]


def ask(tmp_path, rows):
    src = tmp_path / "plan.cpp"
    src.write_text(SRC)
    exe = tmp_path / "plan"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "niqki_amd", "csrc"),
                           str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], input="".join(r + "\n" for r in rows), capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.strip().split("\n")
    assert len(lines) == len(rows)
    return [tuple(int(x) for x in line.split()) for line in lines]


def row(req, view, opts=PRE, aligned=1, pad0=1, nq=4096, hl_cap=0, n=0):
    return " ".join(str(x) for x in (req,) + tuple(view) + tuple(opts) + (aligned, pad0, nq, hl_cap, n))


def flat(want):
    return tuple(x for part in want for x in (part if isinstance(part, tuple) else (part,)))


def test_plan_of_every_row(tmp_path):
    """Every row's answer is the one typed in: whether the pre-pass can serve a view and in which form; the plan of a call
    (pre-pass, packed table, order, chunk, the three scratch sizes, the gather_kernel instantiation with its stat code and
    LDS, which launch_gather has); the pre-pass kernel and the order of one launch; the LDS formula."""
    assert len(FACTS) + len(PLANS) + len(LOOKUPS) + len(ORDERS) + len(LDS) >= 80
    rows = [row("facts", *args) for args, _ in FACTS] + [row("plan", *args) for args, _ in PLANS]
    rows += [row("lookup", *args) for args, _ in LOOKUPS] + [row("order", *args) for args, _ in ORDERS]
    rows += [row("lds", (12, 4096, 1, tile, 6, padded, tile), hl_cap=cap, n=block) for (tile, padded, cap, block), _ in LDS]
    want = [w for _, w in FACTS] + [w + (1,) for _, w in PLANS]
    want += [flat(w[:3]) + flat(tuple(g + (1,) for g in w[3:])) for _, w in LOOKUPS]   # (every kernel launch: an instantiation there is)
    want += [w for _, w in ORDERS] + [w for _, w in LDS]
    got = ask(tmp_path, rows)
    bad = [(r, w, g) for r, w, g in zip(rows, want, got) if w != g]
    assert not bad, "\n".join("%s: expected %r, got %r" % b for b in bad)
