"""The designed keep masks of the niqki_retain tests: shared by tests/test_retain_blocks.py (the block arithmetic of
niqki_amd/csrc/nq_retain_blocks.h on the CPU) and tests/test_gpu_retain.py (the kernels).  The compaction works on
blocks of 4 096 source columns and stores along the destination's grid of 8 columns (16 bytes): the masks put run ends
on and beside the powers of two up to the block size, give a whole block exactly 0, 1, 7, 8 and 9 kept columns, and
lead every residue mod 8 of kept columns up to such a block."""
import numpy as np

BLOCK = 4096
SIZES = [1, 63, 64, 65, 2049, 8300]
EDGES = [64, 256, 1024, 2048, 4096]


def designed_masks(n):
    """list of (name, bool mask of n genomes)"""
    out = []

    def add(name, m):
        assert m.dtype == bool and m.shape == (n,)
        out.append((name, m))

    idx = np.arange(n)
    add("all", np.ones(n, bool))
    add("none", np.zeros(n, bool))
    add("first", idx == 0)
    add("last", idx == n - 1)
    add("even", idx % 2 == 0)
    add("odd", idx % 2 == 1)
    add("run_removed", ~((idx >= n // 3) & (idx < 2 * n // 3 + 1)))
    add("run_kept", (idx >= n // 3) & (idx < 2 * n // 3 + 1))
    if n >= 2049:
        ends = [c + d for c in EDGES for d in (-1, 0, 1) if c + d < n]
        far = n - 37
        for x in ends:
            for name, run in (("from%d" % x, (idx >= x) & (idx < max(far, x + 1))), ("upto%d" % x, (idx >= 5) & (idx < x))):
                add("kept_" + name, run)
                add("removed_" + name, ~run)
    if n > 2 * BLOCK:
        # block 1 = columns [4096, 8192) keeps exactly k columns, spread over it; block 0 keeps a prefix of every
        # length mod 8 (scattered, so that its own image is ragged too); the columns behind block 1 all stay
        for k in (0, 1, 7, 8, 9):
            for r in range(8):
                m = np.zeros(n, bool)
                m[(np.arange(96 + r) * 41) % BLOCK] = True            # 41 is odd: distinct columns
                assert int(m.sum()) == 96 + r
                m[BLOCK + (np.arange(k) * 509 + 3) % BLOCK] = True
                m[2 * BLOCK:] = True
                assert int(m[BLOCK:2 * BLOCK].sum()) == k
                add("block%d_prefix%d" % (k, r), m)
    rng = np.random.default_rng(1000 + n)
    add("random17", rng.random(n) < 0.17)
    add("random99", rng.random(n) < 0.99)
    return out


def expected_ids(mask):
    """new_ids of the definition: the kept genomes below, 0xFFFFFFFF for a dropped genome"""
    ids = (np.cumsum(mask) - 1).astype(np.uint32)
    ids[~mask] = 0xFFFFFFFF
    return ids
