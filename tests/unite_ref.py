"""The reference of the niqki_unite tests and their designed labellings: shared by tests/test_unite_ref_cpu.py (the
reference against a plain loop and against the oracle's sketches) and tests/test_gpu_unite.py (the kernel).  The launch
gives a wavefront 64 consecutive new columns of 16 rows; a label of at most kUniteLaneMax members is folded by one lane,
a larger one by the whole wavefront: the numbers are read from niqki_amd/csrc/nq_unite_blocks.h, not repeated here."""
import os
import re

import numpy as np

EMPTY = 0xFFFF
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "niqki_amd", "csrc", "nq_unite_blocks.h")


def launch_constants():
    """{name: value} of every `constexpr uint32_t kUnite... = <number>;` of the shared header"""
    text = open(HEADER).read()
    out = {m.group(1): int(m.group(2)) for m in re.finditer(r"constexpr uint32_t (kUnite\w+) = (\d+);", text)}
    assert {"kUniteCols", "kUniteWaves", "kUniteRows", "kUniteLaneMax"} <= set(out), out
    return out


def number_labels(labels):
    """(new_ids, L): the distinct labels numbered 0 .. L - 1 by the smallest genome id that carries them"""
    labels = np.asarray(labels).astype(np.uint32).reshape(-1)
    if labels.size == 0:
        return np.zeros(0, np.uint32), 0
    uniq, first, inverse = np.unique(labels, return_index=True, return_inverse=True)
    rank = np.empty(uniq.size, np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(uniq.size)
    return rank[inverse.reshape(-1)].astype(np.uint32), int(uniq.size)


def unite_ref(sk, labels):
    """(U, new_ids) of niqki_unite's definition: sk is (n, F) int32 with -1 for an empty cell; U is (L, F) int32"""
    sk = np.asarray(sk, dtype=np.int32)
    n, f = sk.shape
    new_ids, n_labels = number_labels(labels)
    assert new_ids.size == n
    if n == 0:
        return np.zeros((0, f), np.int32), new_ids
    assert sk.min() >= -1 and sk.max() < EMPTY
    cells = np.where(sk < 0, EMPTY, sk).astype(np.uint16)
    order = np.lexsort((np.arange(n), new_ids))          # by (label number, genome id)
    starts = np.searchsorted(new_ids[order], np.arange(n_labels))
    u = np.minimum.reduceat(cells[order], starts, axis=0).astype(np.int32)
    u[u == EMPTY] = -1
    return u, new_ids


def runs(n, lengths):
    """labels of runs of consecutive genomes whose lengths repeat `lengths`"""
    lab = np.empty(n, np.uint32)
    at = k = 0
    while at < n:
        ln = lengths[k % len(lengths)]
        lab[at:at + ln] = k
        at += ln
        k += 1
    return lab


def designed_labelings(n):
    """list of (name, uint32 labels of n genomes)"""
    c = launch_constants()
    out = []

    def add(name, lab):
        lab = np.asarray(lab).astype(np.uint32)
        assert lab.shape == (n,)
        out.append((name, lab))

    g = np.arange(n, dtype=np.int64)
    add("own", g)
    add("one", np.full(n, 7))
    for m in (2, 3, 64):
        add("mod%d" % m, g % m)
    add("runs", runs(n, [1, 2, 63, 64, 65]))
    rng = np.random.default_rng(2000 + n)
    half = rng.random(n) < 0.5
    add("giant_half", np.where(half, n + 5, g))
    add("huge_descending", np.where(g == n // 2, 0, 0xFFFFFFFF - g // 3))
    # label sizes T - 1, T, T + 1 around every number of the launch, each label's members astride column 2048 of the
    # source (consecutive there, then interleaved with singletons so that the members are not one contiguous run)
    thresholds = sorted({c["kUniteLaneMax"], c["kUniteCols"], c["kUniteRows"], c["kUniteCols"] * c["kUniteWaves"]})
    for t in thresholds:
        for size in (t - 1, t, t + 1):
            for name, step in (("packed", 1), ("spread", 3)):
                lo = 2048 - (size // 2) * step
                members = lo + np.arange(size) * step
                if size < 1 or lo < 1 or members[-1] >= n - 1:
                    continue
                lab = g + 10
                lab[members] = 3
                add("size%d_%s_at2048" % (size, name), lab)
    if n >= 2:
        add("last_alone", np.where(g == n - 1, 1, 0))
        add("last_pair_of_runs", runs(n, [5]))
    return out


def one_valid_cell_in_the_last_member(sk, labels, slots):
    """a copy of sk in which, in the given slots, every member of the LAST label is empty but its last member"""
    sk = sk.copy()
    new_ids, n_labels = number_labels(labels)
    members = np.nonzero(new_ids == n_labels - 1)[0]
    for s in slots:
        sk[members[:-1], s] = -1
        if sk[members[-1], s] < 0:
            sk[members[-1], s] = 5
    return sk


# ---- the algebra the feature rests on: records, groups and the oracle's sketches ---------------------------------------

PAN_K, PAN_S, PAN_W, PAN_H = 31, 8, 10, 4
PAN_GROUPS = [1, 2, 3, 4, 6, 8]
PAN_SEED = 31


def pan_records():
    """24 random ACGT records of 20 000 bases and the label (group number) of each: groups of consecutive records"""
    rng = np.random.default_rng(PAN_SEED)
    records = [np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 20000)].tobytes() for _ in range(sum(PAN_GROUPS))]
    labels = np.repeat(np.arange(len(PAN_GROUPS)), PAN_GROUPS).astype(np.uint32)
    return records, labels


def oracle_pan_sketches(po):
    """(member sketches, group sketches) by the oracle's accumulate: each record alone, a group's records chained"""
    records, labels = pan_records()
    p = po.make_params(PAN_K, PAN_S, PAN_W, PAN_H, 0.0)
    members = np.stack([po.sketch_accumulate(p, r) for r in records])
    groups = []
    for l in range(len(PAN_GROUPS)):
        sk = None
        for i in np.nonzero(labels == l)[0]:
            sk = po.sketch_accumulate(p, records[i], sk)
        groups.append(sk)
    return members, np.stack(groups)
