"""CPU: the designed densification cases of tests/densify_ref.py.  The model of the one-wavefront kernel (windowed passes,
closed-form tail, hand-back, pass over all cells) gives the serial loop's cells (oracle, nqo_densify) on every case and
names the class the table expects -- a designer or hash change that moves a seed out of its class fails here, not
silently on the device (tests/test_gpu_densify_designed.py runs the same table).  The table covers every boundary and
class listed below (one loop per requirement, nothing may be missing), and it tells four wrong models from the oracle."""
import functools

import numpy as np
import pytest

import densify_ref as dr


@functools.lru_cache(maxsize=None)
def modelled():
    """per case: (model cells, model class)"""
    return {c[0]: dr.model_wave(dr.make_cells(c), c[1]) for c in dr.CASES}


@functools.lru_cache(maxsize=None)
def oracle():
    """per case: (cells, oracle cells, rc), from the batches the GPU test uses"""
    out = {}
    for S in sorted({c[1] for c in dr.CASES}):
        names, rows, exp, rc = dr.batch_of(S)
        for i, n in enumerate(names):
            out[n] = (rows[i], exp[i], rc[i])
    return out


def n_ent(case):
    return int((oracle()[case[0]][0] >= 0).sum())


def values(case):
    cells = oracle()[case[0]][0]
    return cells[cells >= 0]


def stride_zeros(v, S):
    b = (dr.hash_words(int(v))[1] & ((1 << S) - 1)) | (1 << S)
    return (b & -b).bit_length() - 1


def some(pred, what):
    hits = [c[0] for c in dr.CASES if pred(c)]
    assert hits, "no case in the table: " + what
    return hits


def test_names_are_unique_and_designers_deterministic():
    names = [c[0] for c in dr.CASES]
    assert len(set(names)) == len(names)
    for c in dr.CASES[::7]:
        assert np.array_equal(dr.make_cells(c), dr.make_cells(c))


def test_model_equals_oracle_and_class_equals_table():
    for c in dr.CASES:
        cells, exp, rc = oracle()[c[0]]
        got, cls = modelled()[c[0]]
        assert np.array_equal(got, exp), c[0]
        assert cls == c[5], (c[0], cls)
        # what the serial loop says about the class
        assert (rc < 0) == (("fixpoint" in cls) or ("unreach" in cls) or (cls == "none" and n_ent(c) == 0)), (c[0], rc, cls)
        occ = cells >= 0
        assert np.array_equal(exp[occ], cells[occ]) and set(exp[exp >= 0].tolist()) <= set(cells[occ].tolist()), c[0]


def test_misaligned_rows_take_no_tail_and_give_the_same_cells():
    """rows that are not 16-byte aligned run the single-cell loops and never the closed form"""
    for c in dr.CASES:
        if c[1] <= 12 and c[5].split("+")[0] in ("tail", "handback"):
            got, cls = dr.model_wave(dr.make_cells(c), c[1], tail=False)
            assert cls.split("+")[0] == "passes" and np.array_equal(got, oracle()[c[0]][1]), c[0]


def test_coverage_list_boundaries():
    for S, ns in dr.BOUNDARY_N.items():
        for n in ns:
            some(lambda c: c[1] == S and c[3] is dr.random_cells and n_ent(c) == n, "S=%d n_ent=%d" % (S, n))
    for S, ns in dr.ALL_CELLS_N.items():
        for n in ns:
            some(lambda c: c[1] == S and n_ent(c) == n and c[5] == "cells", "all-cells pass S=%d n_ent=%d" % (S, n))
    for S, ns in dr.LARGE_F_N.items():
        for n in ns:
            some(lambda c: c[1] == S and n_ent(c) == n and (n == 1 or np.unique(values(c)).size < n),
                 "S=%d n_ent=%d with duplicates" % (S, n))


def test_coverage_every_window_instantiation():
    for rounds in dr.WINDOW_ROUNDS:
        for cls in ("tail", "tail+ties", "handback"):
            some(lambda c: 8 <= c[1] <= 12 and (n_ent(c) + 63) // 64 == rounds and c[5] == cls, "rounds=%d %s" % (rounds, cls))
    assert {dr.rounds_and_window(64 * r)[0] for r in dr.WINDOW_ROUNDS} == {1, 2, 3, 4, 6}


def test_coverage_tail_boundaries():
    for cls in ("tail+unreach", "tail+ties+unreach", "tail+unreach+nowrite"):
        some(lambda c: c[1] == 8 and c[5] == cls, "S=8 " + cls)
    for n_empty in (16, 17):
        some(lambda c: c[1] == 8 and 256 - n_ent(c) == n_empty and c[5].startswith("tail"), "%d empty cells at the start" % n_empty)


def test_coverage_fixpoint_exits():
    for S in (8, 10, 12, 13):
        fix = lambda c: c[1] == S and "fixpoint" in c[5] and oracle()[c[0]][2] == -1  # noqa: E731
        some(lambda c: fix(c) and n_ent(c) == 1 and stride_zeros(values(c)[0], S) == S, "S=%d stride 0 mod F" % S)
        some(lambda c: fix(c) and n_ent(c) == 1 and 0 < stride_zeros(values(c)[0], S) < S
             and 0 <= int((oracle()[c[0]][1] >= 0).sum()) - ((1 << S) >> stride_zeros(values(c)[0], S)) <= 1,   # (the orbit, and the entry's own cell)
             "S=%d even stride, part filled" % S)
        some(lambda c: fix(c) and n_ent(c) > 1 and np.unique(values(c)).size == 1, "S=%d several entries of one value" % S)
    some(lambda c: c[3] is dr.poly_a_like and "fixpoint" in c[5], "poly-A")
    for S in (10, 12):
        some(lambda c: c[1] == S and c[5] == "cells+fixpoint", "fixpoint exit of the all-cells pass, S=%d" % S)


def test_coverage_trivial_duplicates_and_large_values():
    for S in (8, 10, 12, 13, 16):
        some(lambda c: c[1] == S and n_ent(c) == 0 and c[5] == "none", "all empty S=%d" % S)
        some(lambda c: c[1] == S and n_ent(c) == 1 << S and c[5] == "none", "all full S=%d" % S)
    some(lambda c: c[2] == 4 and n_ent(c) == 200 and np.unique(values(c)).size <= 16, "W=4: 16 values over 200 cells")
    some(lambda c: n_ent(c) >= 100 and np.unique(values(c)).size == 1 and "fixpoint" not in c[5], "one value in every occupied cell")
    for S in (8, 10):
        some(lambda c: c[1] == S and np.unique(values(c)).size > 50 and values(c).max() > 1 << 30, "random large values S=%d" % S)
        some(lambda c: c[1] == S and set(values(c).tolist()) == {(1 << 31) - 2}, "constant 2^31 - 2, S=%d" % S)
        some(lambda c: c[1] == S and set(values(c).tolist()) == {1 << c[2]}, "constant 2^W, S=%d" % S)
    some(lambda c: values(c).size and values(c).max() > 1 << 30 and c[5] == "handback", "hand-back with large values")


@pytest.mark.parametrize("mutant", dr.MUTANTS)
def test_wrong_models_differ_from_the_oracle(mutant):
    """discriminating power of the table: ties to the largest index, no hand-back test, a winner's index not lowered, the
    idle count compared with F / 2 -- each is caught by at least one case"""
    caught = []
    for c in dr.CASES:
        if c[1] > 12:
            continue
        got, _ = dr.model_wave(dr.make_cells(c), c[1], mutant=mutant)
        if not np.array_equal(got, oracle()[c[0]][1]):
            caught.append(c[0])
    print(mutant, "caught by", caught)
    assert caught, mutant
    if mutant == "no_handback":   # the closed form without its check is wrong on the hand-back rows, all of them, and on no others
        assert caught == [c[0] for c in dr.CASES if c[5] == "handback"]
