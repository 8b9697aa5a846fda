"""Densification on designed cells: a model of the one-wavefront kernel's process, a classifier, the designers of the
cell sets and the case table that tests/test_densify_ref_cpu.py and tests/test_gpu_densify_designed.py share.  CPU only.

The loop every form must reproduce is the serial one of src/niqki_index.cpp:313-331 (oracle/niqki_oracle.c,
nqo_densify).  model_wave() restates what sketch_reads_kernel does with a row of cells (niqki_amd/csrc/nq_sketch_reads.hip:
densify_wave_entries_window, densify_tail, densify_wave_cells) in plain Python over the oracle's rev64 / unrev64, and
names the path the row took:

    none       nothing to do: no cell or every cell occupied, the row comes back untouched
    cells      more occupied cells than the 384-entry list holds: the plain pass over all cells (densify_wave_cells)
    passes     windowed passes over the entries to the end
    tail       windowed passes, then the closed form for the last <= 16 cells
    handback   the closed form found a losing entry that had won earlier in the tail: nothing written, passes to the end

    +ties      (tail) some cell of the closed form is reached by more than one entry in its winning pass
    +unreach   (tail) some empty cell that no orbit reaches; it stays empty, the oracle's rc is -1
    +nowrite   (tail) the closed form saw only such cells and wrote nothing
    +fixpoint  left through F idle passes with cells still empty (oracle rc = -1)

The frequencies of these classes on random cells, and which test pins which device form: DESIGN.md, "densification".
"""
import concurrent.futures
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import pyoracle as po  # noqa: E402

M32 = 0xFFFFFFFF
LIST_ENTRIES = 384      # kReadMaxEntries (nq_sketch_plan.h): niqki_densify takes the long entry list
TAIL_CELLS = 16         # kTailCells
MUTANTS = ("tie_largest", "no_handback", "mk_not_lowered", "idle_half")


@functools.lru_cache(maxsize=None)
def hash_words(v):
    """(A, B): low words of unrev64(v) and rev64(v); an entry's target in pass s is (A + s B) mod F (:308-310)."""
    return po.unrev64(int(v)) & M32, po.rev64(int(v)) & M32


def rounds_and_window(n_ent):
    """(R, U) of the densify_wave_entries_window instantiation the kernel's dispatch takes for n_ent entries."""
    rounds = (n_ent + 63) >> 6
    if rounds <= 1:
        return 1, 8
    if rounds <= 2:
        return 2, 8
    if rounds <= 3:
        return 3, 4
    if rounds <= 4:
        return 4, 4
    return 6, 4


# ---- the closed-form tail's arithmetic (densify_tail) ----------------------------------------------------------------

def inv_odd(o):
    """o^-1 mod 2^32 by three Newton steps from x = o (correct to 3 bits; every step doubles them: 24 >= log2 F)."""
    x = o
    for _ in range(3):
        x = (x * (2 - o * x)) & M32
    return x


def tail_key(c, T, B, mk, F):
    """Key of an entry for empty cell c: s << 15 | index at the start of the tail, s = the pass (counted from the
    tail's start) in which target T + s B reaches c; None where the orbit never reaches c."""
    Fm = F - 1
    b = (B & Fm) | F
    j = (b & -b).bit_length() - 1
    odd = ((B >> j) | 1) & M32
    x = (c - T) & M32
    if x & ((1 << j) - 1):
        return None
    s = ((x * inv_odd(odd)) & Fm) >> j
    return (s << 15) | (mk & 0x7FFF)


def solve_tail(empties, T, B, mk, F, tie_largest=False):
    """The closed form over the listed empty cells.  T, B, mk: per entry, at the start of the tail.  Returns
    (writes {cell: entry}, ties, unreachable cells, handback).  tie_largest: the mutant that gives a tied cell to
    the entry with the LARGEST index."""
    n = len(T)
    win_min = [1 << 60] * n
    lose_max = [0] * n
    writes, ties, unreach = {}, 0, []
    for c in empties:
        keys = []
        for k in range(n):
            key = tail_key(int(c), T[k], B[k], mk[k], F)
            if key is not None:
                keys.append((key, k))
        if not keys:
            unreach.append(int(c))
            continue
        s_star = min(keys)[0] >> 15
        tied = [(key, k) for key, k in keys if key >> 15 == s_star]
        wkey, wk = max(tied) if tie_largest else min(tied)
        writes[int(c)] = wk
        win_min[wk] = min(win_min[wk], s_star)
        if len(tied) > 1:
            ties += 1
            for key, k in tied:
                if k != wk:
                    lose_max[k] = max(lose_max[k], s_star)
    handback = any(win_min[k] < lose_max[k] for k in range(n))
    return writes, ties, unreach, handback


# ---- the model --------------------------------------------------------------------------------------------------------

def _hash_word_arrays(values):
    uniq, inv = np.unique(np.asarray(values, dtype=np.int64), return_inverse=True)
    hw = np.array([hash_words(v) for v in uniq.tolist()], dtype=np.uint64).reshape(-1, 2)
    return hw[inv, 0], hw[inv, 1]


def _pass_all_cells(cells, F, idle_limit):
    """densify_wave_cells: every occupied cell proposes its index, the smallest wins."""
    Fm = np.uint64(F - 1)
    A, B = np.zeros(F, np.uint64), np.zeros(F, np.uint64)
    occ = cells >= 0
    A[occ], B[occ] = _hash_word_arrays(cells[occ])
    step = idle = 0
    empty = int(F - occ.sum())
    while True:
        t = ((A + np.uint64(step) * B) & Fm).astype(np.int64)
        src = np.nonzero(occ & ~occ[t])[0]           # ascending: the first proposer of a cell is its smallest index
        tt, first = np.unique(t[src], return_index=True)
        src = src[first]
        cells[tt], A[tt], B[tt], occ[tt] = cells[src], A[src], B[src], True
        tot = int(tt.size)
        empty -= tot
        step += 1
        idle = 0 if tot else idle + 1
        if empty == 0:
            return False
        if idle >= idle_limit:
            return True


def model_wave(cells, S, tail=None, mutant=None):
    """The one-wavefront kernel's densification of one row.  cells: F int32, -1 = empty.  tail: whether the closed
    form may run (None: as the kernel with 16-byte aligned rows, F a multiple of 256).  Returns (cells, class)."""
    assert mutant is None or mutant in MUTANTS
    F = 1 << S
    Fm = F - 1
    cells = np.array(cells, dtype=np.int64)
    assert cells.shape == (F,)
    if tail is None:
        tail = F % 256 == 0
    idle_limit = F // 2 if mutant == "idle_half" else F
    occ = np.nonzero(cells >= 0)[0]
    n_ent = int(occ.size)
    empty = F - n_ent
    if n_ent == 0 or empty == 0:
        return cells.astype(np.int32), "none"
    if n_ent > LIST_ENTRIES:
        fix = _pass_all_cells(cells, F, idle_limit)
        return cells.astype(np.int32), "cells" + ("+fixpoint" if fix else "")
    _, U = rounds_and_window(n_ent)
    V = cells[occ].copy()
    hw = np.array([hash_words(v) for v in V.tolist()], dtype=np.uint64)
    A, B = hw[:, 0], hw[:, 1]
    mk = occ.astype(np.int64).copy()
    s = 0            # passes done
    idle = 0
    base, flags = "passes", []
    us = np.arange(U, dtype=np.uint64)[:, None]
    while True:
        # the window read: the targets of the next U passes as the cells are NOW
        tw = ((A[None, :] + (np.uint64(s) + us) * B[None, :]) & np.uint64(Fm)).astype(np.int64)
        pre = cells[tw] < 0
        wins = 0
        for u in range(U):
            if pre[u].any():
                k = np.nonzero(pre[u])[0]
                t = tw[u][k]
                live = cells[t] < 0          # (a stale "empty": the proposal changes nothing)
                k, t = k[live], t[live]
                order = np.lexsort((mk[k], t))
                k, t = k[order], t[order]
                first = np.ones(t.size, bool)
                first[1:] = t[1:] != t[:-1]
                k, t = k[first], t[first]
                cells[t] = V[k]
                if mutant != "mk_not_lowered":
                    mk[k] = np.minimum(mk[k], t)
                wins += int(k.size)
        s += U
        empty -= wins
        idle = 0 if wins else idle + U
        if empty == 0:
            break
        if idle >= idle_limit:
            flags.append("fixpoint")
            break
        if tail and empty <= TAIL_CELLS:
            tail = False                     # once
            empties = np.nonzero(cells < 0)[0]
            Tn = [int(x) for x in ((A + np.uint64(s) * B) & np.uint64(M32)).tolist()]
            writes, ties, unreach, handback = solve_tail(empties, Tn, [int(b) for b in B.tolist()], mk.tolist(), F,
                                                         tie_largest=mutant == "tie_largest")
            if handback and mutant != "no_handback":
                base = "handback"
                continue
            base = "tail"
            for c, k in writes.items():
                cells[c] = V[k]
            if ties:
                flags.append("ties")
            if unreach:
                flags.append("unreach")
            if not writes:
                flags.append("nowrite")
            break
    return cells.astype(np.int32), "+".join([base] + flags)


def expected(S, cells):
    """The oracle's cells and return code (passes, or -1 where the reference would spin)."""
    return po.densify(po.make_params(31, S, 12, 4, 0.0), cells)


# ---- designers: deterministic functions of their arguments ------------------------------------------------------------

def random_cells(S, W, n_ent, seed, vmax=None):
    """n_ent cells chosen at random, values below vmax (default 2^W)."""
    F = 1 << S
    rng = np.random.default_rng([S, W, n_ent, seed])
    cells = np.full(F, -1, np.int32)
    idx = rng.choice(F, n_ent, replace=False)
    cells[idx] = rng.integers(0, (1 << W) if vmax is None else vmax, n_ent)
    return cells


@functools.lru_cache(maxsize=None)
def _stride_zeros():
    """trailing zero bits (capped at 16) of rev64(v) for v < 2^18"""
    out = np.empty(1 << 18, np.uint8)
    for v in range(1 << 18):
        b = (po.rev64(v) & 0xFFFF) | 0x10000
        out[v] = (b & -b).bit_length() - 1
    return out


def short_orbit_pool(S, jmin):
    """values v < 2^18 whose stride rev64(v) mod 2^S has at least jmin trailing zero bits (jmin = S: stride 0)"""
    return np.nonzero(np.minimum(_stride_zeros(), S) >= jmin)[0]


def short_orbit_cells(S, n_empty, jmin, seed):
    """All cells but n_empty hold values (duplicates allowed) whose orbits are short: the stride has >= jmin trailing
    zero bits, so an entry reaches only every 2^jmin-th cell and empty cells that no orbit reaches become likely."""
    F = 1 << S
    pool = short_orbit_pool(S, jmin)
    rng = np.random.default_rng([S, n_empty, jmin, seed])
    cells = pool[rng.integers(0, pool.size, F)].astype(np.int32)
    cells[rng.choice(F, n_empty, replace=False)] = -1
    return cells


def single_value(S, v, cells):
    """copies of one value at the listed cells"""
    out = np.full(1 << S, -1, np.int32)
    out[list(cells)] = v
    return out


def poly_a_like(S, cell=0):
    """What a poly-A record leaves: value 0 in one cell.  Both hash words of 0 are 0: the orbit is cell 0 alone."""
    assert hash_words(0) == (0, 0)
    return single_value(S, 0, [cell])


def spread(S, n, seed):
    """n distinct cells, deterministic (for single_value cases)"""
    return sorted(np.random.default_rng([S, n, seed]).choice(1 << S, n, replace=False).tolist())


def all_but(S, *cells):
    return [c for c in range(1 << S) if c not in cells]


# ---- the case table ----------------------------------------------------------------------------------------------------
# (name, S, W, designer, args, expected class).  Seeds were found by search on the CPU and typed in; test_densify_ref_cpu.py
# fails when a designer or hash change moves one out of its class.
BOUNDARY_N = {
    12: (1, 2, 63, 64, 65, 128, 129, 192, 193, 256, 257, 320, 321, 384, 385),
    10: (1, 2, 63, 64, 65, 128, 129, 192, 193, 256, 257, 320, 321, 384, 385),
    8: (1, 64, 65, 128, 129, 192, 193, 240, 255),
    6: (1, 63),
    1: (1,),
}
ALL_CELLS_N = {S: (385, (1 << S) // 2, (1 << S) - 17, (1 << S) - 16, (1 << S) - 1) for S in (10, 12)}
LARGE_F_N = {S: (1, 300, (1 << S) // 2, (1 << S) - 1) for S in (13, 15, 16)}
WINDOW_ROUNDS = (1, 2, 3, 4, 5, 6)    # ceil(n_ent / 64); 5 and 6 both run the R = 6 instantiation
VMAX = (1 << 31) - 1                  # values up to 2^31 - 2

CASES = [
    # -- list boundaries: n_ent at every edge of the dispatch (R by ceil(n_ent / 64)) and of the 384-entry list
    ("bnd_s12_n1", 12, 12, random_cells, (12, 1, 0), "tail"),
    ("bnd_s12_n2", 12, 12, random_cells, (12, 2, 0), "tail"),
    ("bnd_s12_n63", 12, 12, random_cells, (12, 63, 0), "tail"),
    ("bnd_s12_n64", 12, 12, random_cells, (12, 64, 0), "tail"),
    ("bnd_s12_n65", 12, 12, random_cells, (12, 65, 0), "tail"),
    ("bnd_s12_n128", 12, 12, random_cells, (12, 128, 0), "tail"),
    ("bnd_s12_n129", 12, 12, random_cells, (12, 129, 0), "tail"),
    ("bnd_s12_n192", 12, 12, random_cells, (12, 192, 0), "tail+ties"),
    ("bnd_s12_n193", 12, 12, random_cells, (12, 193, 0), "tail"),
    ("bnd_s12_n256", 12, 12, random_cells, (12, 256, 0), "tail"),
    ("bnd_s12_n257", 12, 12, random_cells, (12, 257, 0), "tail+ties"),
    ("bnd_s12_n320", 12, 12, random_cells, (12, 320, 0), "tail"),
    ("bnd_s12_n321", 12, 12, random_cells, (12, 321, 0), "tail+ties"),
    ("bnd_s12_n384", 12, 12, random_cells, (12, 384, 0), "tail+ties"),
    ("bnd_s12_n385", 12, 12, random_cells, (12, 385, 0), "cells"),
    ("bnd_s10_n1", 10, 12, random_cells, (12, 1, 0), "tail"),
    ("bnd_s10_n2", 10, 12, random_cells, (12, 2, 0), "passes+fixpoint"),
    ("bnd_s10_n63", 10, 12, random_cells, (12, 63, 0), "tail"),
    ("bnd_s10_n64", 10, 12, random_cells, (12, 64, 0), "tail+ties"),
    ("bnd_s10_n65", 10, 12, random_cells, (12, 65, 0), "tail+ties"),
    ("bnd_s10_n128", 10, 12, random_cells, (12, 128, 0), "tail+ties"),
    ("bnd_s10_n129", 10, 12, random_cells, (12, 129, 0), "tail"),
    ("bnd_s10_n192", 10, 12, random_cells, (12, 192, 0), "tail"),
    ("bnd_s10_n193", 10, 12, random_cells, (12, 193, 0), "tail"),
    ("bnd_s10_n256", 10, 12, random_cells, (12, 256, 0), "tail+ties"),
    ("bnd_s10_n257", 10, 12, random_cells, (12, 257, 0), "tail+ties"),
    ("bnd_s10_n320", 10, 12, random_cells, (12, 320, 0), "tail"),
    ("bnd_s10_n321", 10, 12, random_cells, (12, 321, 0), "tail"),
    ("bnd_s10_n384", 10, 12, random_cells, (12, 384, 0), "tail+ties"),
    ("bnd_s10_n385", 10, 12, random_cells, (12, 385, 0), "cells"),
    ("bnd_s8_n1", 8, 12, random_cells, (12, 1, 0), "passes+fixpoint"),
    ("bnd_s8_n64", 8, 12, random_cells, (12, 64, 0), "tail+ties"),
    ("bnd_s8_n65", 8, 12, random_cells, (12, 65, 0), "tail+ties"),
    ("bnd_s8_n128", 8, 12, random_cells, (12, 128, 0), "tail+ties"),
    ("bnd_s8_n129", 8, 12, random_cells, (12, 129, 0), "tail"),
    ("bnd_s8_n192", 8, 12, random_cells, (12, 192, 0), "tail"),
    ("bnd_s8_n193", 8, 12, random_cells, (12, 193, 0), "tail"),
    ("bnd_s8_n240", 8, 12, random_cells, (12, 240, 0), "passes"),
    ("bnd_s8_n255", 8, 12, random_cells, (12, 255, 0), "passes"),
    ("bnd_s6_n1", 6, 12, random_cells, (12, 1, 0), "passes"),
    ("bnd_s6_n63", 6, 12, random_cells, (12, 63, 0), "passes"),
    ("bnd_s1_n1", 1, 12, random_cells, (12, 1, 0), "passes"),
    # -- every window instantiation: closed-form tail without and with ties, and the hand-back (every hand-back row of
    #    the table is one that the closed form would get wrong: a losing entry's index had dropped below the winner's)
    ("win_r1_tail", 10, 12, random_cells, (12, 44, 100), "tail"),
    ("win_r1_tail_ties", 10, 12, random_cells, (12, 44, 104), "tail+ties"),
    ("win_r1_handback", 10, 12, random_cells, (12, 44, 1628), "handback"),
    ("win_r2_tail", 10, 12, random_cells, (12, 108, 102), "tail"),
    ("win_r2_tail_ties", 10, 12, random_cells, (12, 108, 100), "tail+ties"),
    ("win_r2_handback", 10, 12, random_cells, (12, 108, 204), "handback"),
    ("win_r3_tail", 10, 12, random_cells, (12, 172, 100), "tail"),
    ("win_r3_tail_ties", 10, 12, random_cells, (12, 172, 101), "tail+ties"),
    ("win_r3_handback", 10, 12, random_cells, (12, 172, 213), "handback"),
    ("win_r4_tail", 10, 12, random_cells, (12, 236, 101), "tail"),
    ("win_r4_tail_ties", 10, 12, random_cells, (12, 236, 100), "tail+ties"),
    ("win_r4_handback", 10, 12, random_cells, (12, 236, 1106), "handback"),
    ("win_r5_tail", 10, 12, random_cells, (12, 300, 101), "tail"),
    ("win_r5_tail_ties", 10, 12, random_cells, (12, 300, 100), "tail+ties"),
    ("win_r5_handback", 10, 12, random_cells, (12, 300, 340), "handback"),
    ("win_r6_tail", 10, 12, random_cells, (12, 364, 100), "tail"),
    ("win_r6_tail_ties", 10, 12, random_cells, (12, 364, 101), "tail+ties"),
    ("win_r6_handback", 10, 12, random_cells, (12, 364, 124), "handback"),
    ("handback_s12", 12, 12, random_cells, (12, 150, 900), "handback"),
    ("handback_s8", 8, 12, random_cells, (12, 100, 203), "handback"),
    # -- tail boundaries: cells no orbit reaches (short orbits), 16 and 17 empty cells at the start
    ("short_tail_unreach", 8, 12, short_orbit_cells, (16, 5, 8), "tail+unreach"),
    ("short_tail_ties_unreach", 8, 12, short_orbit_cells, (12, 5, 7), "tail+ties+unreach"),
    ("short_tail_nowrite", 8, 12, short_orbit_cells, (8, 5, 19), "tail+unreach+nowrite"),
    ("short_tail_nowrite_stride0", 8, 12, short_orbit_cells, (16, 8, 0), "tail+unreach+nowrite"),
    ("short_cells_fixpoint_s10", 10, 12, short_orbit_cells, (8, 7, 1), "cells+fixpoint"),
    ("short_cells_fixpoint_s12", 12, 12, short_orbit_cells, (4, 8, 0), "cells+fixpoint"),
    ("tail_start16", 8, 12, random_cells, (12, 240, 1), "tail"),
    ("tail_start17", 8, 12, random_cells, (12, 239, 4), "tail"),
    # -- fixpoint exits (oracle rc = -1): stride 0 mod F, an even stride that fills part of the sketch, copies of one value
    ("fix_stride0_s8", 8, 12, single_value, (144, [85]), "passes+fixpoint"),
    ("fix_even_s8", 8, 12, single_value, (260, [5]), "passes+fixpoint"),
    ("fix_copies_s8", 8, 12, single_value, (46, spread(8, 5, 0)), "passes+fixpoint"),
    ("fix_stride0_s10", 10, 12, single_value, (231, [341]), "passes+fixpoint"),
    ("fix_even_s10", 10, 12, single_value, (267, [5]), "passes+fixpoint"),
    ("fix_copies_s10", 10, 12, single_value, (65, spread(10, 5, 0)), "passes+fixpoint"),
    ("fix_stride0_s12", 12, 12, single_value, (1694, [1365]), "passes+fixpoint"),
    ("fix_even_s12", 12, 12, single_value, (290, [5]), "passes+fixpoint"),
    ("fix_copies_s12", 12, 12, single_value, (84, spread(12, 5, 0)), "passes+fixpoint"),
    ("fix_stride0_s13", 13, 12, single_value, (3388, [2730]), "passes+fixpoint"),
    ("fix_even_s13", 13, 12, single_value, (303, [5]), "passes+fixpoint"),
    ("fix_copies_s13", 13, 12, single_value, (85, spread(13, 5, 0)), "passes+fixpoint"),
    ("poly_a_s8", 8, 12, poly_a_like, (77,), "passes+fixpoint"),
    ("poly_a_s10", 10, 12, poly_a_like, (), "passes+fixpoint"),
    ("poly_a_s13", 13, 12, poly_a_like, (4097,), "passes+fixpoint"),
    # -- more occupied cells than the list holds: the plain pass over all cells
    ("cells_s10_n512", 10, 12, random_cells, (12, 512, 0), "cells"),
    ("cells_s10_n1007", 10, 12, random_cells, (12, 1007, 0), "cells"),
    ("cells_s10_n1008", 10, 12, random_cells, (12, 1008, 0), "cells"),
    ("cells_s10_n1023", 10, 12, random_cells, (12, 1023, 0), "cells"),
    ("cells_s12_n2048", 12, 12, random_cells, (12, 2048, 0), "cells"),
    ("cells_s12_n4079", 12, 12, random_cells, (12, 4079, 0), "cells"),
    ("cells_s12_n4080", 12, 12, random_cells, (12, 4080, 0), "cells"),
    ("cells_s12_n4095", 12, 12, random_cells, (12, 4095, 0), "cells"),
    # -- trivial rows: they come back untouched
    ("all_empty_s1", 1, 12, single_value, (0, []), "none"),
    ("all_full_s1", 1, 12, random_cells, (12, 2, 0), "none"),
    ("all_empty_s6", 6, 12, single_value, (0, []), "none"),
    ("all_full_s6", 6, 12, random_cells, (12, 64, 0), "none"),
    ("all_empty_s8", 8, 12, single_value, (0, []), "none"),
    ("all_full_s8", 8, 12, random_cells, (12, 256, 0), "none"),
    ("all_empty_s10", 10, 12, single_value, (0, []), "none"),
    ("all_full_s10", 10, 12, random_cells, (12, 1024, 0), "none"),
    ("all_empty_s12", 12, 12, single_value, (0, []), "none"),
    ("all_full_s12", 12, 12, random_cells, (12, 4096, 0), "none"),
    ("all_empty_s13", 13, 12, single_value, (0, []), "none"),
    ("all_full_s13", 13, 12, random_cells, (12, 8192, 0), "none"),
    ("all_empty_s16", 16, 12, single_value, (0, []), "none"),
    ("all_full_s16", 16, 12, random_cells, (12, 65536, 0), "none"),
    # -- duplicates: 16 distinct values over 200 cells; every occupied cell holds the same value
    ("dup_w4_s8", 8, 4, random_cells, (4, 200, 0), "tail+ties"),
    ("dup_one_value_s8", 8, 12, single_value, (16, spread(8, 200, 1)), "tail+ties"),
    ("dup_one_value_few_s8", 8, 12, single_value, (16, spread(8, 9, 2)), "tail+ties"),
    ("dup_w4_s10", 10, 4, random_cells, (4, 200, 0), "tail+ties"),
    ("dup_one_value_s10", 10, 12, single_value, (16, spread(10, 200, 1)), "tail+ties"),
    ("dup_one_value_few_s10", 10, 12, single_value, (16, spread(10, 9, 2)), "tail+ties"),
    ("dup_w4_s12", 12, 4, random_cells, (4, 200, 0), "tail+ties"),
    ("dup_one_value_s12", 12, 12, single_value, (16, spread(12, 200, 1)), "tail+ties"),
    ("dup_one_value_few_s12", 12, 12, single_value, (16, spread(12, 9, 2)), "tail+ties"),
    # -- large values (what -G leaves: cells >= 2^W)
    ("large_s8_n100", 8, 12, random_cells, (12, 100, 0, VMAX), "tail+ties"),
    ("large_s8_n200", 8, 12, random_cells, (12, 200, 0, VMAX), "tail+ties"),
    ("large_s10_n100", 10, 12, random_cells, (12, 100, 0, VMAX), "tail"),
    ("large_s10_n300", 10, 12, random_cells, (12, 300, 0, VMAX), "tail+ties"),
    ("large_s12_n250", 12, 12, random_cells, (12, 250, 0, VMAX), "tail+ties"),
    ("large_handback_s8", 8, 12, random_cells, (12, 120, 350, VMAX), "handback"),
    ("large_const_max_s8", 8, 12, single_value, (VMAX - 1, spread(8, 40, 3)), "passes+fixpoint"),
    ("large_const_2w_s8", 8, 12, single_value, (1 << 12, spread(8, 40, 4)), "tail+ties"),
    ("large_const_max_s10", 10, 12, single_value, (VMAX - 1, spread(10, 40, 3)), "passes+fixpoint"),
    ("large_const_2w_s10", 10, 12, single_value, (1 << 12, spread(10, 40, 4)), "tail+ties"),
    # -- larger F: densify_lds<1024> (S = 13, 15) and the global-memory kernel (S = 16); W = 8: duplicates
    ("large_f_s13_n1", 13, 8, random_cells, (8, 1, 0), "tail"),
    ("large_f_s13_n300", 13, 8, random_cells, (8, 300, 0), "tail+ties"),
    ("large_f_s13_n4096", 13, 8, random_cells, (8, 4096, 0), "cells"),
    ("large_f_s13_n8191", 13, 8, random_cells, (8, 8191, 0), "cells"),
    ("large_f_s15_n1", 15, 8, random_cells, (8, 1, 1), "tail"),
    ("large_f_s15_n300", 15, 8, random_cells, (8, 300, 0), "tail+ties"),
    ("large_f_s15_n16384", 15, 8, random_cells, (8, 16384, 0), "cells"),
    ("large_f_s15_n32767", 15, 8, random_cells, (8, 32767, 0), "cells"),
    ("large_f_s16_n1", 16, 8, random_cells, (8, 1, 2), "tail"),
    ("large_f_s16_n300", 16, 8, random_cells, (8, 300, 0), "tail+ties"),
    ("large_f_s16_n32768", 16, 8, random_cells, (8, 32768, 0), "cells"),
    ("large_f_s16_n65535", 16, 8, random_cells, (8, 65535, 0), "cells"),
    # -- a fill behind more than F / 2 idle passes (no closed form at F = 64): cell 0 is reached in pass 45
    ("late_fill_s6", 6, 12, single_value, (16, all_but(6, 0)), "passes"),
]


def make_cells(case):
    name, S, W, designer, args, cls = case
    return designer(S, *args)


def cases_of(S):
    return [c for c in CASES if c[1] == S]


def batch_of(S):
    """(names, cells [n, F], expected cells [n, F], oracle rc per row) of all cases of one S; computed once."""
    return _batch_of(S)


@functools.lru_cache(maxsize=None)
def _batch_of(S):
    cs = cases_of(S)
    rows = np.stack([make_cells(c) for c in cs])
    with concurrent.futures.ThreadPoolExecutor(po.cpu_threads()) as pool:   # (the oracle runs outside the interpreter lock)
        exp = list(pool.map(lambda r: expected(S, r), rows))
    out = (tuple(c[0] for c in cs), rows, np.stack([e[0] for e in exp]), tuple(int(e[1]) for e in exp))
    for a in out[1:3]:
        a.setflags(write=False)
    return out
