"""No GPU: tests/exchange_ref.py against a triple loop, its designs against the row classes they are meant to hold, and
the product's pure plan function (niqki_group_plan_batch) against the reference's thresholds and the three rules that
decide between the sparse and the dense exchange."""
import numpy as np
import pytest

import exchange_ref as X

S, W, T = 9, 8, X.T_DESIGN
WORLDS = (2, 3, 5, 8, 16, 17, 64)


def test_partials_against_a_triple_loop():
    rng = np.random.default_rng(11)
    N, nq, F, w = 7, 4, 32, 3
    sk = rng.integers(-1, 1 << w, (N, F)).astype(np.int32)
    q = rng.integers(-1, (1 << w) + 3, (nq, F)).astype(np.int32)       # -1 and values >= 2^W among them
    assert (q < 0).any() and (q >= (1 << w)).any() and (sk < 0).any()
    for world in (1, 3, 5, 32):
        got = X.partials(sk, q, w, world)
        exp = np.zeros((world, nq, N), dtype=np.int64)
        for r in range(world):
            for i in range(nq):
                for g in range(N):
                    for s in range(F * r // world, F * (r + 1) // world):
                        if 0 <= q[i, s] < (1 << w) and sk[g, s] == q[i, s]:
                            exp[r, i, g] += 1
        assert np.array_equal(got, exp), world
        assert np.array_equal(got.sum(axis=0), X.range_counts(sk, q, w, [0, F])[0])


def test_thresholds_and_lists_from_the_definition():
    assert X.thresholds(40, 8) == (5, 2) and X.thresholds(41, 8) == (6, 3) and X.thresholds(7, 8) == (1, 1)
    assert X.thresholds(33, 8) == (5, 2) and X.thresholds(3, 3) == (1, 1)
    sk = np.array([[1, 2, 3, 4], [1, 2, 0, 0], [1, 2, 3, 0], [9, 2, 3, 4], [0, 0, 0, 0]], np.int32)
    q = np.array([[1, 2, 3, 4], [-1, -1, -1, -1]], np.int32)
    ex = X.Exchange(sk, q, 4, 2, 3)                                    # thr 2, sthr 1
    assert ex.total.tolist() == [[4, 2, 3, 3, 0], [0] * 5]
    assert ex.candidates(0, 0).tolist() == [0, 1, 2] and ex.candidates(1, 0).tolist() == [0, 3]
    assert ex.survivors(0, 0).tolist() == [0, 1, 2, 3] and ex.survivors(1, 0).tolist() == [0, 2, 3]
    off, c, g = ex.lists()
    assert off.tolist() == [0, 3, 3] and c.tolist() == [4, 3, 3] and g.tolist() == [0, 3, 2]     # the tie: gid descending
    assert ex.expected_overflow(3, 4) is False and ex.expected_overflow(2, 4) is True and ex.expected_overflow(3, 3) is True


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("which", (0, 1))
def test_design_holds_every_row_class(world, which):
    """From the partial counts of the arrays alone: each of the rows a-j is there, in every full query."""
    ms = X.designed_min_scores(world, T)[which]
    d = X.designed(world, S, W, T, ms)
    qp, per = X.pad_queries(d.q, world)
    assert d.q.shape[0] % world != 0 and qp.shape[0] > d.q.shape[0]            # j: padding rows
    ex = X.Exchange(d.sk, qp, W, world, ms)
    thr, sthr = ex.thr, ex.sthr
    assert (thr, sthr) == (T, 2)
    assert (world * (thr - 1) == ms - 1) if which == 0 else (world * thr == ms)
    p, tot = ex.p, ex.total
    cut = X.cuts(1 << S, world)
    widths = np.diff(cut)
    assert widths.min() >= thr
    if world in (3, 5, 17):
        assert widths[-1] != widths[0]                                        # h: the last rank's width differs
    full = [j for j in range(X.N_QUERIES) if j not in (X.EMPTY_QUERY, X.NO_HIT_QUERY)]
    cand_rank_seen = set()
    for j in full:
        valid = (d.q[j] >= 0) & (d.q[j] < (1 << W))
        vw = np.array([valid[cut[r]:cut[r + 1]].sum() for r in range(world)])
        col = lambda g: p[:, j, g]
        is_c = lambda g: col(g) >= thr
        # a
        g, = d.gids(j, "a")
        assert is_c(g).sum() == 1 and (np.sort(col(g))[:-1] == thr - 1).all() and col(g).max() == thr
        assert tot[j, g] == world * (thr - 1) + 1 and (tot[j, g] == ms) == (which == 0)
        cand_rank_seen.add(int(np.argmax(col(g))))
        # b
        g, = d.gids(j, "b")
        assert (col(g) == thr - 1).all() and tot[j, g] == (ms - 1 if which == 0 else ms - world)
        # c
        g, = d.gids(j, "c")
        assert is_c(g).any() and tot[j, g] == ms - 1
        # d
        gs = d.gids(j, "d")
        assert len(gs) == 2
        for g in gs:
            assert tot[j, g] == ms and is_c(g).any()
            weak = (col(g) >= 1) & (col(g) < sthr)
            assert weak.sum() == 1                                            # the store count of that rank decides
            assert tot[j, g] - col(g)[weak][0] < ms
            if world >= 3:
                assert (col(g) == 0).any()
            if world <= 17:
                assert is_c(g).sum() == 1                                     # (world 64: a shard of 8 slots is too narrow)
        assert np.argmax(col(gs[0]) >= thr) != np.argmax(col(gs[1]) >= thr)
        # e
        gs = d.gids(j, "e")
        seen = set()
        for g in gs:
            assert tot[j, g] == ms and is_c(g).any()
            seen |= set(col(g)[~is_c(g)].tolist()) & {sthr, sthr - 1}
        assert seen == {sthr, sthr - 1}
        if world >= 3:
            assert any({sthr, sthr - 1} <= set(col(g)[~is_c(g)].tolist()) for g in gs)
        # f
        g, = d.gids(j, "f")
        assert (col(g) == thr).all() and tot[j, g] == world * thr and (tot[j, g] == ms) == (which == 1)
        # g
        gs = d.gids(j, "g")
        assert len(gs) == 3 and len({int(tot[j, g]) for g in gs}) == 1 and tot[j, gs[0]] >= ms
        assert len({tuple(col(g).tolist()) for g in gs}) == 3
        # h
        gs = d.gids(j, "h")
        assert col(gs[0])[-1] == vw[-1] and tot[j, gs[0]] == vw[-1]
        if vw[-1] < ms:
            assert len(gs) == 2 and col(gs[1])[-1] == vw[-1] and tot[j, gs[1]] == ms
        # i
        g, = d.gids(j, "i")
        assert np.array_equal(col(g), vw) and tot[j, g] == valid.sum()
        assert (tot[j, g] == 1 << S) == (j not in X.BAD_CELL_QUERIES)
        # a genome of one query matches no other query anywhere
        mine = [g_ for (jj, _, _, g_) in d.rows if jj == j]
        others = np.setdiff1d(np.arange(d.sk.shape[0]), mine)
        assert (tot[j, others] == 0).all()
    assert cand_rank_seen == {j % world for j in full} and len(cand_rank_seen) >= min(world, 7)   # the roles move over the ranks
    # cells that are never queried or indexed
    assert (d.sk == -1).any()
    for j in X.BAD_CELL_QUERIES:
        assert (d.q[j] == -1).any() and (d.q[j] >= (1 << W)).any()
    # j
    assert (d.q[X.EMPTY_QUERY] == -1).all() and ex.n_surv[:, X.EMPTY_QUERY].sum() == 0
    assert ex.n_cand[:, X.NO_HIT_QUERY].sum() > 0 and (tot[X.NO_HIT_QUERY] < ms).all()
    assert ex.n_surv[:, d.q.shape[0]:].sum() == 0                                # padding rows
    off = ex.lists()[0]
    assert off[-1] > 80 and not ex.expected_overflow(64, 1024)


@pytest.mark.parametrize("world", (3, 8))
def test_capacity_design(world):
    ms = X.designed_min_scores(world, T)[0]
    d = X.designed_capacity(world, S, W, ms)
    C, SC = X.CAND_CAP, X.SURV_CAP
    assert (C, SC) == (8, 16) and X.CAP_QUERIES == ("at cap", "cand + 1", "surv + 1")

    def batch(rows):
        return X.Exchange(d.sk, X.pad_queries(d.q[rows], world)[0], W, world, ms)
    at = batch([0])
    assert at.n_cand.max() == C and at.n_surv.max() == SC and int(np.argmax(at.n_cand[:, 0])) != int(np.argmax(at.n_surv[:, 0]))
    assert not at.expected_overflow(C, SC) and at.expected_overflow(C - 1, SC) and at.expected_overflow(C, SC - 1)
    c1 = batch([1])
    assert c1.n_cand.max() == C + 1 and c1.n_surv.max() <= SC and c1.expected_overflow(C, SC)
    s1 = batch([2])
    assert s1.n_surv.max() == SC + 1 and s1.n_cand.max() <= C and s1.expected_overflow(C, SC) and not s1.expected_overflow(C, 32)
    al = batch([0, 1, 2])
    assert al.expected_overflow(C, SC)
    for b in (at, c1, s1):
        assert b.lists()[0][-1] >= 4                                             # every query has hits


def rule_sparse(world, min_score, option, cand_cap):
    """the three rules of the plan, as the issue of the protocol states them"""
    sparse = option == 1 or (option == 0 and min_score >= 4 * world)
    if min_score < world:
        sparse = False
    if world * cand_cap > 4096:
        sparse = False
    return int(sparse)


def test_group_plan_follows_the_reference(native):
    per, N = 3, 300
    for world, ms, option, cand_cap in X.group_cases(T):
        plan = native.group_plan(world, S, ms, option, per, N, cand_cap)
        thr, sthr = X.thresholds(ms, world)
        assert (plan.cand_threshold, plan.surv_threshold) == (thr, sthr), (world, ms)
        assert plan.sparse == rule_sparse(world, ms, option, cand_cap), (world, ms, option, cand_cap)
    want = {(w, 1): 1 for w in (2, 3, 5, 8, 16)}
    want[(17, 1)] = 0
    for world, ms, option, cand_cap in X.group_cases(T):
        if cand_cap == 256 and option == 1 and ms >= world:
            assert native.group_plan(world, S, ms, option, per, N, cand_cap).sparse == want[(world, 1)]
    for world in (2, 3, 8, 17, 64):
        cc = 64 if world == 64 else 32
        # option 0 ("choose"): sparse from min_score = 4 * world on
        assert native.group_plan(world, S, 4 * world - 1, 0, per, N, cc).sparse == 0
        assert native.group_plan(world, S, 4 * world, 0, per, N, cc).sparse == 1
        # option 1 ("sparse"): dense all the same while min_score < world (the candidate threshold must be >= 1)
        assert native.group_plan(world, S, world - 1, 1, per, N, cc).sparse == 0
        assert native.group_plan(world, S, world, 1, per, N, cc).sparse == 1
        assert native.group_plan(world, S, 4 * world, 2, per, N, cc).sparse == 0
    # world * cand_cap: 4096 ids per query are the most cand_hits_kernel orders
    for world, cc, sparse in ((16, 256, 1), (64, 64, 1), (2, 2048, 1), (3, 1366, 0), (17, 256, 0), (2, 2050, 0)):
        assert world * cc in (4096, 4098, 4352, 4100)
        assert native.group_plan(world, S, 5 * world, 1, per, N, cc).sparse == sparse, (world, cc)
        assert native.group_plan(world, S, 5 * world, 0, per, N, cc).sparse == sparse, (world, cc)
