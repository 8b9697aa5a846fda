"""GPU: the slot-shard exchange (niqki_group_*, niqki_amd/csrc/nq_group.hip) on designed sketches, against the plain
reference tests/exchange_ref.py -- never against another engine call.

All ranks run in this process on one device (local transport).  The designs put chosen partial counts on chosen ranks:
counts exactly at the candidate and survivor thresholds and one below, sums exactly at min_score that hinge on one
rank's count from the sketch store, the same id under every rank, ties, the last rank's odd width, lists exactly at and
one over `cand_cap` / `surv_cap`, world sizes on both sides of the 4096-ids limit, and the row-free step calls at
their largest shapes.  tests/test_exchange_ref_cpu.py checks the designs and the reference themselves."""
import numpy as np
import pytest

import exchange_ref as X
from hit_designs import first_difference, reference_lists

pytestmark = pytest.mark.gpu

S, W, T = 9, 8, X.T_DESIGN
E_INVALID = 1
SENTINEL = -0x21524111          # 0xDEADBEEF as int32


def make_group(native, world, min_score, sk, S_=S, tile_genomes=0, **options):
    """`world` shards on this device, the index inserted through the group in two ragged batches"""
    import torch
    dev = torch.device("cuda")
    F = 1 << S_
    engines = []
    for r in range(world):
        b, e = native.group_slot_range(r, world, S_)
        assert (b, e) == (F * r // world, F * (r + 1) // world)
        eng = native.Engine(K=31, S=S_, W=W, H=3, min_score_value=min_score, slot_begin=b, slot_end=e, tile_genomes=tile_genomes)
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        engines.append(eng)
    grp = native.Group(engines)
    assert grp.stat("transport") == 0
    for k, v in options.items():
        grp.set_option(k, v)
    N = sk.shape[0]
    ins_per = max(1, -(-N // (2 * world)) + 1)
    for a in range(0, N, world * ins_per):
        blk = sk[a:a + world * ins_per]
        pad = np.full((world * ins_per, F), -1, np.int32)
        pad[:blk.shape[0]] = blk
        grp.insert_dev([torch.from_numpy(pad[r * ins_per:(r + 1) * ins_per].copy()).to(dev) for r in range(world)], ins_per, blk.shape[0])
    assert all(e.n_genomes == N for e in engines)
    return engines, grp


def close_all(engines, grp):
    grp.close()
    for e in engines:
        e.close()


def local_rows(qp, per, world):
    import torch
    return [torch.from_numpy(qp[r * per:(r + 1) * per].copy()).to("cuda") for r in range(world)]


def joined(res):
    """per-rank (off, counts, gids) -> the lists of all rows of the batch, rank after rank"""
    off, cs, gs = [np.zeros(1, np.int64)], [], []
    for o, c, g in res:
        o = np.asarray(o).astype(np.int64)
        off.append(o[1:] + off[-1][-1])
        cs.append(np.asarray(c)[:o[-1]])
        gs.append(np.asarray(g)[:o[-1]])
    return np.concatenate(off), np.concatenate(cs), np.concatenate(gs)


def query_and_compare(grp, sk, q, world, min_score):
    """one host-output query of the whole batch, sized for the whole answer; -> the reference Exchange"""
    qp, per = X.pad_queries(q, world)
    ex = X.Exchange(sk, qp, W, world, min_score)
    exp = ex.lists()
    res = grp.query(local_rows(qp, per, world), per, capacity=int(exp[0][-1]) + 1)
    diff = first_difference(joined(res), exp)
    assert diff is None, diff
    return ex


@pytest.mark.parametrize("which", (0, 1))
@pytest.mark.parametrize("world", (2, 3, 5, 8, 16, 17))
def test_designed_rows_sparse_requested(native, world, which):
    """Rows a-j at both thresholds, exchange = 1.  World 17 * cand_cap 256 passes the 4096 ids cand_hits_kernel orders:
    the plan turns dense there, and sparse stays on up to world 16."""
    ms = X.designed_min_scores(world, T)[which]
    d = X.designed(world, S, W, T, ms)
    engines, grp = make_group(native, world, ms, d.sk, exchange=1)
    assert grp.stat("sparse") == (1 if world <= 16 else 0)
    ex = query_and_compare(grp, d.sk, d.q, world, ms)
    assert not ex.expected_overflow(256, 1024) and grp.stat("overflows") == 0
    assert ex.lists()[0][-1] > 80
    close_all(engines, grp)


def test_world_64_at_the_id_limit(native):
    """64 shards with cand_cap 64: world * cand_cap is exactly 4096, still sparse; host outputs, rows a-j at the first
    threshold.  This is the one world-64 case of the module (64 shard handles on one device are its costliest set-up:
    0.2 s of the module's 3 s).  World 65 is refused."""
    world = 64
    ms = X.designed_min_scores(world, T)[0]
    d = X.designed(world, S, W, T, ms)
    engines, grp = make_group(native, world, ms, d.sk, exchange=1, cand_cap=64)
    assert grp.stat("sparse") == 1
    ex = query_and_compare(grp, d.sk, d.q, world, ms)
    assert not ex.expected_overflow(64, 1024) and grp.stat("overflows") == 0
    with pytest.raises(native.NiqkiError) as ei:
        native.Group(engines[:1], first_rank=0, world=65)
    assert ei.value.code == E_INVALID
    close_all(engines, grp)


@pytest.mark.parametrize("option,kind", [(2, "first"), (2, "second"), (0, "4w-1"), (0, "4w")])
@pytest.mark.parametrize("world", (3, 8))
def test_dense_and_chosen_exchange(native, world, option, kind):
    """exchange = 2 (dense) at both thresholds; exchange = 0 (choose) on both sides of min_score = 4 * world"""
    ms = {"first": X.designed_min_scores(world, T)[0], "second": X.designed_min_scores(world, T)[1],
          "4w-1": 4 * world - 1, "4w": 4 * world}[kind]
    d = X.designed(world, S, W, X.thresholds(ms, world)[0], ms)
    engines, grp = make_group(native, world, ms, d.sk, exchange=option)
    assert grp.stat("sparse") == (1 if kind == "4w" else 0)
    ex = query_and_compare(grp, d.sk, d.q, world, ms)
    assert grp.stat("overflows") == 0 and ex.lists()[0][-1] > 80
    close_all(engines, grp)


def test_sparse_request_below_world_turns_dense(native):
    """min_score 7 < world 8: the candidate threshold would be 0 on some split, so the plan goes dense"""
    world, ms = 8, 7
    d = X.designed(world, S, W, 1, ms)
    engines, grp = make_group(native, world, ms, d.sk, exchange=1)
    assert grp.stat("sparse") == 0
    ex = query_and_compare(grp, d.sk, d.q, world, ms)
    assert grp.stat("overflows") == 0 and ex.lists()[0][-1] > 80
    close_all(engines, grp)


@pytest.mark.parametrize("world", (3, 8))
def test_lists_at_and_over_their_caps(native, world):
    """cand_cap 8, surv_cap 16: 8 candidates and 16 survivors fit; 9 candidates, 17 survivors, and the three queries
    together each make every rank redo the batch densely, exactly once -- and the lists are right every time"""
    ms = X.designed_min_scores(world, T)[0]
    d = X.designed_capacity(world, S, W, ms)
    C, SC = X.CAND_CAP, X.SURV_CAP
    engines, grp = make_group(native, world, ms, d.sk, exchange=1, cand_cap=C, surv_cap=SC)
    assert grp.stat("sparse") == 1
    seen = []
    for rows in ([0], [1], [2], [0, 1, 2]):
        before = grp.stat("overflows")
        ex = query_and_compare(grp, d.sk, d.q[rows], world, ms)
        assert grp.stat("overflows") - before == (1 if ex.expected_overflow(C, SC) else 0), rows
        seen.append(grp.stat("overflows"))
    assert seen == [0, 1, 2, 3]
    grp.set_option("surv_cap", 32)                      # 17 survivors fit
    ex = query_and_compare(grp, d.sk, d.q[[2]], world, ms)
    assert not ex.expected_overflow(C, 32) and grp.stat("overflows") == 3
    close_all(engines, grp)


def test_shards_of_several_tiles(native):
    """tile_genomes 256, 600 genomes, world 3: the rows of query 0 lie on consecutive ids around the first tile border,
    the other queries' rows anywhere, so candidates and survivors of a query come from all three tiles"""
    world, N = 3, 600
    ms = X.designed_min_scores(world, T)[0]
    d = X.designed(world, S, W, T, ms, n_genomes=N, border=256)
    g0 = sorted(g for (j, _, _, g) in d.rows if j == 0)
    assert g0[0] < 256 <= g0[-1] and g0 == list(range(g0[0], g0[-1] + 1))
    engines, grp = make_group(native, world, ms, d.sk, tile_genomes=256, exchange=1)
    ex = query_and_compare(grp, d.sk, d.q, world, ms)
    assert all(e.stat("tiles") == 3 for e in engines)
    tiles_c = {int(g) // 256 for r in range(world) for g in ex.candidates(r, 0)}
    assert tiles_c == {0, 1}
    assert {int(g) // 256 for r in range(world) for g in ex.survivors(r, 1)} == {0, 1, 2}
    assert grp.stat("sparse") == 1 and grp.stat("overflows") == 0
    close_all(engines, grp)


@pytest.mark.parametrize("option", (1, 2))
@pytest.mark.parametrize("world", (3, 8))
def test_device_outputs_with_too_little_room(native, world, option):
    """query_dev into buffers one entry short of the fullest rank's answer (and half of it): hit_off exact, every entry
    in front of `capacity` right, nothing written behind it; then the begin / end halves with room for everything"""
    import torch
    ms = X.designed_min_scores(world, T)[0]
    d = X.designed(world, S, W, T, ms)
    engines, grp = make_group(native, world, ms, d.sk, exchange=option)
    assert grp.stat("sparse") == (1 if option == 1 else 0)
    qp, per = X.pad_queries(d.q, world)
    ex = X.Exchange(d.sk, qp, W, world, ms)
    exp = reference_lists(ex.total, ms)
    loc = local_rows(qp, per, world)
    rank_lists = [reference_lists(ex.total[r * per:(r + 1) * per], ms) for r in range(world)]
    fullest = max(int(rl[0][-1]) for rl in rank_lists)
    assert fullest > 10

    def run(capacity, halves):
        room = capacity + 16
        off = [torch.full((per + 1,), -1, dtype=torch.int64, device="cuda") for _ in range(world)]
        hc = [torch.full((room,), SENTINEL, dtype=torch.int32, device="cuda") for _ in range(world)]
        hg = [torch.full((room,), SENTINEL, dtype=torch.int32, device="cuda") for _ in range(world)]
        if halves:
            grp.query_begin_dev(loc, per, off, hc, hg, capacity)
            grp.query_end()
        else:
            grp.query_dev(loc, per, off, hc, hg, capacity)
        for e in engines:
            e.synchronize()
        torch.cuda.synchronize()
        for r in range(world):
            eo, ec, eg = rank_lists[r]
            assert np.array_equal(off[r].cpu().numpy(), eo), (r, capacity)
            n = min(int(eo[-1]), capacity)
            c, g = hc[r].cpu().numpy(), hg[r].cpu().numpy()
            assert np.array_equal(c[:n], ec[:n]) and np.array_equal(g[:n], eg[:n]), (r, capacity)
            assert (c[n:] == SENTINEL).all() and (g[n:] == SENTINEL).all(), (r, capacity)

    run(fullest - 1, False)
    run(fullest // 2, False)
    run(fullest, True)
    assert int(exp[0][-1]) == sum(int(rl[0][-1]) for rl in rank_lists) and grp.stat("overflows") == 0
    close_all(engines, grp)


# ---- the row-free step calls on one handle ----------------------------------------------------------------------------

STEP_N, STEP_MS = 3000, 20
PAL_IN = (0, 0, 1, 2, 3, 4, 5, 8, 10, 20)          # matches inside the slots [F/4, F/2)
PAL_OUT = (0, 12, 17, 18, 19, 20, 20, 22, 30, 40)  # ... and outside them


def step_design():
    """3000 genomes that hold query 0's value in PAL_IN[g % 10] slots of [F/4, F/2) and PAL_OUT[g // 10 % 10] slots outside,
    fillers and -1 elsewhere.  Queries: 0; the empty one; 0 with every other slot a cell that is never queried."""
    F, filler = 1 << S, (1 << W) - 1
    rng = np.random.default_rng(41)
    q = np.stack([X.query_values(0, F, W)] * 3)
    q[1] = -1
    q[2, 0::4] = -1
    q[2, 2::4] = 1 << W
    sk = np.full((STEP_N, F), filler, np.int32)
    sk[rng.random((STEP_N, F)) < 0.03] = -1
    inside = np.arange(F // 4, F // 2)
    outside = np.setdiff1d(np.arange(F), inside)
    for g in range(STEP_N):
        pick = np.concatenate([rng.choice(inside, PAL_IN[g % 10], replace=False), rng.choice(outside, PAL_OUT[g // 10 % 10], replace=False)])
        sk[g, pick] = q[0, pick]
    return sk, q


@pytest.fixture(scope="module")
def step_case():
    sk, q = step_design()
    F = 1 << S
    counts = {(0, F): X.range_counts(sk, q, W, [0, F])[0], (F // 4, F // 2): X.range_counts(sk, q, W, [F // 4, F // 2])[0]}
    whole = counts[(0, F)]
    assert np.array_equal(whole[0], np.array([PAL_IN[g % 10] + PAL_OUT[g // 10 % 10] for g in range(STEP_N)]))
    assert (whole[1] == 0).all() and 0 < whole[2].sum() < whole[0].sum()
    for a in counts.values():
        a.setflags(write=False)
    return sk, q, counts


def survivor_lists(cnt, sthr, SC, rng, keep=()):
    """[nq][SC][2] {id, count} of the genomes with count >= sthr, in a random order, and their numbers.  Where more than
    SC qualify the list holds SC of them, those of `keep` first (what a shard's list holds after it overflowed: the
    look-up has to count the others from the sketch store)."""
    nq = cnt.shape[0]
    surv = np.full((nq, SC, 2), -7, np.int32)
    n = np.zeros(nq, np.int32)
    for i in range(nq):
        ids = rng.permutation(np.flatnonzero(cnt[i] >= sthr))
        ids = np.concatenate([[g for g in keep if g in ids], [g for g in ids if g not in keep]]).astype(np.int64)[:SC]
        surv[i, :ids.size, 0] = ids
        surv[i, :ids.size, 1] = cnt[i, ids]
        n[i] = ids.size
    return surv, n


@pytest.mark.parametrize("shard", ("whole", "quarter"))
def test_row_free_steps_at_their_limits(native, step_case, shard):
    """niqki_survivor_counts and niqki_hits_from_candidates on a whole-range handle and on a shard of a quarter of the
    slots: 4096 ids with a 4096-entry survivor table (the largest LDS shapes), m = 1, 3, 4095, all ids equal, all
    ids -1, and the refusals one past the limits.  Survivor lists and totals are made from the reference's counts of
    that slot range."""
    import torch
    sk, q, counts = step_case
    F = 1 << S
    sb, se = (0, F) if shard == "whole" else (F // 4, F // 2)
    cnt, whole = counts[(sb, se)], counts[(0, F)]
    nq = q.shape[0]
    rng = np.random.default_rng(5 + sb)
    e = native.Engine(K=31, S=S, W=W, H=3, min_score_value=STEP_MS, slot_begin=sb, slot_end=se)
    e.set_stream(torch.cuda.current_stream().cuda_stream)
    e.insert(sk)
    dq = torch.from_numpy(q).to("cuda")
    sthr = 10 if shard == "whole" else 3

    def counts_of(ids, m, SC, sthr_, keep=()):
        surv, ns = survivor_lists(cnt, sthr_, SC, rng, keep)
        out = torch.full((nq, max(m, 1)), 0x5555, dtype=torch.int16, device="cuda")
        e.survivor_counts_dev(dq, nq, torch.from_numpy(ids).to("cuda"), m, torch.from_numpy(surv).to("cuda"),
                              torch.from_numpy(ns).to("cuda"), SC, out)
        e.synchronize()
        got = out.cpu().numpy().view(np.uint16).astype(np.int64)
        exp = np.where(ids >= 0, np.take_along_axis(cnt, np.maximum(ids, 0).astype(np.int64), axis=1), 0)
        assert np.array_equal(got, exp), (m, SC, np.argwhere(got != exp)[:4].tolist())
        return ns

    # m = 4096, surv_cap 4096: every genome once (survivors, weak ones with and without a match), -1s, duplicates
    m = 4096
    ids = np.empty((nq, m), np.int32)
    for i in range(nq):
        ids[i] = np.concatenate([rng.permutation(STEP_N), np.full(96, -1), rng.integers(0, STEP_N, m - STEP_N - 96)])
        ids[i] = ids[i][rng.permutation(m)]
    ns = counts_of(ids, m, 4096, sthr)
    weak = (cnt[0] < sthr)
    assert ns[0] > 1024 and ns[1] == 0 and (weak & (cnt[0] > 0)).sum() > 100 and (cnt[0] == 0).sum() > 50
    assert 0 < ns[2] < ns[0]
    # m = 4095, 3 and 1 (not powers of two), a small table
    counts_of(ids[:, :4095].copy(), 4095, 4096, sthr)
    strong = int(np.argmax(cnt[0])), int(np.flatnonzero((cnt[0] > 0) & (cnt[0] < sthr))[0]), int(np.flatnonzero(cnt[0] == 0)[0])
    few = np.array([[strong[0], strong[1], strong[2]], [strong[0], -1, strong[0]], [strong[1], strong[1], strong[1]]], np.int32)
    assert cnt[0, strong[0]] >= sthr > cnt[0, strong[1]]
    assert counts_of(few, 3, 16, sthr, keep=strong[:1])[0] == 16            # a full table that holds the first id
    counts_of(few, 3, 16, sthr)                                            # ... and most likely none of them
    assert counts_of(few[:, :1].copy(), 1, 2, sthr, keep=strong[:1])[0] == 2
    # refused: one past the limits
    surv, ns = survivor_lists(cnt, sthr, 4097, rng)
    d_surv, d_ns = torch.from_numpy(surv).to("cuda"), torch.from_numpy(ns).to("cuda")
    big_ids = torch.full((nq, 4097), -1, dtype=torch.int32, device="cuda")
    big_out = torch.zeros((nq, 4097), dtype=torch.int16, device="cuda")
    for m_, sc_ in ((4097, 4096), (4096, 4097)):
        with pytest.raises(native.NiqkiError) as ei:
            e.survivor_counts_dev(dq, nq, big_ids, m_, d_surv, d_ns, sc_, big_out)
        assert ei.value.code == E_INVALID

    # hits from candidates: ids and the whole index's totals of them
    def hits_of(ids, tot):
        m_ = ids.shape[1]
        cap = nq * m_
        h_off = torch.full((nq + 1,), -1, dtype=torch.int64, device="cuda")
        hc = torch.full((cap,), SENTINEL, dtype=torch.int32, device="cuda")
        hg = torch.full((cap,), SENTINEL, dtype=torch.int32, device="cuda")
        e.hits_from_candidates_dev(torch.from_numpy(ids).to("cuda"), torch.from_numpy(tot.astype(np.uint16).view(np.int16)).to("cuda"),
                                   nq, m_, h_off, hc, hg, cap)
        e.synchronize()
        rows = np.zeros((nq, STEP_N), np.int64)                     # what was offered: distinct ids with their totals
        for i in range(nq):
            ok = ids[i] >= 0
            rows[i, ids[i][ok]] = tot[i][ok]
        exp = reference_lists(rows, STEP_MS)
        diff = first_difference((h_off.cpu().numpy(), hc.cpu().numpy(), hg.cpu().numpy()), exp)
        assert diff is None, diff
        assert (hc.cpu().numpy()[int(exp[0][-1]):] == SENTINEL).all()
        return exp

    tot = np.where(ids >= 0, np.take_along_axis(whole, np.maximum(ids, 0).astype(np.int64), axis=1), 0)
    exp = hits_of(ids, tot)
    n0 = int(exp[0][1])
    c0 = exp[1][:n0]
    assert n0 > 2048 and (c0 == STEP_MS).sum() > 100 and (whole[0] == STEP_MS - 1).sum() > 100        # at min_score and one below
    assert np.unique(c0).size < n0 // 20                                                           # ties all over
    assert exp[0][2] == exp[0][1] and exp[0][3] > exp[0][2]
    best = int(np.argmax(whole[0]))
    at_ms = int(np.flatnonzero(whole[0] == STEP_MS)[0])
    below = int(np.flatnonzero(whole[0] == STEP_MS - 1)[0])
    same = np.array([[best] * 3, [at_ms] * 3, [below] * 3], np.int32)
    tot3 = np.array([[whole[0, best]] * 3, [STEP_MS] * 3, [STEP_MS - 1] * 3])
    exp = hits_of(same, tot3)
    assert np.diff(exp[0]).tolist() == [1, 1, 0]
    exp = hits_of(np.full((nq, 3), -1, np.int32), np.zeros((nq, 3), np.int64))
    assert exp[0][-1] == 0
    with pytest.raises(native.NiqkiError) as ei:
        e.hits_from_candidates_dev(big_ids, big_out, nq, 4097, torch.zeros(nq + 1, dtype=torch.int64, device="cuda"),
                                   torch.zeros(8, dtype=torch.int32, device="cuda"), torch.zeros(8, dtype=torch.int32, device="cuda"), 8)
    assert ei.value.code == E_INVALID
    e.close()


# ---- S = 15: counts of 2^15 through the packed pairs -------------------------------------------------------------------

@pytest.mark.parametrize("option", (1, 2))
def test_s15_counts_of_two_to_the_15(native, option):
    """World 2 at S = 15: a genome equal to the query in all 2^15 slots, its neighbour in the same u32 word of the dense
    exchange at 2^15 - 1 (one query) or 0 (another): a carry between the u16 halves would show in either."""
    S15, world, ms = 15, 2, 100
    F, filler = 1 << S15, (1 << W) - 1
    rng = np.random.default_rng(15)
    q = np.stack([X.query_values(j, F, W) for j in range(3)])
    sk = np.full((8, F), filler, np.int32)
    sk[0, rng.random(F) < 0.1] = -1
    sk[1, :150] = q[0, :150]                  # a plain hit of query 0, all of it on rank 0
    sk[2] = q[0]                              # (2, 3): 2^15 in the low half, 2^15 - 1 beside it
    sk[3] = q[0]
    sk[3, F // 2 + 5] = filler
    sk[4] = q[1]                              # (4, 5): 2^15 beside 0
    sk[6] = q[2]                              # (6, 7): 2^15 in the high half, 2^15 - 1 below it
    sk[6, 9] = -1
    sk[7] = q[2]
    want = np.zeros((3, 8), np.int64)
    want[0, 1:4] = (150, F, F - 1)
    want[1, 4] = F
    want[2, 6:8] = (F - 1, F)
    qp, per = X.pad_queries(q, world)
    ex = X.Exchange(sk, qp, W, world, ms)
    assert np.array_equal(ex.total[:3], want) and (ex.p[:, 1, 4] == F // 2).all()
    engines, grp = make_group(native, world, ms, sk, S_=S15, exchange=option)
    assert grp.stat("sparse") == (1 if option == 1 else 0)
    exp = ex.lists()
    res = grp.query(local_rows(qp, per, world), per, capacity=int(exp[0][-1]) + 1)
    diff = first_difference(joined(res), exp)
    assert diff is None, diff
    assert exp[1].tolist() == [F, F - 1, 150, F, F, F - 1] and grp.stat("overflows") == 0
    close_all(engines, grp)
