"""GPU: every densification form against the serial loop (oracle, nqo_densify) on the designed cells of
tests/densify_ref.py -- list boundaries, every window instantiation with and without ties, hand-backs, unreachable cells,
fixpoint exits, duplicates, large values -- and, through low-complexity records, the two distinct-value forms.  All cases
of one S go to the device in ONE niqki_densify call, rows of mixed classes side by side; equality is bit for bit, the
oracle's rc < 0 rows included.  Every run asserts the form it took (stat "last_densify_form")."""
import numpy as np
import pytest

import densify_ref as dr

pytestmark = pytest.mark.gpu

WAVE, PLAIN, DISTINCT, DISTINCT_LATE, GLOBAL = 1, 2, 3, 4, 5   # last_densify_form
SMALL_S = (1, 6, 8, 10, 12)


def check(S, got, what, sel=None):
    names, rows, exp, rc = dr.batch_of(S)
    if sel is not None:
        names, rows, exp, rc = [names[i] for i in sel], rows[sel], exp[sel], [rc[i] for i in sel]
    assert got.shape == exp.shape
    bad = [names[i] for i in range(len(names)) if not np.array_equal(got[i], exp[i])]
    assert not bad, (what, S, bad)
    for i, n in enumerate(names):      # (implied by the equality; states what a densified row is)
        occ = rows[i] >= 0
        assert np.array_equal(got[i][occ], rows[i][occ]), (what, n)
        assert set(got[i][got[i] >= 0].tolist()) <= set(rows[i][occ].tolist()), (what, n)
        assert (rc[i] < 0) == bool((got[i] < 0).any()), (what, n)


def engine(native, S, **kw):
    return native.Engine(K=31, S=S, W=12, H=4, **kw)


@pytest.mark.parametrize("S", SMALL_S)
def test_host_rows_wave_kernel(native, S):
    """default: sketch_reads_kernel with its 384-entry list; rows of the workspace are 16-byte aligned, so S >= 8 runs
    the closed-form tail"""
    e = engine(native, S)
    assert e.stat("last_densify_form") == 0
    got = e.densify(dr.batch_of(S)[1])
    assert e.stat("last_densify_form") == WAVE
    check(S, got, "host rows")
    # a batch of one row, and an empty one
    one = e.densify(dr.batch_of(S)[1][-1:])
    assert e.stat("last_densify_form") == WAVE and np.array_equal(one[0], dr.batch_of(S)[2][-1])
    none = e.densify(np.empty((0, 1 << S), np.int32))
    assert none.shape == (0, 1 << S) and e.stat("last_densify_form") == 0
    e.close()


@pytest.mark.parametrize("S", SMALL_S)
def test_host_rows_workgroup_kernel(native, monkeypatch, S):
    """NIQKI_SKETCH_WAVE=0: sketch_kernel<256> with densify_lds"""
    monkeypatch.setenv("NIQKI_SKETCH_WAVE", "0")
    e = engine(native, S)
    got = e.densify(dr.batch_of(S)[1])
    assert e.stat("last_densify_form") == PLAIN
    check(S, got, "NIQKI_SKETCH_WAVE=0")
    e.close()


@pytest.mark.parametrize("S", SMALL_S)
def test_device_rows_in_place_aligned_and_not(native, S):
    """NIQKI_MEM_DEVICE on a torch tensor: once 16-byte aligned, once starting 4 bytes into the allocation -- the second
    runs the single-cell loops and never the closed-form tail, and gives the same cells"""
    import torch
    rows = dr.batch_of(S)[1]
    n, F = rows.shape
    e = engine(native, S)
    e.set_stream(torch.cuda.current_stream().cuda_stream)
    for shift in (0, 1):
        buf = torch.full((n * F + 4,), -7, dtype=torch.int32, device="cuda")
        view = buf[shift:shift + n * F]
        assert view.data_ptr() % 16 == 4 * shift
        view.copy_(torch.from_numpy(rows.reshape(-1).copy()))
        e.densify_dev(view, n)
        e.synchronize()
        assert e.stat("last_densify_form") == WAVE
        host = buf.cpu().numpy()
        check(S, host[shift:shift + n * F].reshape(n, F), "device rows + %d bytes" % (4 * shift))
        assert (host[:shift] == -7).all() and (host[shift + n * F:] == -7).all()   # nothing beside the rows is touched
    e.close()


@pytest.mark.parametrize("S", SMALL_S)
def test_handle_after_select_best_h(native, po, S):
    """-G leaves irregular fingerprint parameters and cells >= 2^W; densification takes any cells"""
    e = engine(native, S)
    assert e.select_best_H(5e6) == po.select_best_H(5e6, S, 12, 4)
    got = e.densify(dr.batch_of(S)[1])
    assert e.stat("last_densify_form") == WAVE
    check(S, got, "after select_best_H")
    e.close()


@pytest.mark.parametrize("S,form,single", [(13, PLAIN, False), (15, PLAIN, False), (16, GLOBAL, False), (16, GLOBAL, True)])
def test_larger_sketches(native, S, form, single):
    """densify_lds<1024> in the workgroup kernel (S = 13, 15), densify_global_kernel (S = 16).  The S = 16 row with ONE
    occupied cell is a case of its own: 2^16 passes of one workgroup over global memory, one cell filled per pass, take
    28 s on an MI355X (the oracle's 2^32 cell visits 8 .. 15 s beside them); the other S = 16 rows together 1 s."""
    names = dr.batch_of(S)[0]
    lone = [i for i, n in enumerate(names) if n == "large_f_s16_n1"]
    sel = lone if single else [i for i in range(len(names)) if i not in lone]
    assert sel
    e = engine(native, S)
    got = e.densify(dr.batch_of(S)[1][sel])
    assert e.stat("last_densify_form") == form
    check(S, got, "host rows", sel)
    e.close()


# ---- the distinct-value forms, through records -----------------------------------------------------------------------

def low_complexity_records():
    rng = np.random.default_rng(11)
    alpha = np.frombuffer(b"ACGT", np.uint8)
    recs = []
    for period in range(1, 13):
        unit = alpha[np.arange(period) % 4] if period <= 4 else alpha[rng.integers(0, 4, period)]
        rep = np.tile(unit, 600 // period + 1)[:600].copy()
        recs.append(rep)
        sub = rep.copy()
        sub[301] = alpha[(int(np.nonzero(alpha == sub[301])[0][0]) + 1) % 4]   # one substitution
        recs.append(sub)
    for L in (450, 700, 2000):
        recs.append(alpha[rng.integers(0, 4, L)].copy())
    return recs


@pytest.mark.parametrize("S,W,form", [(10, 4, DISTINCT), (10, 8, DISTINCT), (13, 11, DISTINCT),
                                      (14, 12, DISTINCT_LATE), (14, 6, DISTINCT_LATE), (15, 12, DISTINCT_LATE),
                                      (10, 12, PLAIN)])
def test_records_distinct_value_forms(native, po, S, W, form):
    """Tandem repeats of period 1..12 (poly-A: a fixpoint exit), the same with one substitution, random records; all
    longer than 415 bases, so the one-wavefront kernel is not chosen.  densify_lds_distinct where 4 * 2^W <= 2^S and
    S <= 13, densify_distinct_kernel at S = 14, 15, the plain passes where the values are many against the cells."""
    H = min(4, W // 2)
    recs = low_complexity_records()
    assert sum(len(r) for r in recs) // len(recs) > 415
    p = po.make_params(31, S, W, H, 0.0)
    # po.densify(po.sketch_accumulate(record)) per record, on the oracle's threads: a repeat occupies a handful of cells, and
    # the serial loop then takes thousands of passes over all 2^S of them
    exp = po.sketch_batch(p, *native.Engine.pack_records(recs), threads=po.cpu_threads())
    assert np.array_equal(exp[1], po.densify(p, po.sketch_accumulate(p, recs[1]))[0])
    spins = (exp < 0).any(axis=1)                                   # the oracle's rc < 0: cells no orbit reaches
    assert spins[0] and not spins.all()                             # poly-A leaves cells empty; others fill up
    e = native.Engine(K=31, S=S, W=W, H=H)
    got = e.sketch(recs)
    assert e.stat("last_densify_form") == form
    bad = [i for i in range(len(recs)) if not np.array_equal(got[i], exp[i])]
    assert not bad, (S, W, bad, spins[bad].tolist())
    e.close()
