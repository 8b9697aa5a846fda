"""The chunked sketch loop (nq_sketch.hip roll_records; the launch in nq_api_build.hip sketch_dev) against the oracle,
bit for bit, on the designed batches of tests/sketch_chunks.py: record lengths at the edges of the chunk rule, address
phases, dirty bytes at chunk edges, the candidate stack under full pressure, the filter-strength rule at its
boundaries, irregular parameters after niqki_select_best_H, split counts other than 32 and whole-file entries.

Every case asserts the launch shape it means to run (sketch_chunks.shape_of, held against the compiled rule by
tests/test_sketch_chunks_cpu.py) and the densification form the handle reports.  The oracle's sketches are computed
once per batch, whatever the filter mode (NIQKI_SKETCH_FILTER: "1" automatic, "n" forces n - 1 leading zeros, "0" off)."""
import numpy as np
import pytest

import sketch_chunks as sc

pytestmark = pytest.mark.gpu


def _cases(batches):
    return [pytest.param(b, mode, id="%s-mode%s" % (b.name, mode)) for b in batches for mode in b.modes]


def _compare(b, mode, sk, ref):
    assert sk.shape == ref.shape
    bad = [(i, int((sk[i] != ref[i]).sum())) for i in range(ref.shape[0]) if not np.array_equal(sk[i], ref[i])]
    assert not bad, "%s mode %s: (sketch, differing cells) %r" % (b.name, mode, bad)


def _run(native, po, monkeypatch, b, mode):
    """Batch b through the host-memory call under filter mode `mode`: shape, densify form, every sketch."""
    monkeypatch.setenv("NIQKI_SKETCH_FILTER", mode)
    plan = b.check_shape(mode)
    p, ref = sc.reference(po, b)
    e = native.Engine(K=b.K, S=b.S, W=b.W, H=b.H)
    if b.G:
        assert e.select_best_H(b.G) == p.H
    sk = e.sketch(b.records(), entry_rec=b.entry_rec())
    form = e.stat("last_densify_form")
    e.close()
    assert form == plan["form"], (b.name, mode, form)
    _compare(b, mode, sk, ref)


@pytest.mark.parametrize("b,mode", _cases(sc.LENGTH_EDGES + [sc.UNFILTERED_32]))
def test_length_edges(native, po, b, mode, monkeypatch):
    """1. One record per sketch at the lengths of the design tables: a last chunk of 1, CHUNK - 1 and CHUNK k-mers; 1, 63
    and 64 live lanes in the last row of 64 chunks (the fast full-chunk body or the predicated one); one lane with a
    round more; both sides of every change of `groups`; all eight values of `groups` inside one 1024 x 8 launch; the
    256-lane shape; and the unfiltered loop under GROUPS = 32."""
    _run(native, po, monkeypatch, b, mode)


def _dev_call(native, torch, b, shift, fill):
    """The device-buffer call with the records back to back and `seqs` at `shift` bytes past a 16-byte boundary.
    fill: what stands around the records -- the pad and the slack behind it, and the bytes before `seqs` -- zero bytes
    or random ACGT.  Returns (sketches, densify form)."""
    records = b.records()
    total = sum(r.size for r in records)
    n = total + native.SEQ_PAD + 512
    if fill:
        raw = torch.from_numpy(sc.text(n, 7_000_000).copy()).cuda()
    else:
        raw = torch.zeros(n, dtype=torch.uint8, device="cuda")
    lead = (-raw.data_ptr()) % 16 + 16 + shift
    seqs = raw[lead:lead + total + native.SEQ_PAD]
    assert seqs.data_ptr() % 16 == shift
    seqs[:total] = torch.from_numpy(np.concatenate(records)).cuda()
    off = np.zeros(len(records) + 1, np.int64)
    off[1:] = np.cumsum([r.size for r in records])
    rec_off = torch.from_numpy(off).cuda()
    er = torch.from_numpy(b.entry_rec().astype(np.int32)).cuda()
    n_entry = b.n_entry()
    sk = torch.empty((n_entry, 1 << b.S), dtype=torch.int32, device="cuda")
    e = native.Engine(K=b.K, S=b.S, W=b.W, H=b.H)
    e.set_stream(torch.cuda.current_stream().cuda_stream)
    e.sketch_dev(seqs, rec_off, len(records), sk, entry_rec=er, n_entry=n_entry)
    e.synchronize()
    out = sk.cpu().numpy()
    form = e.stat("last_densify_form")
    e.close()
    return out, form


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
@pytest.mark.parametrize("b,mode", _cases(sc.PHASES))
def test_address_phases_and_bytes_behind_the_end(native, po, b, mode, shift, monkeypatch):
    """2. Records back to back in a device buffer that starts 0..3 bytes past a 16-byte boundary: record starts of every
    residue mod 4 and five residues mod 16.  The buffer's last record has every chunk full, so the fast body, which reads
    up to 40 bytes past a chunk, runs to the buffer's very end: whether the pad and what follows hold zeroes or more
    ACGT, and whether the next record or the pad stands behind a record, the sketches are the oracle's."""
    import torch
    monkeypatch.setenv("NIQKI_SKETCH_FILTER", mode)
    plan = b.check_shape(mode)
    _, ref = sc.reference(po, b)
    for fill in (False, True):
        sk, form = _dev_call(native, torch, b, shift, fill)
        assert form == plan["form"]
        _compare(b, "%s shift %d fill %d" % (mode, shift, fill), sk, ref)


@pytest.mark.parametrize("b,mode", _cases(sc.DIRTY))
def test_dirty_bytes_at_chunk_edges(native, po, b, mode, monkeypatch):
    """3. 'N' and lower case on the last base of a chunk and the first of the next, inside the K - 1 prefix (an illegal
    byte zeroes all its digits, legal lower case is kept) and in the first K - 1 + (31 - K) bases, where the first wave
    takes the generic warm-up; K = 31, 30, 17 (the fast loop), 16 and 9 (the generic filtered one)."""
    _run(native, po, monkeypatch, b, mode)


@pytest.mark.parametrize("b,mode", _cases(sc.STACK))
def test_stack_under_full_pressure(native, po, b, mode, monkeypatch):
    """4. Runs of N, A and T longer than three rows of a wave's chunks: all 64 lanes push on every step, for thousands of
    steps, and every candidate is the zero word (candidate_update's general leading-zero form) -- in the chunked fast
    loops, the generic filtered loop (K = 16), the half-slot workgroups of S = 16 and the line loop."""
    _run(native, po, monkeypatch, b, mode)


@pytest.mark.parametrize("b,mode", _cases(sc.STRENGTH))
def test_filter_strength_boundaries(native, po, b, mode, monkeypatch):
    """5. S = 9, one record per sketch with 55, 115 and 240 k-mers per slot and one k-mer fewer: the strength changes
    between neighbours, and at H = 2, 1 and 0 the guard T <= 2^H - 1 must switch the filter off (automatic at 240 per
    slot for H = 2, always for H <= 1; forced T = 4 at H = 2), while forced T = 1 at H = 1 stays on; forced T = 6
    leaves slots without candidate and takes the exact re-run."""
    kmers = b.entry_kmers()
    assert kmers == sc.STRENGTH_KMERS
    want = {"1": {4: [0, 2, 2, 3, 3, 4], 7: [0, 2, 2, 3, 3, 4], 2: [0, 2, 2, 3, 3, 0], 1: [0] * 6, 0: [0] * 6}[b.H],
            "2": [1] * 6, "5": [0] * 6, "7": [6] * 6}[mode]
    assert [sc.strength(b.S, b.H, n, 1, int(mode)) for n in kmers] == want
    _run(native, po, monkeypatch, b, mode)


@pytest.mark.parametrize("b,mode", _cases(sc.SELECTED))
def test_long_records_after_select_best_h(native, po, b, mode, monkeypatch):
    """6. K = 31, S = 12, W = 12, H = 4, then niqki_select_best_H for a genome size of 150: H changes, the fingerprint
    parts overlap and cells exceed 2^W, so the filter and the distinct-value forms are off -- records of 20 000, 300 000
    and 2^21 + 77 bases (the three 1024-lane shapes) and an entry of three records."""
    p, ref = sc.reference(po, b)
    assert p.H != b.H and (ref >= (1 << b.W)).any()
    assert b.shape(mode)[4] is False
    _run(native, po, monkeypatch, b, mode)


@pytest.mark.parametrize("b,mode", _cases(sc.SPLITS))
def test_splits_other_than_32(native, po, b, mode, monkeypatch):
    """7. No entry_rec: 17 records of 2^20 bases and a little are cut into 30 parts each, 37 records into 13; the part
    boundaries n_chunks * part / splits are uneven.  Every record against the oracle, unfiltered ("1": a part's share
    is below 55 k-mers per slot), filtered ("4"), with the exact re-run ("7"), and with half-slot workgroups (S = 16)."""
    assert b.shape(mode)[3] == b.splits and b.splits not in (1, 32)
    _run(native, po, monkeypatch, b, mode)


@pytest.mark.parametrize("b,mode", _cases(sc.FILES))
def test_whole_file_entries(native, po, b, mode, monkeypatch):
    """8. Two sketches of six records each -- [long, K bases, K + 1, empty, 40 bases, long], and the same with the second
    long record 2 K + 1 bases behind the first: the filter strength follows the entry's total, and records of one chunk
    sit in a 1024-lane launch."""
    _run(native, po, monkeypatch, b, mode)
