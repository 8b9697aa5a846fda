"""The line-aligned sketch loop (nq_sketch.hip roll_records_lines, geometry in nq_sketch_lines.h) against the oracle,
as test_candidate_filter_is_exact does: S = 10, W = 12, candidate filter automatic ("1") and forced to three leading
zeros ("4").

The loop serves the 1024 x 32 launch shape: an average of at least 2^21 bases per workgroup.  A call with few sketches
and one record each is cut into parts (nq_api_build.hip sketch_dev), which divides that average, so the cases here pass
`entry_rec` (one record per sketch where nothing else is said): whole-file mode is never cut.  Only the split case
goes without, with a record long enough for 32 parts of 2^21.

Sequences are slices of one random text and every reference is computed once, for both filter modes."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LONG = 1 << 21
MODES = ["1", "4"]
_cache = {}


def _text(n, at=0):
    """n bases of one seeded random ACGT text, from position `at`."""
    if "text" not in _cache:
        rng = np.random.default_rng(20261017)
        _cache["text"] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (1 << 26) + (1 << 22), dtype=np.uint8)]
    assert at + n <= _cache["text"].size
    return _cache["text"][at:at + n]


def _ref(po, key, K, S, records):
    """Oracle sketch of one entry made of `records`, computed once per key."""
    if key not in _cache:
        p = po.make_params(K, S, 12, 4, 0.0)
        if len(records) == 1:
            _cache[key] = po.compute_sketch(p, records[0])
        else:
            acc = np.full(1 << S, -1, np.int32)
            for r in records:
                po.sketch_accumulate(p, r, acc)
            _cache[key] = po.densify(p, acc)[0]
    return _cache[key]


def _one_per_sketch(n):
    return np.arange(n + 1, dtype=np.uint32)


@pytest.mark.parametrize("mode", MODES)
def test_record_starts_cover_the_residues(native, po, mode, monkeypatch):
    """Records back to back, lengths 2^21 + {0, 1, 3, 15, 17, 63, 65, 127} and two more: the starts are 0, 0, 1, 4, 19,
    36, 99, 36, 35 and 66 past a multiple of 128 -- residues 0, 1 and 3 mod 4 from the eight lengths and 2 from the
    tenth record, several residues mod 16, and at 99 a first line with 29 < K - 1 bytes."""
    monkeypatch.setenv("NIQKI_SKETCH_FILTER", mode)
    extra = [0, 1, 3, 15, 17, 63, 65, 127, 31, 5]
    recs, at = [], 0
    for x in extra:
        recs.append(_text(LONG + x, at))
        at += LONG + x
    e = native.Engine(K=31, S=10, W=12, H=4)
    sk = e.sketch(recs, entry_rec=_one_per_sketch(len(recs)))
    e.close()
    for i, r in enumerate(recs):
        assert np.array_equal(sk[i], _ref(po, ("starts", i), 31, 10, [r])), (mode, i)


@pytest.mark.parametrize("mode", MODES)
def test_kmer_count_edges(native, po, mode, monkeypatch):
    """Records of 16 * 131072 - 1, 16 * 131072 and 16 * 131072 + 1 k-mers (the last k-mer of a record is skipped:
    n = len - K): 2^21 hash bytes are 16 384 lines when the record starts on a line, one line per lane and sixteen
    lanes' worth; one k-mer less or more moves the ragged end."""
    monkeypatch.setenv("NIQKI_SKETCH_FILTER", mode)
    recs = [_text(16 * 131072 + d + 31, 1000 * (d + 2)) for d in (-1, 0, 1)]
    e = native.Engine(K=31, S=10, W=12, H=4)
    sk = e.sketch(recs, entry_rec=_one_per_sketch(3))
    e.close()
    for i, r in enumerate(recs):
        assert np.array_equal(sk[i], _ref(po, ("edges", i), 31, 10, [r])), (mode, i)


def _dev_call(native, torch, K, S, records, shift, entry_rec):
    """The device-buffer call with `seqs` at `shift` bytes past a 128-byte aligned address.  Returns the sketches."""
    total = sum(r.size for r in records)
    raw = torch.zeros(total + native.SEQ_PAD + 256, dtype=torch.uint8, device="cuda")
    lead = (-raw.data_ptr()) % 128 + shift
    seqs = raw[lead:lead + total + native.SEQ_PAD]
    assert seqs.data_ptr() % 128 == shift % 128
    seqs[:total] = torch.from_numpy(np.concatenate(records)).cuda()
    off = np.zeros(len(records) + 1, np.int64)
    off[1:] = np.cumsum([r.size for r in records])
    rec_off = torch.from_numpy(off).cuda()
    er = torch.from_numpy(entry_rec.astype(np.int32)).cuda()
    n_entry = entry_rec.size - 1
    sk = torch.empty((n_entry, 1 << S), dtype=torch.int32, device="cuda")
    e = native.Engine(K=K, S=S, W=12, H=4)
    e.set_stream(torch.cuda.current_stream().cuda_stream)
    e.sketch_dev(seqs, rec_off, len(records), sk, entry_rec=er, n_entry=n_entry)
    e.synchronize()
    out = sk.cpu().numpy()
    e.close()
    return out


@pytest.mark.parametrize("mode", MODES)
def test_dirty_bytes_at_line_edges(native, po, mode, monkeypatch):
    """'N' and lower-case bytes on the last byte of a line, on the first byte of the next, and inside the K - 1 prefix
    (which zeroes all its digits).  The buffer is 128-byte aligned here, so buffer offsets are line offsets."""
    import torch
    monkeypatch.setenv("NIQKI_SKETCH_FILTER", mode)
    r = _text(LONG + 5, 777).copy()
    for line, tail, head in ((3, b"N", b"a"), (500, b"c", b"N"), (9000, b"g", b"t"), (16383, b"N", b"N")):
        r[128 * line + 127] = tail[0]
        r[128 * line + 128] = head[0]
    r[200_000:200_040] = ord("N")
    r[7] = ord("n")   # inside the prefix, and no legal prefix character
    r2 = _text(LONG + 5, 777).copy()
    r2[3] = ord("g")  # a legal lower-case prefix character
    r2[130:140] = np.frombuffer(b"acgtNacgtn", np.uint8)
    sk = _dev_call(native, torch, 31, 10, [r, r2], 0, _one_per_sketch(2))
    assert np.array_equal(sk[0], _ref(po, "dirty0", 31, 10, [r])), mode
    assert np.array_equal(sk[1], _ref(po, "dirty1", 31, 10, [r2])), mode


@pytest.mark.parametrize("K", [21, 17])
@pytest.mark.parametrize("mode", MODES)
def test_other_k(native, po, K, mode, monkeypatch):
    """K = 21 and K = 17 (the smallest K of the fast loop): table entries, forward mask and the warm-up's reach depend on K."""
    monkeypatch.setenv("NIQKI_SKETCH_FILTER", mode)
    recs = [_text(LONG + 77, 31), _text(LONG + 100, 5_000_003)]
    e = native.Engine(K=K, S=10, W=12, H=4)
    sk = e.sketch(recs, entry_rec=_one_per_sketch(2))
    e.close()
    for i, r in enumerate(recs):
        assert np.array_equal(sk[i], _ref(po, ("k", K, i), K, 10, [r])), (K, mode, i)


@pytest.mark.parametrize("mode", MODES)
def test_whole_file_mode_with_tiny_records(native, po, mode, monkeypatch):
    """One sketch of four records: a long one, one of K bases (no k-mer: the last one is skipped), one of K + 1 (one
    k-mer, one line, one lane), and a long one whose start is 2 * K + 1 past the first one's end."""
    monkeypatch.setenv("NIQKI_SKETCH_FILTER", mode)
    recs = [_text(LONG + 11, 123), _text(31, 9_000_000), _text(32, 9_100_000), _text(LONG + 130, 4_400_000)]
    e = native.Engine(K=31, S=10, W=12, H=4)
    sk = e.sketch(recs, entry_rec=np.array([0, 4], np.uint32))
    e.close()
    assert np.array_equal(sk[0], _ref(po, "file", 31, 10, recs)), mode


@pytest.mark.parametrize("mode", MODES)
def test_split_record_alone_and_in_a_batch(native, po, mode, monkeypatch):
    """A record of 2^26 + 77 bases alone in a call is cut into 32 parts of 2^21 bases each (every part is a range of the
    record's lines); inside a whole-file call it is one workgroup's.  Both equal the oracle."""
    monkeypatch.setenv("NIQKI_SKETCH_FILTER", mode)
    big = _text((1 << 26) + 77, 50)
    e = native.Engine(K=31, S=10, W=12, H=4)
    alone = e.sketch([big])[0]
    batch = e.sketch([_text(LONG + 3, 99), big], entry_rec=_one_per_sketch(2))[1]
    e.close()
    ref = _ref(po, "big", 31, 10, [big])
    assert np.array_equal(alone, batch), mode
    assert np.array_equal(alone, ref), mode


@pytest.mark.parametrize("mode", MODES)
def test_bench_parameters(native, po, mode, monkeypatch):
    """One 2^21-base record at the benchmark's S = 15."""
    monkeypatch.setenv("NIQKI_SKETCH_FILTER", mode)
    r = _text(LONG, 2_000_000)
    e = native.Engine(K=31, S=15, W=12, H=4)
    sk = e.sketch([r], entry_rec=_one_per_sketch(1))
    e.close()
    assert np.array_equal(sk[0], _ref(po, "bench", 31, 15, [r])), mode


@pytest.mark.parametrize("shift", [1, 61, 127])
@pytest.mark.parametrize("mode", MODES)
def test_buffer_offsets(native, po, shift, mode, monkeypatch):
    """The device-buffer call with `seqs` 1, 61 and 127 bytes past a 128-byte aligned address: the first line of the
    buffer starts before it and the last one ends behind its pad -- neither may be loaded whole."""
    import torch
    monkeypatch.setenv("NIQKI_SKETCH_FILTER", mode)
    recs = [_text(LONG + 33, 1_000_000), _text(LONG + 64, 3_300_000)]
    sk = _dev_call(native, torch, 31, 10, recs, shift, _one_per_sketch(2))
    for i, r in enumerate(recs):
        assert np.array_equal(sk[i], _ref(po, ("shift", i), 31, 10, [r])), (shift, mode, i)
