"""The candidate drain of the filtered fast loops (nq_sketch.hip candidate_update: both hashes finished from x1, the
word after the first round of the filter's hash) against the oracle, on what ordinary text almost never holds:
planted k-mers whose hash is tiny.  canon = unrev(h) for a small h has hash h: poly-A (h = 0, x1 = 0, hash 0, slot 0)
and hashes with a zero high word, which take the whole-wave clz64 branch of the fingerprint.

S = 12, W = 12, H = 4; candidate filter automatic ("1") and forced to three leading zeros ("4").  Three cases, each on
the loop it names (asserted from the shape rule of sketch_dev / sketch_plan, restated in _shape()):
  * one 2^18-base record: the chunked fast loop of sketch_kernel<1024, 8, 31>, whose last round of chunks is partial
    and takes the generic steps beside it;
  * one 2^21-base entry passed with entry_rec: the line loop of sketch_kernel<1024, 32, 31>;
  * the same with K = 21: the line loop of sketch_kernel<1024, 32, 0>.

Every reference is computed once, for both filter modes."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

S, W, H = 12, 12, 4
MODES = ["1", "4"]
M64 = (1 << 64) - 1
C = 0xD6E8FEB86659FD93
U = 0xCFEE444D8B59A89B
SEED = 20261018   # of the text around the planted k-mers
_cache = {}

# K = 31: every h < 256 whose unrev(h) is a canonical 31-mer (35 of them, h = 0 among them).
# K = 21: unrev(h) < 4^21 holds for one h in 2^22, so the hashes come from a search done once: the 35 smallest h
# whose unrev(h) is a canonical 21-mer.  All are below 2^29; _planted() checks each of them.
H21 = [0, 2049564, 4099128, 25956654, 45750787, 49887102, 60909371, 64379229, 78653785, 86309187, 89858192, 112219710,
       126009781, 158524266, 163280627, 165824603, 172618374, 175538128, 176123173, 191572807, 199213896, 200223835,
       213080685, 216207399, 220619931, 224439420, 225898570, 240903536, 243833154, 254047658, 269006146, 303872547,
       307908322, 314949088, 332537411]


def _mix64(x, c):
    x = ((x ^ (x >> 32)) * c) & M64
    x = ((x ^ (x >> 32)) * c) & M64
    return x ^ (x >> 32)


def _revcomp(x, K):
    r = 0
    for i in range(K):
        r = (r << 2) | (3 - ((x >> (2 * i)) & 3))
    return r


def _slot(canon):
    x = ((canon ^ (canon >> 32)) * U) & M64
    x = ((x ^ (x >> 32)) * U) & M64
    return x >> (64 - S)


def _planted(K):
    """(hash, canonical k-mer) pairs: 35 for either K, in distinct slots at S = 12."""
    out = []
    for h in (range(256) if K == 31 else H21):
        canon = _mix64(h, U)
        assert _mix64(canon, C) == h
        if K != 31:
            assert canon < (1 << (2 * K)) and canon < _revcomp(canon, K), h
        if canon < (1 << (2 * K)) and canon < _revcomp(canon, K):
            out.append((h, canon))
    assert len(out) == 35 and out[0] == (0, 0)
    assert len({_slot(c) for _, c in out}) == 35
    assert all(h < (1 << 32) for h, _ in out)   # a zero high word of the hash
    return out


def _record(K, n):
    """n bases of seeded random ACGT text with the planted k-mers written over it, spread over the record; most of
    them straddle the end of a 128-byte line."""
    rng = np.random.default_rng(SEED + K)
    r = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n, dtype=np.uint8)].copy()
    pl = _planted(K)
    for i, (_, canon) in enumerate(pl):
        at = (i + 1) * (n // (len(pl) + 2)) // 128 * 128 - (i * 7) % 40
        assert K <= at and at + K + 2 < n
        codes = [(canon >> (2 * (K - 1 - j))) & 3 for j in range(K)]
        r[at:at + K] = np.frombuffer(b"ACGT", np.uint8)[codes]
    return r


def _ref(po, K, n):
    """(record, oracle sketch), once per case.  A condition on the reference alone: at least 32 of the 35 planted
    hashes are the value of their slot before densification (a random k-mer with 15 or more leading zeros can beat
    one: 0.3 expected at 2^21 bases)."""
    if (K, n) not in _cache:
        p = po.make_params(K, S, W, H, 0.0)
        r = _record(K, n)
        acc = po.sketch_accumulate(p, r)
        won = sum(int(acc[_slot(canon)]) == po.fingerprint(h, W, H) for h, canon in _planted(K))
        assert won >= 32, (K, n, won)
        _cache[(K, n)] = (r, po.densify(p, acc)[0])
    return _cache[(K, n)]


def _shape(K, total, n_entry, entry_rec):
    """(BLOCK, GROUPS, KFIX, line loop) of the sketch launch: sketch_dev's cut into parts (nq_api_build.hip) and
    sketch_plan's thresholds on the average bases per workgroup (nq_sketch_plan.h)."""
    avg = total // n_entry
    splits = min(32, 512 // n_entry) if (not entry_rec and n_entry < 128 and avg >= (1 << 20)) else 1
    avg //= splits
    assert avg >= 16384
    groups = 2 if avg < (1 << 18) else 8 if avg < (1 << 21) else 32
    return 1024, groups, 31 if K == 31 else 0, groups == 32 and 17 <= K <= 31


@pytest.mark.parametrize("mode", MODES)
def test_chunked_fast_loop(native, po, mode, monkeypatch):
    monkeypatch.setenv("NIQKI_SKETCH_FILTER", mode)
    n = 1 << 18
    assert _shape(31, n, 1, False) == (1024, 8, 31, False)
    r, ref = _ref(po, 31, n)
    e = native.Engine(K=31, S=S, W=W, H=H)
    sk = e.sketch([r])
    e.close()
    assert np.array_equal(sk[0], ref), mode


@pytest.mark.parametrize("K", [31, 21])
@pytest.mark.parametrize("mode", MODES)
def test_line_loop(native, po, K, mode, monkeypatch):
    monkeypatch.setenv("NIQKI_SKETCH_FILTER", mode)
    n = 1 << 21
    assert _shape(K, n, 1, True) == (1024, 32, 31 if K == 31 else 0, True)
    r, ref = _ref(po, K, n)
    e = native.Engine(K=K, S=S, W=W, H=H)
    sk = e.sketch([r], entry_rec=np.array([0, 1], np.uint32))
    e.close()
    assert np.array_equal(sk[0], ref), (K, mode)
