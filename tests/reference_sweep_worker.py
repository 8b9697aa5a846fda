"""The REAL reference (oracle/_ref/libniqki_ref.so through pyoracle.Ref) over lists of cases, in a child process
of its own: the reference never returns from records whose sketch it cannot finish densifying, so whoever asks runs
it under a time limit.  CPU only: nothing here opens a GPU.

As a module: the seeded case and record generators shared by oracle/make_goldens_sweep.py (which records the
reference's outputs into tests/golden/reference_sweep.*) and tests/test_oracle_vs_reference.py (which compares the
oracle with the live reference where it has been built), and run_reference(), which starts the child.

As a program:  reference_sweep_worker.py JOB OUT      cases of JOB (pickle) -> results in OUT (pickle)
               reference_sweep_worker.py --one JOB    one compute_sketch; prints "ready" right before the call and
                                                      "done" after it (the hang predictor's other direction)
"""
import gzip
import hashlib
import json
import os
import pickle
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ACGT = np.frombuffer(b"ACGT", np.uint8)
FULL = np.frombuffer(b"ACGTacgtNnRY-\r", np.uint8)
NON_ACGT = np.frombuffer(b"Nnacgt-RY\r", np.uint8)   # (lower case is foreign to the rolling update: src/niqki_index.cpp:211-221)
VERBATIM_MAX = 4096                                  # longer records are named by their generator arguments
MAX_LEFT_OUT = 0.15


# ---- records ---------------------------------------------------------------------------------------------------

def depends_on_bsr0(K, seq):
    """True when a record can reach get_fingerprint(0) -- the reference's bsr on 0, whose result is undefined
    (src/niqki_index.cpp:199-206).  Only a canonical word of 0 hashes to 0 (revhash64 is a bijection with 0 -> 0):
    any byte outside upper-case ACGT (zero in both code tables), A x K or T x K."""
    b = bytes(seq)
    return bool(b.translate(None, b"ACGT")) or b"A" * K in b or b"T" * K in b


def clean(rng, L):
    return ACGT[rng.integers(0, 4, L)].copy()


def mutate(rng, s, rate):
    t = s.copy()
    m = rng.random(t.size) < rate
    t[m] = ACGT[rng.integers(0, 4, int(m.sum()))]
    return t


def synth(native, args):
    return native.synth_genome_host(*[int(a) for a in args])


def make_records(rng, native, K, seed, clean_only, long_len=20000, huge=False):
    """The records of one case: [(seq uint8, synth args or None)].  Lengths K+1, K+2, 60, 150, 200, 201, 300, 1000 and
    (long_len != 0) two related records of long_len bases from niqki_synth_genome_host, (huge) one of 300 000;
    alphabets clean, mixed case, with N, and everything a FASTA file may hold; a foreign byte inside the first K-1
    bases; a run of >= K foreign bytes.  clean_only (the constructor's H >= 7): upper-case ACGT throughout, without
    A x K and T x K -- nothing may depend on bsr(0)."""
    def pick(make):
        for _ in range(64):
            s = make()
            if not clean_only or not depends_on_bsr0(K, s):
                return s
        raise AssertionError("no record without a canonical-zero k-mer at K=%d" % K)

    recs = [(pick(lambda: clean(rng, K + 1)), None), (pick(lambda: clean(rng, K + 2)), None)]
    if clean_only:
        for L in (60, 150, 300, 150, 300):
            recs.append((pick(lambda: clean(rng, L)), None))
    else:
        s = clean(rng, 60)
        s[rng.random(60) < 0.3] |= 0x20                                   # mixed case
        recs.append((s, None))
        s = clean(rng, 150)
        s[rng.integers(K, 150, 3)] = ord("N")                             # N past the prefix
        recs.append((s, None))
        s = clean(rng, 300)
        at = rng.integers(0, 300, 30)
        s[at] = FULL[rng.integers(0, FULL.size, 30)]                      # the whole alphabet
        recs.append((s, None))
        s = clean(rng, 150)
        if K > 1:
            s[int(rng.integers(0, K - 1))] = NON_ACGT[int(rng.integers(0, NON_ACGT.size))]   # inside the first K-1 bases
        recs.append((s, None))
        s = clean(rng, 300)
        a, n = int(rng.integers(20, 200)), K + int(rng.integers(0, 6))
        s[a:a + n] = NON_ACGT[rng.integers(0, NON_ACGT.size, n)]          # >= K foreign bytes: canonical word 0
        recs.append((s, None))
    recs.append((pick(lambda: clean(rng, 200)), None))
    recs.append((pick(lambda: clean(rng, 201)), None))
    base = pick(lambda: clean(rng, 1000))
    recs.append((base, None))
    recs.append((pick(lambda: mutate(rng, base, 0.03)), None))
    member = [0]

    def next_synth(rate, L):
        def make():
            args = [seed, seed % 1000, member[0], rate if member[0] else 0, L]
            member[0] += 1
            make.args = args
            return synth(native, args)
        s = pick(make)
        return s, make.args
    if long_len:
        recs.append(next_synth(0, long_len))
        recs.append(next_synth(200, long_len))
    if huge:
        recs.append(next_synth(120, 300_000))
    return recs


def will_return(po, p, seq):
    """The oracle's prediction: the reference's compute_sketch returns on this record (its drivers skip records of
    up to K bases; its densification spins forever where no pass can fill the last cells)."""
    if len(seq) <= p.K:
        return False
    return po.densify(p, po.sketch_accumulate(p, seq))[1] >= 0


# ---- cases -----------------------------------------------------------------------------------------------------

def random_case(rng, max_S=12):
    """Seeded random parameters over what niqki_create accepts with S + W <= 20 (a reference constructor allocates
    24 bytes per bucket: 25 MB there), H up to W."""
    W = int(rng.integers(1, 16))
    H = int(rng.integers(0, W + 1))
    K = int(rng.integers(1, 32)) if rng.random() < 0.8 else 31
    # (2^W fingerprint values, 4^K / 2 canonical words: far fewer of either than cells, and the reference finishes no
    # sketch at all -- there S stays small, as in the designed rows)
    S = int(rng.integers(1, min(max_S, 20 - W, 3 if W <= 2 else max_S, 2 * K) + 1))
    J = float(rng.choice([0.0, 0.1, 0.33, 0.9]))
    G = 0.0
    if W >= 6 and rng.random() < 0.25:            # (select_best_H tries H = 2..6: W - H must not wrap)
        G = float(rng.choice([3.0, 150.0, 1e4, 5e6]))
    if H >= 7:
        K = max(K, 12)                            # (A x K / T x K must be rare enough to leave records)
    return dict(K=K, S=S, W=W, H=H, J=J, G=G)


def case_records(native, po, case, seed, long_len=20000, huge=False):
    """-> (kept records [(seq, synth args)], generated, left out) of one case."""
    rng = np.random.default_rng(seed)
    clean_only = case["H"] >= 7
    recs = make_records(rng, native, case["K"], seed, clean_only, long_len, huge)
    p = po.make_params(case["K"], case["S"], case["W"], case["H"], case["J"], genome_size=case["G"])
    kept = [r for r in recs if will_return(po, p, r[0])]
    if clean_only:
        for s, _ in kept:
            assert case["K"] >= 8 and not depends_on_bsr0(case["K"], s), case
    return kept, len(recs), len(recs) - len(kept)


# ---- the recorded sweep (tests/golden/reference_sweep.*, written by oracle/make_goldens_sweep.py) ----------------

def load_sweep():
    gold = os.path.join(ROOT, "tests", "golden")
    vec = np.load(os.path.join(gold, "reference_sweep.npz"))
    with open(os.path.join(gold, "reference_sweep.json")) as f:
        meta = json.load(f)
    return vec, meta


def case_tag(i, m):
    return "case %d (seed %d): K=%d S=%d W=%d H=%d J=%g G=%g" % (i, m["seed"], m["K"], m["S"], m["W"], m["H"], m["J"], m["G"])


def sweep_records(native, po, vec, m):
    """The input records of a recorded case; generated ones are checked against their recorded checksum."""
    out = []
    for r in m["records"]:
        if "verbatim" in r:
            i = r["verbatim"]
            s = vec["seqs"][int(vec["seq_off"][i]):int(vec["seq_off"][i + 1])]
        else:
            s = synth(native, r["synth"])
            assert "%016x" % po.fnv1a64(s) == r["fnv"], ("generated record differs from the recorded one", r)
        assert s.size == r["len"]
        out.append(s)
    return out


def check_sketches(po, vec, i, m, sk, tag):
    """sk (n, F) int32 against the reference's recorded sketches of case i (F > 1024: checksum and first 8 cells)."""
    if "sketch_fnv" in m:
        fnv = ["%016x" % po.fnv1a64(s) for s in sk]
        bad = [j for j in range(len(fnv)) if fnv[j] != m["sketch_fnv"][j]]
        assert not bad and len(fnv) == len(m["sketch_fnv"]), (tag, "records", bad, [m["records"][j]["len"] for j in bad])
        assert np.array_equal(sk[:, :8], vec["head_%03d" % i]), tag
    else:
        exp = vec["sk_%03d" % i].astype(np.int32)
        bad = [j for j in range(len(exp)) if not np.array_equal(sk[j], exp[j])]
        assert not bad and sk.shape == exp.shape, (tag, "records", bad, [m["records"][j]["len"] for j in bad])


def recorded_hits(vec, m, q):
    n = vec["hit_n"][m["q0"]:m["q0"] + len(m["records"])].astype(np.int64)
    lo = m["h0"] + int(n[:q].sum())
    return vec["hit_counts"][lo:lo + int(n[q])], vec["hit_gids"][lo:lo + int(n[q])].astype(np.uint32)


def dump_names(n):
    """The names the harness gave the reference's genomes: they end its dump."""
    return "".join("g%d\n" % i for i in range(n)).encode()


# ---- the child -------------------------------------------------------------------------------------------------

def run_reference(cases, timeout):
    """cases: [dict(K,S,W,H,J,G, records=[uint8 arrays])] -> [dict(min_score, H_final, sketches (n, F) int32,
    hit_n, hit_counts, hit_gids, dump_len, dump_md5)] from the reference's own Index, one per case, computed by a
    child process that is killed after `timeout` seconds (subprocess.TimeoutExpired)."""
    with tempfile.TemporaryDirectory() as td:
        job, out = os.path.join(td, "job.pkl"), os.path.join(td, "out.pkl")
        with open(job, "wb") as f:
            pickle.dump(cases, f)
        env = dict(os.environ, OMP_NUM_THREADS="1")
        subprocess.run([sys.executable, os.path.abspath(__file__), job, out], check=True, timeout=timeout, env=env,
                       stdout=subprocess.DEVNULL)
        with open(out, "rb") as f:
            return pickle.load(f)


def _reference_case(po, c, td):
    r = po.Ref(K=c["K"], S=c["S"], W=c["W"], H=c["H"], J=c["J"], out_path=os.path.join(td, "scratch.gz"))
    if c["G"]:
        r.select_best_H(c["G"])
    recs = c["records"]
    sk = np.stack([r.compute_sketch(s) for s in recs]) if recs else np.zeros((0, 1 << c["S"]), np.int32)
    for i, s in enumerate(sk):
        r.insert(s, "g%d" % i)
    hit_n, hc, hg = [], [np.zeros(0, np.uint32)], [np.zeros(0, np.uint32)]
    for s in sk:
        a, b = r.query(s)
        hit_n.append(len(a))
        hc.append(a)
        hg.append(b)
    path = os.path.join(td, "idx.gz")
    r.dump(path)
    with gzip.open(path, "rb") as f:
        raw = f.read()
    res = dict(min_score=int(r.min_score()), H_final=int(r.H), sketches=sk, hit_n=np.array(hit_n, np.uint32),
               hit_counts=np.concatenate(hc).astype(np.uint32), hit_gids=np.concatenate(hg).astype(np.uint32),
               dump_len=len(raw), dump_md5=hashlib.md5(raw).hexdigest())
    r.close()
    return res


def main(argv):
    from oracle import pyoracle as po
    assert po.have_ref(), "oracle/_ref/libniqki_ref.so is not built"
    if argv[0] == "--one":
        with open(argv[1], "rb") as f:
            c = pickle.load(f)
        with tempfile.TemporaryDirectory() as td:
            r = po.Ref(K=c["K"], S=c["S"], W=c["W"], H=c["H"], J=0.0, out_path=os.path.join(td, "scratch.gz"))
            print("ready", flush=True)
            r.compute_sketch(c["records"][0])
            print("done", flush=True)
        return 0
    with open(argv[0], "rb") as f:
        cases = pickle.load(f)
    # select_best_H prints to the C stdout: keep it away from whoever reads ours
    devnull = os.open(os.devnull, os.O_WRONLY)
    os.dup2(devnull, 1)
    with tempfile.TemporaryDirectory() as td:
        results = [_reference_case(po, c, td) for c in cases]
    with open(argv[1], "wb") as f:
        pickle.dump(results, f)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
