"""CPU: the reference of the niqki_unite tests (tests/unite_ref.py) against a plain loop, and the algebra the feature
rests on against the oracle: a cell holds the smallest fingerprint seen in its slot, so the per-slot minimum over a
group's member sketches is the sketch of the group's pooled records."""
import numpy as np

from unite_ref import PAN_GROUPS, designed_labelings, launch_constants, number_labels, oracle_pan_sketches, unite_ref


def loop_ref(sk, labels):
    number, ids = {}, []
    for lab in labels:
        ids.append(number.setdefault(int(lab), len(number)))
    u = [[-1] * sk.shape[1] for _ in number]
    for g, l in enumerate(ids):
        for s in range(sk.shape[1]):
            c = int(sk[g, s])
            if c >= 0 and (u[l][s] < 0 or c < u[l][s]):
                u[l][s] = c
    return np.array(u, np.int32).reshape(len(number), sk.shape[1]), np.array(ids, np.uint32)


def test_unite_ref_equals_a_plain_loop():
    rng = np.random.default_rng(4)
    sk = rng.integers(0, 1 << 8, (40, 64)).astype(np.int32)
    sk[rng.random(sk.shape) < 0.05] = -1
    sk[np.arange(3, 40, 13), 9] = -1                           # under g % 13: a label without a valid cell in slot 9
    for labels in (rng.integers(0, 6, 40), np.arange(40) % 13, 0xFFFFFFFF - np.arange(40) // 3, np.zeros(40), np.arange(40)):
        u, ids = unite_ref(sk, labels)
        eu, eids = loop_ref(sk, np.asarray(labels).astype(np.uint32))
        assert ids.dtype == np.uint32 and np.array_equal(ids, eids)
        assert u.dtype == np.int32 and np.array_equal(u, eu)
    u, _ = unite_ref(sk, np.arange(40) % 13)
    assert u[3, 9] == -1                                       # label 3 = genomes 3, 16, 29: no valid cell in slot 9


def test_designed_labelings_cover_the_launch_numbers():
    c = launch_constants()
    names = [name for name, _ in designed_labelings(8300)]
    assert len(set(names)) == len(names)
    for t in (c["kUniteLaneMax"], c["kUniteCols"], c["kUniteRows"], c["kUniteCols"] * c["kUniteWaves"]):
        for size in (t - 1, t, t + 1):
            assert "size%d_packed_at2048" % size in names and "size%d_spread_at2048" % size in names
    for name, lab in designed_labelings(8300):
        ids, n_labels = number_labels(lab)
        assert ids.max() == n_labels - 1 and ids[0] == 0, name
        if name.startswith("size"):
            members = np.nonzero(lab == 3)[0]
            assert members[0] < 2048 <= members[-1] and members.size == int(name[4:].split("_")[0]), name
    for n in (1, 7, 64, 65, 2049):
        for name, lab in designed_labelings(n):
            assert lab.shape == (n,) and lab.dtype == np.uint32, name


def test_the_minimum_of_member_sketches_is_the_sketch_of_the_pooled_records(po):
    members, groups = oracle_pan_sketches(po)
    assert members.shape == (sum(PAN_GROUPS), 256) and groups.shape == (len(PAN_GROUPS), 256)
    assert (members >= 0).all()                                # no empty cell: densification plays no part
    labels = np.repeat(np.arange(len(PAN_GROUPS)), PAN_GROUPS)
    u, ids = unite_ref(members, labels)
    assert np.array_equal(ids, labels)
    assert np.array_equal(u, groups)
    assert not np.array_equal(u[1], members[1])                # (the union differs from its first member)
