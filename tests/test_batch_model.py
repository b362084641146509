"""CPU: the batch preparation model (tests/batch_model.py) against oracle/zip215.py's arithmetic
alone, on four signed messages: the combined equation holds for valid signatures and fails for a
changed one, and a pair of signatures whose errors cancel passes it with equal coefficients but
not with the model's own -- the failure the GPU tests of the coefficients are there to exclude."""
import hashlib

import pytest

import batch_model as BM
import zip215 as Z

SECRET = hashlib.sha256(b"batch model secret").digest()


@pytest.fixture(scope="module")
def rows():
    seeds = [hashlib.sha256(b"seed %d" % i).digest() for i in range(4)]
    msg = [hashlib.sha256(b"msg %d" % i).digest() for i in range(4)]
    pk = [Z.public_key(s) for s in seeds]
    sig = [Z.sign(s, m) for s, m in zip(seeds, msg)]
    assert all(Z.verify(a, sg, m) for a, sg, m in zip(pk, sig, msg))
    return msg, sig, pk


def test_coefficients_are_the_keyed_hash():
    z = [BM.coefficient(SECRET, 7, i) for i in range(4)]
    assert len(set(z)) == 4 and all(0 < x < 1 << 127 for x in z)
    h = hashlib.blake2b(SECRET + (7).to_bytes(8, "little") + (2).to_bytes(8, "little"), digest_size=32).digest()
    assert z[2] == int.from_bytes(h[:16], "little") % (1 << 127)
    assert BM.coefficient(SECRET, 8, 2) != z[2]


def test_geometry_matches_whole_chunk_groups():
    assert BM.group_geometry(1, 8) == (1, 1024)
    assert BM.group_geometry(4113, 3) == (3, 2048)  # 5 chunks in groups of 2: 2 + 2 + 1
    assert BM.group_geometry(4113, 8) == (5, 1024)
    assert BM.group_geometry(16384 + 100, 8) == (6, 3072)
    assert BM.group_geometry(9000, 16) == (9, 1024)
    assert BM.group_geometry(1 << 20, 99) == (16, 65536)


def test_equation_holds_for_valid_signatures(rows):
    msg, sig, pk = rows
    p = BM.prep(msg, sig, pk, SECRET, 1)
    assert [l.status for l in p.lanes] == [0] * 4
    assert all(l.zk == l.z * l.k % Z.L for l in p.lanes)
    assert p.sums[0] == sum(l.z * l.s for l in p.lanes)
    assert BM.equation_holds(p)


def test_equation_fails_for_one_changed_s(rows):
    msg, sig, pk = rows
    s2 = list(sig)
    s2[2] = sig[2][:32] + ((int.from_bytes(sig[2][32:], "little") + 1) % Z.L).to_bytes(32, "little")
    assert not Z.verify(pk[2], s2[2], msg[2])
    assert not BM.equation_holds(BM.prep(msg, s2, pk, SECRET, 1))


def test_prerejected_lanes_are_left_out(rows):
    msg, sig, pk = rows
    s2 = list(sig)
    s2[1] = sig[1][:32] + Z.L.to_bytes(32, "little")  # s = l
    bad_y = next(y for y in range(2, 50) if Z.decompress(y.to_bytes(32, "little")) is None).to_bytes(32, "little")
    s2[3] = bad_y + sig[3][32:]
    pk2 = list(pk)
    pk2[0] = bad_y
    p = BM.prep(msg, s2, pk2, SECRET, 1)
    assert [l.status for l in p.lanes] == [2, 1, 0, 1]
    assert all(l.z == 0 and l.zk == 0 for l in p.lanes if l.status)
    assert p.sums[0] == p.lanes[2].z * p.lanes[2].s
    assert BM.equation_holds(p)


@pytest.mark.parametrize("delta", [1, 1 << 125, Z.L - 1])
def test_cancelling_pair_needs_distinct_coefficients(rows, delta):
    msg, sig, pk = rows
    s2 = BM.cancelling_pair(sig, 1, 3, delta)
    assert not Z.verify(pk[1], s2[1], msg[1]) and not Z.verify(pk[3], s2[3], msg[3])
    z_eq = BM.coefficient(SECRET, 1, 0)
    assert BM.equation_holds(BM.prep(msg, s2, pk, SECRET, 1, z=[z_eq] * 4))  # equal z: the forgery passes
    assert not BM.equation_holds(BM.prep(msg, s2, pk, SECRET, 1))           # the model's z: it does not
