"""GPU: the radix-256 comb tables themselves (k_comb_init, csrc/comb.h), read back entry by entry
(Engine.comb_table, mv_selftest_comb_table: a plain copy) and compared bit for bit with the
big-integer model of tests/comb_model.py: C[i][j] = [j 256^i]P for the base point and
[j 256^i](-A) for committee keys, as canonical (y+x, y-x, 2dxy) in 29-bit limbs and five zero words.

The verdict tests reach a table only through the entries their inputs' digits happen to pick; here
all 32 x 129 entries of each table are held, entries 17..128 of row 31 included (which no scalar below
l reaches), for ordinary keys, +-B, every encoding of every small-order point (whose rows 1.. are
the identity after up to 248 doublings of exceptional points) and for the first, last and
neighbouring tables of a 512-key committee (each key's table at its own place, none overwritten)."""
import numpy as np
import pytest

import comb_model as CM
import zip215 as Z
from test_gpu_batch_msm import committee as msm_committee

pytestmark = pytest.mark.gpu


def assert_table(got, want, what):
    assert got.shape == want.shape == (32, 129, 32) and got.dtype == np.uint32
    if (got == want).all():
        return
    bad = np.argwhere((got != want).any(axis=2))
    i, j = (int(v) for v in bad[0])
    raise AssertionError(f"{what}: {len(bad)} of 4128 entries differ, first at row {i}, entry {j}: "
                         f"got {CM.entry_values(got[i, j])} tail {got[i, j, 27:].tolist()}, "
                         f"want {CM.entry_values(want[i, j])}")


def undecodable():
    y = 2
    while Z.decompress(y.to_bytes(32, "little")) is not None:
        y += 1
    return y.to_bytes(32, "little")


def test_base_point_table(engine):
    assert_table(engine.comb_table(), CM.table(Z.B_POINT), "B table")


def test_key_outside_the_committee_is_refused(engine):
    import mysticeti_amd as M

    engine.set_committee(np.tile(np.frombuffer(Z.compress(Z.B_POINT), np.uint8), (2, 1)), np.ones(2, np.uint64))
    engine.comb_table(1)
    with pytest.raises(M.MvError):
        engine.comb_table(2)


def test_edge_keys(engine):
    """A random key, B, -B, every small-order point in every encoding ZIP-215 decodes (canonical,
    y >= p, x = 0 with the sign bit set) and one key that does not decode."""
    rng = np.random.default_rng(5)
    rand = Z.public_key(rng.integers(0, 256, size=32, dtype=np.uint8).tobytes())
    small = Z.small_order_encodings()
    assert len({e for e, _ in small}) == len(small) >= 12 and any(not c for _, c in small)
    assert any(int.from_bytes(e, "little") & (2**255 - 1) >= Z.P for e, _ in small)  # a y >= p form
    keys = [rand, Z.compress(Z.B_POINT), Z.compress(Z.neg(Z.B_POINT))] + [e for e, _ in small]
    bad = len(keys)
    keys.append(undecodable())
    assert len(keys) <= 32
    pks = np.frombuffer(b"".join(keys), dtype=np.uint8).reshape(-1, 32)
    ok = engine.set_committee(pks, np.ones(len(keys), np.uint64))
    assert [int(x) for x in ok] == [1] * bad + [0]
    for b in range(bad):
        assert_table(engine.comb_table(b), CM.table(Z.decompress(keys[b]), negate=True), f"key {b} ({keys[b].hex()})")
    assert_table(engine.comb_table(), CM.table(Z.B_POINT), "B table after set_committee")
    # the table of a key that does not decode is unspecified: only its key_ok and the verdicts
    # under it (MalformedPublicKey whatever the signature) are held
    it = CM.b_cover()[:5]
    st = engine.ed25519_verify(np.array([np.frombuffer(x.msg, np.uint8) for x in it]),
                               np.array([np.frombuffer(x.sig, np.uint8) for x in it]),
                               key_idx=np.full(len(it), bad, np.uint32))
    assert (st == 2).all()


@pytest.fixture(scope="module")
def big(engine):
    keys, mult = msm_committee(512)
    ok = engine.set_committee(keys, np.ones(512, np.uint64))
    assert ok.all()
    return keys, mult


@pytest.mark.parametrize("key", [0, 1, 255, 510, 511])
def test_512_key_committee_places_every_table(engine, big, key):
    keys, mult = big
    A = Z.decompress(keys[key].tobytes())
    assert Z.point_eq(A, Z.scalarmult(Z.B_POINT, mult[key]))
    assert_table(engine.comb_table(key), CM.table(A, negate=True), f"key {key} of 512")


def test_base_point_table_after_the_512_key_committee(engine, big):
    assert_table(engine.comb_table(), CM.table(Z.B_POINT), "B table after a 512-key set_committee")
