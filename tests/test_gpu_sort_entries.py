"""GPU: the bucket sort's two partition-entry forms (batch.hip PartEntry) against tests/msm_model.py.

Between k_part_scatter_lds and k_fine_sort_lds an entry is 32 bits, (key & 0xff) << 24 | pt << 1 |
sign, whenever the batch's point references fit 24 bits (2 n <= 2^23), and otherwise the 8-byte
global key and reference. MV_SORT_WIDE = 1 forces the 8-byte form at any size, which is how the form
that batches above 2^22 signatures take stays under test here. Every case runs in both forms
through engine.batch_msm, as test_gpu_batch_msm.py's check does (imported, with that file's cached
rows): every group's every window sum and every flag must equal the model.

What the narrow entry can get wrong, at the smallest shapes that show it: the reference 2 n - 1
with the sign bit set, in the last lane of the last chunk (the entry's 24 low bits); a key whose low
byte is 0 and one whose low byte is 255 (the 8 high bits; a bin read as its neighbour's moves the
point to another bucket); a partition holding a whole chunk's entries (the slot -> partition bytes
of the scatter's store loop, one run as long as the buffer); and the fine sort's direct path, a
partition above FINE_LDS = 16,384 entries. References above 2^13 are beyond a model-checked batch:
the 2^20-signature golden test and config 4's 2^21 blocks run them.
"""
import functools

import pytest

import msm_model as MM
import test_gpu_batch_msm as TM

pytestmark = pytest.mark.gpu

FORMS = pytest.mark.parametrize("wide", [0, 1], ids=["narrow", "wide"])
FINE_LDS = 16384


@FORMS
@pytest.mark.parametrize("n,groups", [(1, 1), (255, 1), (1025, 2), (2049, 2), (4096, 1), (16384, 16)])
def test_random_rows(engine, opts, n, groups, wide):
    opts("MV_SORT_WIDE", wide)
    rows = TM.random_rows(n, groups)
    assert rows.groups == groups
    TM.check(engine, rows, expect=[1] * groups)


@FORMS
@pytest.mark.parametrize("name", ["zk_largest", "z_all_windows_min", "zero_group", "one_scalar_for_all",
                                  "one_scalar_one_point"])
def test_edge_rows(engine, opts, name, wide):
    opts("MV_SORT_WIDE", wide)
    rows = TM.edge_rows(name)
    TM.check(engine, rows, expect=[1] * rows.groups)


@functools.lru_cache(maxsize=None)
def entry_edge_rows():
    """Two full chunks. Rows 0, 1023, 1024 and 2047 (both ends of both chunks) carry chosen digits:
    z with |d| - 1 = 0x0000, 0x0100 (low byte 0) and 0x00ff, 0x01ff (low byte 255) in both signs,
    and z k = ZK_ALL_MIN, every window at -2^15: |d| - 1 = 0x7fff, low byte 255, sign set. The last
    row's A point is reference 2 n - 1."""
    n = 2048
    z, zk = TM.rand_scalars(n, 31)
    dz = [1, -1, 257, -257, 256, -256, 512, 1]
    for i in (0, 1023, 1024, n - 1):
        z[i] = MM.from_digits(dz)
        zk[i] = MM.ZK_ALL_MIN
    dr, da = MM.digits(z[n - 1], zk[n - 1])
    assert dr == dz and da[:15] == [-MM.HALF] * 15
    assert sorted({(abs(d) - 1) & 0xFF for d in dr}) == [0, 255] and (MM.HALF - 1) & 0xFF == 255
    return MM.Rows(z, zk, want=2)


@FORMS
def test_entry_edges(engine, opts, wide):
    opts("MV_SORT_WIDE", wide)
    rows = entry_edge_rows()
    assert rows.groups == 2 and rows.n == 2048
    TM.check(engine, rows, expect=[1, 1])


@functools.lru_cache(maxsize=None)
def direct_path_rows():
    """17 chunks in one group, every row the same scalars and the same two points: each of the 24
    partitions that has entries holds 17,408 of them, more than FINE_LDS."""
    n = 17 * 1024
    z, zk = TM.rand_scalars(1, 7)
    rows = MM.Rows(z * n, zk * n, want=1, a=[3] * n + [5] * n)
    occ = MM.bucket_occupancy(rows.z[:1], rows.zk[:1], rows.group_sigs)
    assert len(occ) == 24 and n > FINE_LDS
    return rows


@FORMS
def test_fine_sort_direct_path(engine, opts, wide):
    opts("MV_SORT_WIDE", wide)
    rows = direct_path_rows()
    assert rows.groups == 1
    TM.check(engine, rows, expect=[1])
