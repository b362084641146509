"""fe_mul's two orders of summation (fe25519.h MulOrder) limb for limb against each other.

The default order (chained: every low column one v_mad_u64_u32 chain that starts from the previous
column's carry) is selftest op 64; the split order (every column summed on its own, then the ripple
with 64-bit adds), which k_bv_bucket_bal's point addition uses, is op 82, and op 83 runs it in
place, the result an operand of the next call (a * b^n). Both orders add the same non-negative
integers, so the contract is equality of all 9 raw limbs, not of the value alone; the value is
checked against Python big integers as well, the raw limbs against the earlier order's model of
test_gpu_fe_carry.py, and the output bound N on every limb.

Inputs are the other field tests' own, imported: test_gpu_fe_carry's edges (every limb at the A and
N maxima, each single limb at either maximum, lazy forms of 0 and p - 1) and its 256 drawn values,
each on the 64 lanes of a wave, and test_gpu_limb_bounds' N x N, A x A, A x N, N x A pairs (edges
of one side against the extremes of the other, and 1200 drawn pairs).
"""
import numpy as np
import pytest

import test_gpu_fe_carry as FC
import test_gpu_limb_bounds as LB

pytestmark = pytest.mark.gpu

P = FC.P
OP_MUL, OP_MUL_SPLIT, OP_MUL_SPLIT_N = 64, 82, 83


def both_orders(engine, items, copies=1):
    """Ops 64 and 82 on the same rows: (chained, split) outputs, one row per item."""
    w = LB.rows(items, 0, copies)
    outs = []
    for op in (OP_MUL, OP_MUL_SPLIT):
        out = engine.selftest(op, w)
        if copies > 1:
            assert (out == np.repeat(out[::copies], copies, axis=0)).all(), "the lanes of one wave disagree"
            out = out[::copies]
        outs.append(out)
    return outs


def assert_same_and_right(items, chained, split):
    assert (split[:, :9] == chained[:, :9]).all(), "raw limbs differ between the two orders"
    assert (split[:, 40:48] == chained[:, 40:48]).all()
    for (a, b), o in zip(items, split):
        limbs = [int(x) for x in o[:9]]
        v = FC.value(a) * FC.value(b) % P
        assert FC.value(limbs) % P == v, (a, b)
        assert LB.words_value(o[40:48]) == v, (a, b)
        assert max(limbs) <= FC.N_MAX, (a, b, limbs)


@pytest.mark.parametrize("which", ["edge", "drawn"])
def test_split_order_limbs_carry_inputs(engine, which):
    items = FC.pairs(which)
    chained, split = both_orders(engine, items, 64 if which == "drawn" else 1)
    assert_same_and_right(items, chained, split)
    for (a, b), o, m in zip(items, split, FC.expected(OP_MUL, which)):  # the earlier order's model
        assert [int(x) for x in o[:9]] == m, (a, b)


def test_split_order_limbs_lazy_operands(engine):
    items = LB.mixed_pairs()
    chained, split = both_orders(engine, items)
    assert_same_and_right(items, chained, split)


@pytest.mark.parametrize("n", [1, 3, 20])
def test_split_order_in_place(engine, n):
    """r = a, then n times fe_mul<split>(r, r, b): the limbs of op 64 applied n times from the host,
    and the value a b^n."""
    items = FC.pairs("edge") + FC.pairs("drawn")
    out = engine.selftest(OP_MUL_SPLIT_N, LB.rows(items, n))
    step = [(a, b) for a, b in items]
    for _ in range(n):
        ref = engine.selftest(OP_MUL, LB.rows(step))
        step = [([int(x) for x in r[:9]], b) for r, (_, b) in zip(ref, items)]
    assert (out[:, :9] == ref[:, :9]).all(), "raw limbs differ between the two orders"
    for (a, b), o in zip(items, out):
        v = FC.value(a) * pow(FC.value(b), n, P) % P
        assert FC.value([int(x) for x in o[:9]]) % P == v and LB.words_value(o[40:48]) == v, (n, a, b)
