"""CPU: the independent model of the include checks and the threshold clock (tests/quorum_model.py,
written from types.rs:339-375, threshold_clock.rs:12-35, committee.rs:50-57,121-127) against the C
oracle (oracle/block.c) on every generated case: the two were written apart, so a disagreement is a
bug in one of them. test_gpu_quorum.py then holds every device form to the same verdicts."""
import numpy as np
import pytest

import oracle as O
import quorum_model as Q


def test_status_codes_are_the_oracles():
    for k, name in enumerate(Q.NAMES):
        assert getattr(O, "BLOCK_" + name) == k == getattr(Q, name)


@pytest.fixture(scope="module")
def all_cases():
    return {name: Q.quorum_cases(len(stakes), stakes) for name, stakes in Q.COMMITTEES.items()}


@pytest.mark.parametrize("name", list(Q.COMMITTEES))
def test_oracle_gives_the_models_verdict(name, all_cases):
    stakes = Q.COMMITTEES[name]
    n = len(stakes)
    cases = all_cases[name]
    pks = np.frombuffer(b"".join(Q.committee_keys(n)), dtype=np.uint8).reshape(-1, 32)
    st = np.array(stakes, dtype=np.uint64)
    assert [int(x) for x in st] == stakes  # (nothing lost in the uint64 array)
    assert len({c.note for c in cases}) == len(cases)
    for c in cases:
        got = O.block_verify(c.bincode, pks, st, 0)[0]
        assert got == c.status, f"{name}: {c.note}: oracle {Q.NAMES[got]}, model {Q.NAMES[c.status]}"
    # every committee sees both sides of its quorum
    assert {Q.OK, Q.THRESHOLD_CLOCK} <= {c.status for c in cases}, name


def test_the_cases_cover_the_verdicts_and_both_walk_widths(all_cases):
    status = {c.status for cases in all_cases.values() for c in cases}
    assert {Q.OK, Q.THRESHOLD_CLOCK, Q.INCLUDE_ROUND, Q.INCLUDE_UNKNOWN_AUTHORITY, Q.UNKNOWN_AUTHOR,
            Q.SIG_INVALID} <= status
    sizes = {len(s) for s in Q.COMMITTEES.values()}
    assert min(sizes) <= 128 < max(sizes) and {1, 2, 3, 4, 7, 33, 128, 129, 512, 100, 5} <= sizes
    longest = max(len(c.bincode) for cases in all_cases.values() for c in cases)
    assert 700 * 56 < longest < 80 * 1024


def test_model_on_hand_worked_blocks():
    """The model itself, on blocks small enough to work out by hand (stakes 3,1,1,2,1,1,1: total
    10, threshold 6)."""
    s = [3, 1, 1, 2, 1, 1, 1]
    assert Q.quorum_threshold(s) == 6
    assert Q.verdict(0, 5, [(0, 4), (3, 4), (1, 4)], s, True) == Q.THRESHOLD_CLOCK  # 6 is not > 6
    assert Q.verdict(0, 5, [(0, 4), (3, 4), (1, 4), (2, 4)], s, True) == Q.OK
    assert Q.verdict(0, 5, [(0, 4), (0, 4), (0, 4)], s, True) == Q.THRESHOLD_CLOCK  # 3, not 9
    assert Q.verdict(0, 5, [(0, 4), (3, 4), (1, 3), (2, 0)], s, True) == Q.THRESHOLD_CLOCK
    assert Q.verdict(0, 5, [(7, 9), (0, 5)], s, True) == Q.INCLUDE_UNKNOWN_AUTHORITY
    assert Q.verdict(0, 5, [(0, 5), (7, 4)], s, True) == Q.INCLUDE_ROUND
    assert Q.verdict(0, 5, [(0, 5)], s, False) == Q.SIG_INVALID
    assert Q.verdict(7, 5, [], s, False) == Q.UNKNOWN_AUTHOR
    assert Q.verdict(0, 0, [], s, True) == Q.GENESIS
    assert Q.verdict(0, 5, [], s, True, ranges=[(4, 3)]) == Q.VOTE_RANGE
    assert Q.verdict(0, 5, [(0, 5)], s, True, ranges=[(4, 3)]) == Q.INCLUDE_ROUND
    with pytest.raises(OverflowError):
        Q.quorum_threshold([2**63, 2**63])
    with pytest.raises(OverflowError):
        Q.quorum_threshold([2**62] * 4)
    assert Q.quorum_threshold(Q.COMMITTEES["n5_2p60"]) == sum(Q.COMMITTEES["n5_2p60"][k] for k in (0, 2, 4))
