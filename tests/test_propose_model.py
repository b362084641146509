"""CPU: tests/propose_model.py. Core is the reference's text (threshold_clock.rs:58-89, core.rs:181-278);
the reference's own test sequence pins its clock, and BatchRule -- the segment form propose.hip
runs -- is held to Core on seeded sequences. The library exports the mv_propose_* symbols."""
import os
import random
import re
import subprocess

import pytest

import propose_model as PM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "mysticeti_amd", "libmysti_verify.so")
SYMBOLS = ["mv_propose_reserve", "mv_propose_add", "mv_dev_propose_add", "mv_propose_take", "mv_propose_own",
           "mv_propose_stats"]


def test_reference_sequence():
    """threshold_clock.rs:136-153, test_threshold_clock_aggregator: BlockReference::new_test(authority, round)."""
    c = PM.Core([1, 1, 1, 1], 0)
    b = PM.BatchRule([1, 1, 1, 1])
    rounds, batch = [], []
    for ref in [(0, 0), (0, 1), (1, 0), (1, 1), (2, 1), (3, 1)]:
        c.add_block(ref)
        rounds.append(c.round)
        batch.append(b.add([ref], in_order=True)[0])
    assert rounds == [0, 1, 1, 1, 2, 2]
    assert batch == rounds
    one = PM.BatchRule([1, 1, 1, 1])
    assert one.add([(0, 0), (0, 1), (1, 0), (1, 1), (2, 1), (3, 1)], in_order=True)[0] == 2


def test_greater_ignores_the_quorum():
    """Stakes [7, 1, 1, 1]: quorum_threshold 6, so seat 0 alone is a quorum -- which Greater does not ask for."""
    for nxt in ((0, 3, "x"), (1, 3, "y")):  # the same row again, or another seat's: Equal, and add answers true
        c = PM.Core([7, 1, 1, 1], 0)
        b = PM.BatchRule([7, 1, 1, 1])
        assert c.add_blocks([(0, 3, "x")])[0] == 3 and b.add([(0, 3, "x")])[0] == 3
        assert c.add_blocks([nxt])[0] == 4 and b.add([nxt])[0] == 4


def test_sorted_and_in_order_differ():
    rows = [(0, 2, "A2"), (1, 1, "B1"), (0, 1, "A1")]
    for in_order, want in ((False, 3), (True, 2)):
        c, b = PM.Core([7, 1, 1, 1], 0), PM.BatchRule([7, 1, 1, 1])
        c.round = b.round = 1
        assert c.add_blocks(rows, in_order=in_order)[0] == want
        assert b.add(rows, in_order=in_order)[0] == want
        assert [w for _, (_, w) in c.pending] == (rows if in_order else [rows[1], rows[2], rows[0]])
        assert b.pending == c.pending


def sequence(seed):
    """One seeded run: a committee, then calls whose rows lie below, at and above the clock."""
    rng = random.Random(seed)
    n = rng.choice([3, 4, 5, 33, 512])
    kind = rng.randrange(4)
    if kind == 0:
        stakes = [1] * n
    elif kind == 1:
        stakes = [rng.randrange(1, 10) for _ in range(n)]
    elif kind == 2:
        stakes = [1 << 40] * n
    else:
        stakes = [1] * n
        stakes[rng.randrange(n)] = 2 * n  # one seat is a quorum alone
    c, b = PM.Core(stakes, 0), PM.BatchRule(stakes)
    serial = 0
    for _ in range(rng.randrange(3, 9)):
        rows = []
        base = c.round
        for _ in range(rng.randrange(0, 3 * min(n, 40))):
            rnd = max(0, base + rng.choice([-2, -1, 0, 0, 0, 0, 1, 1, 2, 5]))
            serial += 1
            # an equivocation is a second reference of one (authority, round)
            rows.append((rng.randrange(n), rnd, serial if rng.random() < 0.9 else serial - 1))
        in_order = rng.random() < 0.3
        payload = rng.randrange(1 << 60) if rng.random() < 0.5 else None
        positions = [rng.randrange(1 << 50) for _ in rows]
        yield c, b, rows, positions, in_order, payload


@pytest.mark.parametrize("chunk", range(8))
def test_batch_rule_is_the_automaton(chunk):
    """400 seeded sequences: after every call the clock (round, stake, voters) and the queue are equal."""
    for seed in range(50 * chunk, 50 * chunk + 50):
        for c, b, rows, positions, in_order, payload in sequence(seed):
            want = c.add_blocks(rows, positions, in_order, payload)
            got = b.add(rows, positions, in_order, payload)
            assert got == want, (seed, rows)
            assert b.votes == c.votes and b.pending == c.pending, seed


def test_take_compresses_and_cuts():
    c = PM.Core([1, 1, 1, 1], 0)
    g = [(a, 0, "g") for a in range(4)]
    c.add_blocks(g[1:], in_order=True)
    c.own_block(g[0], [])
    assert c.round == 1
    r1 = [(a, 1, "r1") for a in range(1, 4)]
    for r in r1:
        c.blocks[r] = list(g)
    c.add_blocks(r1[:1], positions=[11])
    rnd, inc, pay, taken, flags, nxt = c.try_new_block()
    # the genesis entries are taken with the clock at 1; the round-1 entry stays; genesis has no record
    assert (rnd, inc, pay, taken, flags, nxt) == (1, g[1:], [], 3, 0, 11)
    own1 = (0, 1, "own")
    c.own_block(own1)
    assert c.own == (own1, [g[0]] + g[1:]) and c.round == 1
    assert c.try_new_block() is None  # the clock is at 1, and so is the own last block
    c.add_blocks(r1[1:], positions=[12, 13], payload=77)
    assert c.round == 2
    rnd, inc, pay, taken, flags, nxt = c.try_new_block()
    assert (rnd, inc, pay, taken, flags, nxt) == (2, r1, [77], 4, 0, PM.NO_ENTRY)
    # a pending block that another taken block names is dropped
    c.own_block((0, 2, "own"))
    r2 = (1, 2, "r2")
    c.blocks[r2] = [r1[0], (2, 1, "late")]
    c.add_blocks([(2, 1, "late"), r2, (3, 2, "r2"), (2, 2, "r2")])
    assert c.round == 3
    assert c.try_new_block()[1] == [r2, (3, 2, "r2"), (2, 2, "r2")] and c.dropped == 1


def test_library_exports_the_propose_symbols():
    if not os.path.exists(LIB):
        from mysticeti_amd.build import build

        build()
    import mysticeti_amd as M

    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (mv_[a-z0-9_]+)", out))
    assert [s for s in SYMBOLS if s not in exported] == []
    assert [s for s in SYMBOLS if s not in M.EXPORTS] == []
    lib = M.load_library()
    assert all(hasattr(lib, s) for s in SYMBOLS)
