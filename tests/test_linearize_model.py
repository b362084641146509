"""CPU: tests/linearize_model.py's LevelRule -- the rule mv_linearize states and the engine is held to --
against Verbatim, collect_sub_dag as the reference writes it (consensus/linearizer.rs:125-166): the
block order of every sub-DAG and the committed set after every commit, on seeded DAGs with omitted
authors, equivocation, weak links to any lower round, duplicate and shuffled includes, a random
pre-committed set and several leaders in sequence; then the divergences and the status rows."""
import random

import pytest

import linearize_model as L

SEEDS = range(400)


def dag_of(seed):
    rng = random.Random(seed)
    blocks, by_round = L.random_dag(rng, rng.randint(1, 10), rng.randint(2, 14))
    return rng, blocks, by_round


def split(blocks):
    """The engine's view: genesis has an index entry and no record."""
    return {b: incs for b, incs in blocks.items() if b[1] > 0}


@pytest.mark.parametrize("chunk", range(8))
def test_level_rule_is_the_stack_order(chunk):
    commits = 0
    for seed in SEEDS[chunk::8]:
        rng, blocks, by_round = dag_of(seed)
        pre = {b for b in blocks if rng.random() < 0.1} if seed % 3 == 0 else set()
        v, m = L.Verbatim(blocks), L.LevelRule(split(blocks), pre)
        v.committed = set(pre)
        for leader in L.leader_sequence(rng, by_round):
            status, _ = m.sub_dag(leader)
            if status == L.COMMITTED:
                with pytest.raises(AssertionError):
                    v.collect_sub_dag(leader)
                continue
            assert status == L.OK, (seed, leader)  # (the generator makes no INCOMPLETE or OVERFLOW row)
            got, sub = m.linearize([leader])
            (want, height), = v.handle_commit([leader])
            assert got == want and sub == [[L.OK, 0, len(want), height]], (seed, leader)
            assert m.marked == v.committed and m.last_height == v.last_height, (seed, leader)
            commits += 1
    assert commits > 100


def test_a_sequence_in_one_call_is_the_calls_one_by_one():
    for seed in SEEDS[:60]:
        rng, blocks, by_round = dag_of(seed)
        leaders = L.leader_sequence(rng, by_round)
        one, many = L.LevelRule(split(blocks)), L.LevelRule(split(blocks))
        blocks_1, sub_1 = one.linearize(leaders)
        at, stopped = 0, False
        for k, leader in enumerate(leaders):
            if stopped:
                assert sub_1[k] == [L.STOPPED, at, 0, 0]
                continue
            b, (row,) = many.linearize([leader])
            assert sub_1[k] == [row[0], at, row[2], row[3]] and blocks_1[at:at + row[2]] == b
            at += row[2]
            stopped = row[0] != L.OK
        assert one.marked == many.marked and one.last_height == many.last_height


def test_leader_already_committed():
    _, blocks, by_round = dag_of(5)
    top, low = by_round[-1][0], by_round[-2][0]
    m = L.LevelRule(split(blocks))
    got, sub = m.linearize([top, low, by_round[-1][-1]])
    assert low in got and sub[1] == [L.COMMITTED, len(got), 0, 0] and sub[2] == [L.STOPPED, len(got), 0, 0]
    assert m.last_height == 1 and m.marked == set(got)
    assert m.linearize([top])[1] == [[L.COMMITTED, 0, 0, 0]]


def test_missing_record_above_round_0_and_genesis_leaves():
    _, blocks, by_round = dag_of(7)
    leader = by_round[-1][0]
    whole, _ = L.LevelRule(split(blocks)).linearize([leader])
    assert any(b[1] == 0 for b in whole)  # genesis: leaves, put out and marked
    gone = next(b for b in whole if 0 < b[1] < leader[1])
    records = split(blocks)
    del records[gone]
    m = L.LevelRule(records)
    assert m.linearize([leader]) == ([], [[L.INCOMPLETE, 0, 0, 0]]) and not m.marked and m.last_height == 0
    m.mark([gone], 0)  # a marked reference is passed over with or without a record
    got, sub = m.linearize([leader])
    assert sub[0][0] == L.OK and gone not in got
    assert L.LevelRule({}).linearize([leader])[1] == [[L.INCOMPLETE, 0, 0, 0]]


def test_path_depth_at_and_past_the_key():
    blocks, leader = L.chain(L.MAX_DEPTH)
    got, sub = L.LevelRule(split(blocks)).linearize([leader])
    assert sub == [[L.OK, 0, L.MAX_DEPTH + 1, 1]] and got == sorted(blocks, key=lambda b: b[1])
    blocks, leader = L.chain(L.MAX_DEPTH + 1)
    m = L.LevelRule(split(blocks))
    assert m.linearize([leader, (0, 1, 0)]) == ([], [[L.OVERFLOW, 0, 0, 0], [L.STOPPED, 0, 0, 0]]) and not m.marked
    v = L.Verbatim(blocks)
    assert len(v.collect_sub_dag(leader)[0]) == L.MAX_DEPTH + 2  # (the reference has no such limit)


def test_include_number_past_the_component():
    wide = [(1, 0, k) for k in range(L.MAX_INCLUDE + 2)]
    records = {(0, 1, 0): wide}
    assert L.LevelRule(records).linearize([(0, 1, 0)])[1] == [[L.OVERFLOW, 0, 0, 0]]
    records = {(0, 1, 0): wide[:-1]}
    got, sub = L.LevelRule(records).linearize([(0, 1, 0)])
    assert sub[0][:3] == [L.OK, 0, L.MAX_INCLUDE + 2] and got[0] == wide[-2]  # the last pushed is popped first


def test_cap():
    _, blocks, by_round = dag_of(9)
    leaders = [by_round[-2][0], by_round[-1][0]]
    whole, sub = L.LevelRule(split(blocks)).linearize(leaders)
    assert [r[0] for r in sub] == [L.OK, L.OK]
    m = L.LevelRule(split(blocks))
    got, rows = m.linearize(leaders, cap=len(whole) - 1)
    assert rows == [sub[0], [L.OVERFLOW, sub[0][2], 0, 0]] and got == whole[:sub[0][2]] and m.last_height == 1
