"""The two statements of the vote-aggregation rule (votes_model.py) agree: the reference restated
as written (range map, splits, removal of emptied entries) and the per-cell rule that
mv_aggregate_votes is held to."""
import pytest

import votes_cases as vc
from votes_model import CellRule, VerbatimAggregator, shared_ranges


def run_both(stakes, calls):
    ref, cell = VerbatimAggregator(stakes), CellRule(stakes)
    for blocks, register_only in calls:
        for b in blocks:
            a, c = ref.process_block(b, register_only), cell.process_block(b, register_only)
            assert a.processed == c.processed
            assert (a.unknown, a.duplicate, a.flags) == (c.unknown, c.duplicate, c.flags)
            assert ref.len() == cell.len()
    return ref, cell


@pytest.mark.parametrize("n_auth", [4, 7])
def test_models_agree_on_random_sequences(n_auth):
    stakes = vc.unequal_stakes(n_auth)
    certified = 0
    for seed in range(1500):
        _, cell = run_both(stakes, [(vc.random_blocks(1000 * n_auth + seed, n_auth, 30), False)])
        certified += cell.certified
    assert certified > 0  # (a check of the generator: some sequences reach the threshold)


@pytest.mark.parametrize("name", sorted(vc.named_cases()))
def test_models_agree_on_named_cases(name):
    stakes, calls = vc.named_cases()[name]
    run_both(stakes, calls)


def test_removed_block_and_empty_cells_are_one_state():
    """Once every cell of a sharing block is certified the reference drops the block from `pending`;
    the cell rule just leaves its cells empty. Votes, a second registration and len() cannot tell."""
    stakes = [1, 1, 1, 1]
    b = vc.block(0, 1, vc.shares(2))
    voters = [vc.block(a, 2, [("range", b[1], 0, 2)]) for a in (1, 2)]
    ref, cell = run_both(stakes, [([b] + voters, False)])
    assert ref.len() == 0 and b[1] not in ref.pending
    assert cell.cells[b[1]] == {} and cell.len() == 0
    late = vc.block(3, 3, [("range", b[1], 0, 2)])
    assert ref.process_block(late) == cell.process_block(late)
    assert ref.process_block(late).unknown == 2
    assert ref.process_block(b) == cell.process_block(b)  # registers afresh in both
    assert ref.len() == cell.len() == 1


def test_share_runs():
    b = vc.block(0, 1, [("share", b"a"), ("vote", vc.ref_of(1, 1), 0), ("share", b"b"), ("share", b"c")])
    assert shared_ranges(b[2]) == [(0, 1), (2, 4)]
