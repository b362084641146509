"""CPU: the two restatements in tests/index_model.py held to each other. Reference keeps
BlockManager's own structures (blocks_pending, block_references_waiting, missing, the unlock
cascade of add_blocks, block_manager.rs:19-145) under process_blocks' skip and early return
(net_sync.rs:314-386); TwoState keeps one state per reference, as include/mysti_verify.h states
mv_accept_blocks. That the two states suffice is checked here, not assumed: after every call of 100
seeded deliveries of a 12-round DAG (random order and chunking, duplicates, withheld blocks, a bad
signature now and then) the missing references returned, the `processed` answers and
missing_blocks() are equal. Verdicts are the CPU oracle's."""
import hashlib
import random

import numpy as np
import pytest

import blocks as B
import index_model as IM
import oracle as O
import replay_model as RM

N_AUTH, ROUNDS = 4, 12


def bad_signature(block: bytes) -> bytes:
    """One bit of s flipped and the digest recomputed: parses, digest matches, signature invalid."""
    sig = bytearray(block[-64:])
    sig[40] ^= 0x10
    dig = hashlib.blake2b(O.block_preimage(block) + bytes(sig), digest_size=32).digest()
    return block[:24] + dig + block[56:-64] + bytes(sig)


@pytest.fixture(scope="module")
def dag():
    """48 signed config-1 blocks (4 authorities x 12 rounds, every block includes the four of the
    round before), the genesis references and the oracle's verdict function."""
    bins = [b.bincode() for b in B.gen_config1(O.sign, rounds=ROUNDS, n_auth=N_AUTH)]
    genesis = [(a, 0, B.genesis(a).digest) for a in range(N_AUTH)]
    pk = np.frombuffer(O.public_key(B.ZERO_SEED) * N_AUTH, dtype=np.uint8).reshape(N_AUTH, 32)
    verdicts = RM.oracle_verdicts(pk, np.ones(N_AUTH, dtype=np.uint64), 0)
    assert IM.run_verdicts(verdicts, bins) == [0] * len(bins)
    return bins, genesis, verdicts


def both(dag):
    bins, genesis, verdicts = dag
    return IM.Reference(N_AUTH, verdicts, genesis), IM.TwoState(verdicts, genesis)


def step(ref, two, blocks, groups, what):
    processed, missing = ref.accept(blocks, groups)
    got = two.accept(blocks, groups)
    assert [s == IM.KNOWN for s in got.blk_state] == processed, what
    assert len(set(got.missing)) == len(got.missing) and set(got.missing) == missing, what
    assert two.missing_blocks(N_AUTH) == ref.missing_blocks(), what
    have = {r for r, s in two.state.items() if s == IM.HAVE}
    assert have == ref.store | set(ref.blocks_pending), what
    return got


@pytest.mark.parametrize("seed", range(100))
def test_random_deliveries(dag, seed):
    bins = dag[0]
    rng = random.Random(seed)
    ref, two = both(dag)
    order = list(range(len(bins)))
    rng.shuffle(order)
    order = [i for i in order if rng.random() > 0.1]  # withheld blocks
    order += rng.sample(order, k=len(order) // 5)  # duplicates, later
    rng.shuffle(order)
    bad = bad_signature(bins[rng.randrange(len(bins))])
    p, call = 0, 0
    while p < len(order):
        m = rng.randint(1, 9)
        blocks = [bins[i] for i in order[p:p + m]]
        if rng.random() < 0.15:
            blocks.insert(rng.randrange(len(blocks) + 1), bad)
        if rng.random() < 0.2:
            blocks.append(blocks[0])  # a duplicate inside the call
        kind = rng.randrange(3)
        groups = None if kind == 0 else [0] * len(blocks) if kind == 1 else sorted(rng.randrange(3) for _ in blocks)
        step(ref, two, blocks, groups, (seed, call))
        p, call = p + m, call + 1
    # everything withheld is delivered in the end: nothing stays wanted, everything is stored
    step(ref, two, bins, [0] * len(bins), (seed, "rest"))
    assert two.wanted() == set() and not ref.blocks_pending and len(ref.store) == len(bins) + N_AUTH


def test_state_transitions(dag):
    bins, genesis, verdicts = dag
    two = IM.TwoState(verdicts)
    r1, r2 = IM.own_ref(bins[0]), IM.own_ref(bins[1])
    assert two.insert([r1, r1, r2], IM.WANTED) == [IM.ABSENT] * 3  # duplicates report the state before the call
    assert two.insert([r1], IM.HAVE) == [IM.WANTED] and two.lookup(r1) == IM.HAVE  # WANTED -> HAVE
    assert two.insert([r1], IM.WANTED) == [IM.HAVE] and two.lookup(r1) == IM.HAVE  # nothing is lowered
    assert two.insert([genesis[0]], IM.HAVE) == [IM.ABSENT]  # absent -> HAVE
    assert two.counts() == (2, 1) and two.wanted() == {r2}


def test_round_two_before_round_one(dag):
    bins = dag[0]
    ref, two = both(dag)
    got = step(ref, two, bins[4:8], [7] * 4, "round 2")
    assert got.blk_state == [IM.NEW] * 4 and got.missing == IM.includes(bins[4])  # the four of round 1, once each
    got = step(ref, two, bins[4:8] + bins[0:2], None, "round 2 again, half of round 1")
    assert got.blk_state == [IM.KNOWN] * 4 + [IM.NEW] * 2 and got.missing == []
    assert two.wanted() == {IM.own_ref(bins[2]), IM.own_ref(bins[3])}
    got = step(ref, two, bins[2:4], None, "the rest of round 1")
    assert two.wanted() == set() and len(ref.store) == 8 + N_AUTH  # the cascade stored round 2


def test_dropped_group_and_duplicates(dag):
    bins = dag[0]
    ref, two = both(dag)
    blocks = [bins[0], bad_signature(bins[1]), bins[2], bins[0], bins[0]]
    got = step(ref, two, blocks, [1, 1, 1, 2, 3], "first group rejected")
    assert got.blk_state == [IM.DROPPED, IM.REJECTED, IM.DROPPED, IM.NEW, IM.DUP]
    assert two.lookup(IM.own_ref(bins[2])) == IM.ABSENT and got.missing == []
    got = step(ref, two, [bins[0], bins[1], bins[1]], None, "again")
    assert got.blk_state == [IM.KNOWN, IM.NEW, IM.DUP]


def test_tampered_known_block(dag):
    """The reference skips on the claimed reference alone (net_sync.rs:333-336): a known block
    whose body was tampered with is not verified and does not reject its message."""
    bins = dag[0]
    ref, two = both(dag)
    step(ref, two, bins[0:1], None, "first")
    tampered = bins[0][:100] + bytes([bins[0][100] ^ 0xFF]) + bins[0][101:]
    assert IM.run_verdicts(dag[2], [tampered]) != [0]
    got = step(ref, two, [bins[1], tampered, bins[2]], [5, 5, 5], "tampered")
    assert got.blk_state == [IM.NEW, IM.KNOWN, IM.NEW] and got.blk_status == [0, 0, 0]


def test_short_and_malformed_references(dag):
    bins, _, verdicts = dag
    two = IM.TwoState(verdicts, [IM.own_ref(bins[0])])
    len31 = bins[0][:16] + (31).to_bytes(8, "little") + bins[0][24:]
    # under 56 bytes, or a length word that is not 32, no reference is read: not KNOWN although the
    # bytes are a known block's; at 56 bytes a reference that is not in the index is read
    cases = [b"", bins[0][:1], bins[0][:55], bins[1][:56], len31]
    got = two.accept(cases)
    assert got.blk_state == [IM.REJECTED] * 5 and got.blk_status == [IM.BLOCK_PARSE_ERROR] * 5
    # the probe goes by the claimed reference alone: 56 bytes of a known block are KNOWN
    assert two.accept([bins[0][:56]]).blk_state == [IM.KNOWN]


def test_ref_table_probe_lengths():
    t = IM.RefTable(16)
    keys = [bytes([k]) * 48 for k in range(8)]
    probes = [t.insert(k) for k in keys]
    assert len(t.tab) == 8 and t.longest == max(probes) >= 1
    assert [t.insert(k) for k in keys] == probes  # found where they were put
