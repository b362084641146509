"""Helper (not a test): small DAGs over wide committees, for tests/test_wide_committee_model.py (which
holds every case to the oracle and the models to each other) and tests/test_gpu_wide_committee.py
(which holds the library to the models on them).

The decision kernels keep blame, vote and certificate bitmaps of 16 words (512 seats), bitmap_stake
makes eight passes of 64 seats, and the replay summary fills seen[512] in two strides. A 512-seat DAG
with equal stakes needs blocks of 342 includes, so the stakes here are skewed: thirteen heavy seats
carry a quorum between them, and every other seat has stake 1. A committee of n seats with 13 heavy
ones of stake H has quorum_thr = 2 * (13 H + n - 13) / 3 (mv_set_committee's formula); plan() picks
the H at which m = 11 heavy seats and k light ones (2 <= k <= 4) sum to exactly quorum_thr + 1:

  512 seats: H = 142, total 2,345, quorum_thr 1,563; 11 heavy + 2 light = 1,564, 11 heavy + 1 light =
  1,563, 12 heavy = 1,704: a valid block needs 12 includes (or 13: 11 heavy and 2 light).

The heavy seats of the 512-seat cases sit at the bitmap-word and pass edges. Only the seats a case
needs produce blocks. Blocks are built and signed through test_gpu_decide.Dag with whatever signs
(the engine on the GPU, OracleSigner here)."""
import functools
import itertools

import numpy as np

import commit_seq_model as S
import oracle as O
from test_gpu_decide import Dag

N = 512
HEAVY = (0, 31, 32, 63, 64, 127, 128, 255, 256, 479, 480, 510, 511)
LIGHT_W4, LIGHT_W15, LIGHT_MID = 130, 500, 300  # a light seat of word 4, of word 15, and one more
TOP_SEATS = (33, 65, 129, 257, 511, 512)
MAX_INCLUDES = 16


def quorum_threshold(stakes):
    return 2 * sum(stakes) // 3  # mv_set_committee; a quorum is a stake above it


class Plan:
    """n seats, the heavy ones with stake H: m heavy and k light seats sum to quorum_thr + 1."""

    def __init__(self, n, heavy, H, m, k):
        self.n, self.heavy, self.H, self.m, self.k = n, tuple(heavy), H, m, k
        self.stakes = [H if a in heavy else 1 for a in range(n)]
        self.thr = quorum_threshold(self.stakes)

    def lights(self, first=()):
        """k light seats, `first` among them, the rest the lowest light seats."""
        out = list(first)
        out += [a for a in range(self.n) if a not in self.heavy and a not in out][:self.k - len(out)]
        return out

    def stake(self, seats):
        return sum(self.stakes[a] for a in set(seats))


@functools.lru_cache(maxsize=None)
def plan(n, heavy):
    m = len(heavy) - 2  # a block that leaves one heavy seat out still has m + 1 of them
    for k in (2, 3, 4):  # the fewest light seats first
        for H in range(5, 4 * n):
            if m * H + k == 2 * (len(heavy) * H + n - len(heavy)) // 3 + 1:
                return Plan(n, heavy, H, m, k)
    raise ValueError(n)


def top_heavy(n):
    """Thirteen heavy seats below the top seat n - 1, at the word edges where the committee has them."""
    out = [a for a in HEAVY if a < n - 1]
    out += [a for a in range(n - 1) if a not in out][:len(HEAVY) - len(out)]
    return tuple(sorted(out))


def main_plan():
    return plan(N, HEAVY)


def top_plan(n):
    return plan(n, top_heavy(n))


def conditions(p, tips):
    """The four conditions of the stakes, on the numbers themselves; tips: light seats that must be able to tip the sum."""
    heavy_first = sorted(p.stakes, reverse=True)
    need = next(i for i in range(1, p.n + 1) if sum(heavy_first[:i]) > p.thr)
    assert need <= MAX_INCLUDES and p.m + p.k <= MAX_INCLUDES  # 1. a valid block within 16 includes
    for tip in tips:  # 2., 3. heavy seats and k light ones at quorum_thr + 1, any light one less at quorum_thr
        assert p.stakes[tip] == 1
        seats = list(p.heavy[:p.m]) + p.lights([tip])
        assert tip in seats and len(set(seats)) == p.m + p.k and p.stake(seats) == p.thr + 1
        for light in seats[p.m:]:
            assert p.stake([a for a in seats if a != light]) == p.thr
    assert sum(p.stakes) < 1 << 32  # 4.
    assert (p.m + 1) * p.H > p.thr and not p.m * p.H > p.thr
    return need


class OracleSigner:
    """Stands in for the engine in Dag and blocks.committee: the CPU oracle signs."""

    def ed25519_sign(self, seeds, msgs):
        return O.sign_batch(np.ascontiguousarray(seeds), np.ascontiguousarray(msgs))


class Case:
    def __init__(self, dag, plan, leaders, **notes):
        self.dag, self.plan, self.leaders, self.notes = dag, plan, list(leaders), notes


def new_dag(engine, p, distinct=False):
    d = Dag(engine, p.n, p.stakes, distinct)
    d.heavy = p.heavy
    return d


def step(d, authors, omit=None, pick=None):
    """One layer: every author includes the first block of every author of the round before (round 1:
    the genesis blocks of the heavy seats); omit: {author: authorities it leaves out}; pick:
    {author: the authorities it includes, and no other}."""
    rnd = len(d.rounds)
    prev = [d.genesis[a] for a in d.heavy] if rnd == 1 else d.first(rnd - 1)
    omit, pick = omit or {}, pick or {}
    specs = []
    for a in authors:
        incs = [r for r in prev if r[0] not in omit.get(a, ())]
        if a in pick:
            incs = [r for r in incs if r[0] in pick[a]]
        specs.append((a, incs))
    return d.layer(specs)


# ---------------------------------------------------------------- one word per row
def word_leader(w):
    return 32 * w if w % 2 == 0 else 32 * w + 31


def word_other(w):
    return 32 * w + 31 if w % 2 == 0 else 32 * w


WORD_LEADERS = [word_leader(w) for w in range(16)]
WORD_BLAMERS = [word_other(w) for w in range(16)]
PRODUCERS = sorted(set(WORD_LEADERS + WORD_BLAMERS + [510, LIGHT_MID]))
LIGHT_LEADERS = [a for a in PRODUCERS if a not in HEAVY][:16]


def one_blame_rounds(d):
    """Rounds 1-4: round 2 has 16 leaders, leader w a seat of word w; in round 3 one voter of word w
    includes no block of leader w, every other voter includes it; round 4 certifies all 16."""
    step(d, PRODUCERS)
    step(d, PRODUCERS)
    step(d, PRODUCERS, omit={s: [a] for s, a in zip(WORD_BLAMERS, WORD_LEADERS)})
    step(d, PRODUCERS)


def one_blame(engine):
    p = main_plan()
    d = new_dag(engine, p)
    one_blame_rounds(d)
    return Case(d, p, [(a, 2) for a in WORD_LEADERS])


def one_vote(engine):
    """16 light leaders at round 1; leader w's block is included by one voter alone, a seat of word w."""
    p = main_plan()
    d = new_dag(engine, p)
    step(d, PRODUCERS)
    omit = {s: [a for a, v in zip(LIGHT_LEADERS, WORD_LEADERS) if v != s] for s in PRODUCERS}
    step(d, PRODUCERS, omit=omit)
    step(d, PRODUCERS)
    return Case(d, p, [(a, 1) for a in LIGHT_LEADERS])


def one_cert(engine):
    """16 light leaders at round 1; leader w has the votes of all heavy seats but two (a pair of its
    own) and of two light ones, quorum_thr + 1; the decision block of a seat of word w includes exactly
    those votes, so every decision block certifies one leader."""
    p = main_plan()
    d = new_dag(engine, p)
    step(d, PRODUCERS)
    lights = p.lights([LIGHT_MID])
    voters = list(p.heavy) + lights
    pairs = list(itertools.combinations(p.heavy, len(p.heavy) - p.m))[:16]
    step(d, voters, omit={h: [a for a, pair in zip(LIGHT_LEADERS, pairs) if h in pair] for h in p.heavy})
    step(d, WORD_LEADERS, pick={c: [v for v in voters if v not in pair] for c, pair in zip(WORD_LEADERS, pairs)})
    return Case(d, p, [(a, 1) for a in LIGHT_LEADERS], certifiers=WORD_LEADERS)


# ---------------------------------------------------------------- the blame edge
def blame_edge_rows(engine, p, rows, lights, distinct=False):
    """rows: (leader, blamers) -- leader k stands at round k + 1 and the blamers' blocks of round k + 2
    include no block of it. One more round ends the DAG."""
    d = new_dag(engine, p, distinct)
    authors = sorted(set(p.heavy) | set(lights))
    step(d, authors)
    for leader, blamers in rows:
        step(d, authors, omit={b: [leader] for b in blamers})
    step(d, authors)
    return Case(d, p, [(leader, k + 1) for k, (leader, _) in enumerate(rows)], blamers=[b for _, b in rows])


def blamers_of(p, leader, tip, with_tip):
    others = [a for a in p.lights([tip]) if a != tip]
    return [a for a in p.heavy if a != leader][:p.m] + others + ([tip] if with_tip else [])


def blame_edge(engine):
    """Leaders at seat 511 and at seat 128, blame at quorum_thr and at quorum_thr + 1; the seat that
    tips the sum is light, in word 15 and in word 4. Distinct keys."""
    p = main_plan()
    rows = [(511, blamers_of(p, 511, LIGHT_W15, False)), (511, blamers_of(p, 511, LIGHT_W15, True)),
            (128, blamers_of(p, 128, LIGHT_W4, False)), (128, blamers_of(p, 128, LIGHT_W4, True))]
    return blame_edge_rows(engine, p, rows, [LIGHT_W4, LIGHT_W15] + p.lights([LIGHT_W4]), distinct=True)


def top_blame(engine, n):
    p = top_plan(n)
    leader, tip = p.heavy[0], n - 1
    rows = [(leader, blamers_of(p, leader, tip, True)), (leader, blamers_of(p, leader, tip, False))]
    return blame_edge_rows(engine, p, rows, p.lights([tip]))


# ---------------------------------------------------------------- votes and certificates at quorum
def edge_set(p, tip, lights, full=True):
    """m heavy and k light seats with `tip` among them (quorum_thr + 1); not full: one light seat less
    (quorum_thr) -- the tip itself when it is light."""
    heavy = ([tip] if tip in p.heavy else []) + [a for a in p.heavy if a != tip]
    light = [a for a in lights if a != tip] + ([tip] if tip not in p.heavy else [])
    return heavy[:p.m] + (light if full else light[:-1])


def vote_edge_rows(engine, p, rows, lights, z):
    """rows: (leader, vote tip, certifier tip, full) -- leader k stands at round 3 k + 1. Every block of
    the next round includes it but z's. In the decision round a certifier includes the votes of an
    edge_set with the vote tip, quorum_thr + 1; every other block the same votes less a light one, and
    z's block: quorum_thr of votes in a valid block. The certifiers are an edge_set with the certifier
    tip, full or not."""
    d = new_dag(engine, p)
    authors = sorted(set(p.heavy) | set(lights) | {z})
    note = []
    for leader, vote_tip, cert_tip, full in rows:
        step(d, authors)
        step(d, authors, omit={z: [leader]})
        certifiers = edge_set(p, cert_tip, lights, full)
        enough, short = edge_set(p, vote_tip, lights), edge_set(p, vote_tip, lights, False) + [z]
        step(d, authors, pick={a: enough if a in certifiers else short for a in authors})
        note.append((certifiers, enough, short))
    return Case(d, p, [(leader, 3 * k + 1) for k, (leader, *_) in enumerate(rows)], sets=note)


def quorum_edge(engine):
    """(64, 1): the vote stake a decision block counts is quorum_thr + 1 with seat 510's vote in it, or
    quorum_thr; the certifiers' stake is quorum_thr + 1 with seat 511 among them. (64, 4): the same with
    seat 256's vote, and certifiers of quorum_thr."""
    p = main_plan()
    return vote_edge_rows(engine, p, [(64, 510, 511, True), (64, 256, 511, False)], [LIGHT_W4, LIGHT_W15], LIGHT_MID)


def top_vote(engine, n):
    p = top_plan(n)
    lights = p.lights([n - 1])
    z = next(a for a in range(n) if a not in p.heavy and a not in lights)
    return vote_edge_rows(engine, p, [(p.heavy[0], n - 1, n - 1, True)], lights, z)


# ---------------------------------------------------------------- equivocation at seat 511
LOW = [a for a in HEAVY if a < 256] + [LIGHT_W4]
HIGH = [a for a in HEAVY if a >= 256] + [LIGHT_W15]


def equivocation(engine, certified):
    """Two leader blocks at seat 511, round 1: B has the votes of the seats below 256, B' of those from
    256 up -- neither half is a quorum (two disjoint sets cannot both be one), so neither block is
    certified. certified = 1: the seats below 256 vote for B' as well, each with a second block;
    certified = 2: the seats from 256 up also do so for B. The decision round includes every voting block."""
    p = main_plan()
    d = new_dag(engine, p)
    authors = sorted(LOW + HIGH)
    g = [d.genesis[a] for a in p.heavy]
    r1 = d.layer([(a, g) for a in authors] + [(511, g[1:] + g[:1])])
    b, b2 = r1[authors.index(511)], r1[-1]
    rest = [r for r in r1 if r[0] != 511]
    specs = [(a, rest + [b if a in LOW else b2]) for a in authors]
    if certified >= 1:
        specs += [(a, rest + [b2]) for a in LOW]
    if certified >= 2:
        specs += [(a, rest + [b]) for a in HIGH]
    r2 = d.layer(specs)
    d.layer([(a, r2) for a in authors])
    return Case(d, p, [(511, 1)], blocks=(b, b2))


def overflow(engine):
    """Nine leader blocks at seat 511: at round 1 every voter includes the first (OVERFLOW), at round
    4 every other heavy seat includes none (a quorum of blame: SKIP)."""
    p = main_plan()
    d = new_dag(engine, p)
    authors = sorted(set(p.heavy) | {LIGHT_W4, LIGHT_W15})
    g = [d.genesis[a] for a in p.heavy]
    d.layer([(a, g) for a in authors] + [(511, g[k:] + g[:k]) for k in range(1, 9)])
    step(d, authors)
    step(d, authors)
    prev = d.first(3)
    d.layer([(a, prev) for a in authors] + [(511, prev[k:] + prev[:k]) for k in range(1, 9)])
    step(d, authors, omit={a: [511] for a in p.heavy if a != 511})
    step(d, authors)
    return Case(d, p, [(511, 1), (511, 4)])


# ---------------------------------------------------------------- the commit sequence
LATER = sorted(HEAVY + (95, 96))  # the seats that go on after the one-word-per-row rounds

def elect_rows():
    """Rows at rounds 2, 5 and 8 (16 committers of round offset 2): the one-word-per-row leaders, then
    seat 480 and seat 511 first in their rounds, the other seats of those rounds, and seat 1, which has no block."""
    at = {2: WORD_LEADERS, 5: [480] + [a for a in LATER if a != 480] + [1], 8: [511] + [a for a in LATER if a != 511] + [1]}
    return [(2, k) for k in range(16)], lambda rnd, offset: at[rnd][offset]


def sequence(engine, linked):
    """The one-word-per-row DAG and six more rounds. (480, 5) has votes of quorum_thr + 1 at round 6 and
    one certificate, seat 0's block of round 7: undecided directly. (511, 8) is committed directly;
    linked: its block includes seat 0's block of round 7 (an indirect COMMIT); else not (an indirect SKIP)."""
    p = main_plan()
    d = new_dag(engine, p)
    one_blame_rounds(d)
    step(d, LATER)
    voters = edge_set(p, 480, [95, 96])
    step(d, LATER, omit={a: [480] for a in LATER if a not in voters})
    step(d, LATER, omit={a: [31] for a in LATER if a != 0})
    step(d, LATER, omit={} if linked else {511: [0]})
    step(d, LATER)
    step(d, LATER)
    committers, elect = elect_rows()
    return Case(d, p, S.leader_rows(committers, elect, len(d.rounds) - 1), committers=committers, elect=elect)


CASES = {
    "one_blame": one_blame, "one_vote": one_vote, "one_cert": one_cert, "blame_edge": blame_edge,
    "quorum_edge": quorum_edge, "equivocation_0": lambda e: equivocation(e, 0), "equivocation_1": lambda e: equivocation(e, 1),
    "equivocation_2": lambda e: equivocation(e, 2), "overflow": overflow,
    "sequence_linked": lambda e: sequence(e, True), "sequence_unlinked": lambda e: sequence(e, False),
}
for _n in TOP_SEATS:
    CASES[f"top_blame_{_n}"] = lambda e, n=_n: top_blame(e, n)
    CASES[f"top_vote_{_n}"] = lambda e, n=_n: top_vote(e, n)


# ---------------------------------------------------------------- what the bitmaps of a row hold
def bitmaps(p, blocks, authority, rnd):
    """The authors of the blame bitmap of row (authority, rnd), and of the vote and the certificate
    bitmap of each of its leader blocks, from the words of include/mysti_verify.h (mv_decide_leaders);
    blocks: reference -> (bincode, includes)."""
    voting = {ref: incs for ref, (_, incs) in blocks.items() if ref[1] == rnd + 1}
    sup = {ref: next((i for i in incs if i[:2] == (authority, rnd)), None) for ref, incs in voting.items()}
    blame = {ref[0] for ref, incs in voting.items() if all(i[0] != authority for i in incs)}
    votes, certs = [], []
    for b in [ref for ref in blocks if ref[:2] == (authority, rnd)]:
        votes.append({ref[0] for ref in voting if sup[ref] == b})
        certs.append({ref[0] for ref, (_, incs) in blocks.items() if ref[1] == rnd + 2 and
                      p.stake({i[0] for i in incs if i in voting and sup[i] == b}) > p.thr})
    return blame, votes, certs


def words_of(seats):
    return {a >> 5 for a in seats}
