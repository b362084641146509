"""Two models of Linearizer::handle_commit (consensus/linearizer.rs:125-166).

Verbatim   collect_sub_dag as the reference writes it: the stack, the mark on push, the stable sort by
           round. Its store holds every block, genesis included (a genesis block has no includes).
LevelRule  the rule of include/mysti_verify.h (mv_linearize): the same order built round by round, top
           down, from the least pair (path(x), j) per block, with the engine's divergences (a round-0
           reference without a record is a leaf; a missing record above round 0 is INCOMPLETE; a marked
           reference is passed over with or without a record) and its status rows.

A reference is any hashable whose [1] is its round. tests/test_linearize_model.py holds the two to each
other; tests/test_gpu_linearize.py holds the engine to LevelRule.
"""
import random

OK, INCOMPLETE, COMMITTED, OVERFLOW, STOPPED = range(5)
MAX_DEPTH, MAX_INCLUDE, BIG = 16, 0xFFFE, 0xFFFF


class Verbatim:
    def __init__(self, blocks):
        self.blocks = blocks  # reference -> includes, every block of the store
        self.committed, self.last_height = set(), 0

    def recover_state(self, sub_dags):
        assert not self.committed and self.last_height == 0
        for height, leader, refs in sub_dags:
            assert height > self.last_height
            self.last_height = height
            self.committed.update(refs)
            assert leader in self.committed

    def collect_sub_dag(self, leader):
        to_commit = []
        buffer = [leader]
        assert leader not in self.committed
        self.committed.add(leader)
        while buffer:
            x = buffer.pop()
            to_commit.append(x)
            for reference in self.blocks[x]:
                assert reference in self.blocks, "We should have the whole sub-dag by now"
                if reference not in self.committed:
                    self.committed.add(reference)
                    buffer.append(reference)
        self.last_height += 1
        return to_commit, self.last_height

    def handle_commit(self, leaders):
        out = []
        for leader in leaders:
            blocks, height = self.collect_sub_dag(leader)
            blocks.sort(key=lambda b: b[1])  # (stable, as sort_by_key is)
            out.append((blocks, height))
        return out


class LevelRule:
    def __init__(self, records, marked=(), last_height=0):
        self.records = dict(records)  # reference -> includes, the blocks with a record
        self.marked, self.last_height = set(marked), last_height

    def mark(self, refs, height):
        self.marked.update(refs)
        self.last_height = max(self.last_height, height)

    def sub_dag(self, leader):
        """(status, the members in output order). Changes nothing."""
        if leader in self.marked:
            return COMMITTED, []
        if leader not in self.records:
            return INCOMPLETE, []
        path, status = {leader: ()}, OK
        edges = {}  # round -> [(includer, j, reference)]

        def joins(x):
            for j, b in enumerate(self.records.get(x, ())):
                if b[1] < x[1]:  # (an include lies below its block)
                    edges.setdefault(b[1], []).append((x, j, b))

        joins(leader)
        while edges:
            rho = max(edges)
            best = {}
            for x, j, b in edges.pop(rho):
                if b in self.marked or b in path:
                    continue
                key = (path[x], min(j, BIG))
                if b not in best or key < best[b]:
                    best[b] = key
            for b, (px, j) in best.items():
                if len(px) >= MAX_DEPTH or j > MAX_INCLUDE:
                    status = max(status, OVERFLOW)
                elif b not in self.records and b[1] > 0:
                    status = max(status, INCOMPLETE)
                else:
                    path[b] = px + (BIG - j,)
            for b in best:
                if b in path:
                    joins(b)
        return status, sorted(path, key=lambda b: (b[1], path[b]))

    def linearize(self, leaders, cap=1 << 62):
        """(blocks, sub rows): state moves for the OK prefix only."""
        blocks, sub, stopped = [], [], False
        for leader in leaders:
            if stopped:
                sub.append([STOPPED, len(blocks), 0, 0])
                continue
            status, members = self.sub_dag(leader)
            if status == OK and len(blocks) + len(members) > cap:
                status = OVERFLOW
            if status != OK:
                sub.append([status, len(blocks), 0, 0])
                stopped = True
                continue
            self.last_height += 1
            sub.append([OK, len(blocks), len(members), self.last_height])
            blocks.extend(members)
            self.marked.update(members)
        return blocks, sub


# ---------------------------------------------------------------- seeded DAGs (the models' own, unsigned)
def random_dag(rng, n_auth, rounds, p_omit=0.2, p_equiv=0.15, p_weak=0.3, p_dup=0.15):
    """reference -> includes for rounds 0..rounds: references are (author, round, k); every block
    includes some blocks of the round before, maybe weak links to any lower round, maybe duplicates,
    in shuffled order."""
    blocks = {(a, 0, 0): [] for a in range(n_auth)}
    by_round = [[(a, 0, 0) for a in range(n_auth)]]
    for r in range(1, rounds + 1):
        layer = []
        for a in range(n_auth):
            if rng.random() < p_omit and (a or layer):  # (the round keeps a block)
                continue
            for k in range(2 if rng.random() < p_equiv else 1):
                prev = [b for b in by_round[r - 1] if rng.random() < 0.8] or [rng.choice(by_round[r - 1])]
                incs = list(prev)
                while r > 1 and rng.random() < p_weak:
                    incs.append(rng.choice(by_round[rng.randrange(0, r - 1)]))
                while rng.random() < p_dup:
                    incs.append(rng.choice(incs))
                rng.shuffle(incs)
                blocks[(a, r, k)] = incs
                layer.append((a, r, k))
        if not layer:
            layer.append((0, r, 0))
            blocks[(0, r, 0)] = [rng.choice(by_round[r - 1])]
        by_round.append(layer)
    return blocks, by_round


def leader_sequence(rng, by_round, first=1):
    """Some blocks of ascending rounds, at most one per round: what a committed sequence looks like."""
    return [rng.choice(layer) for layer in by_round[first:] if rng.random() < 0.6]


def chain(depth):
    """A leader whose deepest block stands `depth` includes below it: one block per round."""
    blocks = {(0, 0, 0): []}
    for r in range(1, depth + 1):
        blocks[(0, r, 0)] = [(0, r - 1, 0)]
    return blocks, (0, depth, 0)
