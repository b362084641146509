"""Helper (not a test): the direct decision rule of the committers, restated twice in plain Python,
for tests/test_commit_model.py (which holds the two to each other) and tests/test_gpu_decide.py
(which holds mv_decide_leaders to the second).

  Verbatim     BaseCommitter::try_direct_decide as consensus/base_committer.rs writes it: a
               dict-of-dicts block store (round -> (authority, digest) -> block), the recursive
               find_support (:109-134), is_vote, is_certificate with its all_votes cache (:152-180),
               enough_leader_blame (:228-249), enough_leader_support with the total_stake quick
               reject (:253-289), StakeAggregator::add with its early exits (committee.rs:314-320),
               any wave length. Where the reference panics it raises Panic.
  DirectRule   the restatement of include/mysti_verify.h (mv_decide_leaders): sets of authors and
               whole stake sums at wave length 3, over a list of records.

A block is (reference, includes): reference = (authority, round, digest), includes a list of
references in include order. Nothing here is shared with the library's kernels."""
import random

UNDECIDED, COMMIT, SKIP, CONFLICT, OVERFLOW = range(5)
MAX_LEADER_BLOCKS = 8


class Panic(Exception):
    pass


class StakeAggregator:  # committee.rs:257-320, QuorumThreshold
    def __init__(self, model):
        self.m, self.votes, self.stake = model, set(), 0

    def add(self, authority):
        if authority not in self.votes:
            self.votes.add(authority)
            self.stake += self.m.stakes[authority]
        return self.m.is_quorum(self.stake)


class Verbatim:
    def __init__(self, stakes, wave_length=3):
        assert wave_length >= 3
        self.stakes = list(stakes)
        self.quorum_threshold = 2 * sum(self.stakes) // 3  # committee.rs:56-57
        self.wave_length = wave_length
        self.index = {}  # BlockStore: round -> {(authority, digest): (reference, includes)}

    def is_quorum(self, amount):  # committee.rs:125-127
        return amount > self.quorum_threshold

    def add(self, ref, includes):
        self.index.setdefault(ref[1], {})[(ref[0], ref[2])] = (ref, list(includes))

    def get_block(self, ref):
        return self.index.get(ref[1], {}).get((ref[0], ref[2]))

    def get_blocks_by_round(self, rnd):
        return list(self.index.get(rnd, {}).values())

    def get_blocks_at_authority_round(self, authority, rnd):
        return [b for (a, _), b in self.index.get(rnd, {}).items() if a == authority]

    def find_support(self, author, rnd, frm):  # :109-134
        ref, includes = frm
        if ref[1] < rnd:
            return None
        for inc in includes:
            if (inc[0], inc[1]) == (author, rnd):
                return inc
            if inc[1] <= rnd:
                continue
            block = self.get_block(inc)
            if block is None:
                raise Panic("We should have the whole sub-dag by now")
            support = self.find_support(author, rnd, block)
            if support is not None:
                return support
        return None

    def is_vote(self, potential_vote, leader_block):  # :138-145
        a, r, _ = leader_block[0]
        return self.find_support(a, r, potential_vote) == leader_block[0]

    def is_certificate(self, potential_certificate, leader_block, all_votes):  # :152-180
        agg = StakeAggregator(self)
        for reference in potential_certificate[1]:
            if reference in all_votes:
                is_vote = all_votes[reference]
            else:
                potential_vote = self.get_block(reference)
                if potential_vote is None:
                    raise Panic("We should have the whole sub-dag by now")
                is_vote = self.is_vote(potential_vote, leader_block)
                all_votes[reference] = is_vote
            if is_vote and agg.add(reference[0]):
                return True
        return False

    def enough_leader_blame(self, voting_round, leader):  # :228-249
        agg = StakeAggregator(self)
        for ref, includes in self.get_blocks_by_round(voting_round):
            if all(inc[0] != leader for inc in includes) and agg.add(ref[0]):
                return True
        return False

    def enough_leader_support(self, decision_round, leader_block):  # :253-289
        decision_blocks = self.get_blocks_by_round(decision_round)
        total_stake = sum(self.stakes[ref[0]] for ref, _ in decision_blocks)
        if total_stake < self.quorum_threshold + 1:  # Committee::quorum_threshold() is the field + 1 (:79-81)
            return False
        agg, all_votes = StakeAggregator(self), {}
        for block in decision_blocks:
            if self.is_certificate(block, leader_block, all_votes) and agg.add(block[0][0]):
                return True
        return False

    def try_direct_decide(self, authority, rnd):  # :323-357, for the committer whose round_offset makes rnd a leader round
        """-> (SKIP, None) | (COMMIT, reference) | (UNDECIDED, None); raises Panic."""
        if self.enough_leader_blame(rnd + 1, authority):
            return SKIP, None
        offset = rnd % self.wave_length
        wave = (rnd - offset) // self.wave_length
        decision_round = wave * self.wave_length + self.wave_length - 1 + offset
        supported = [b for b in self.get_blocks_at_authority_round(authority, rnd)
                     if self.enough_leader_support(decision_round, b)]
        if len(supported) > 1:
            raise Panic("More than one certified block")
        return (COMMIT, supported[0][0]) if supported else (UNDECIDED, None)


class Row:
    def __init__(self, status, ref, found, stakes, supported):
        self.status, self.ref, self.found, self.stakes, self.supported = status, ref, found, stakes, supported

    def words(self, authority, rnd):
        """The eight words of the out row."""
        if self.status == COMMIT:
            a, r, d = self.ref
            return [a, r] + [int.from_bytes(d[8 * i:8 * i + 8], "little") for i in range(4)] + [COMMIT, self.found]
        return [authority, rnd, 0, 0, 0, 0, self.status, self.found]


class DirectRule:
    """include/mysti_verify.h, mv_decide_leaders: the records are the stored blocks."""

    def __init__(self, stakes):
        self.stakes = list(stakes)
        self.threshold = 2 * sum(self.stakes) // 3
        self.records = []  # (reference, includes), in the order they were stored

    def add(self, ref, includes):
        self.records.append((ref, list(includes)))

    def stake(self, authors):
        return sum(self.stakes[a] for a in authors)

    def decide(self, authority, rnd) -> Row:
        if authority >= len(self.stakes):
            return Row(UNDECIDED, None, 0, (0, 0, 0), 0)
        have = {ref for ref, _ in self.records}
        voting = [b for b in self.records if b[0][1] == rnd + 1]
        decision = [b for b in self.records if b[0][1] == rnd + 2]
        leader_blocks = [b[0] for b in self.records if b[0][:2] == (authority, rnd)]
        blame = self.stake({ref[0] for ref, incs in voting if all(i[0] != authority for i in incs)})

        def support(incs):
            return next((i for i in incs if i[:2] == (authority, rnd)), None)

        sup = {ref: support(incs) for ref, incs in voting}
        per_block = []
        for b in leader_blocks:
            vote = self.stake({ref[0] for ref, _ in voting if sup[ref] == b})
            certs = set()
            for ref, incs in decision:
                voters = {i[0] for i in incs if i in have and i[1] == rnd + 1 and sup[i] == b}
                if self.stake(voters) > self.threshold:
                    certs.add(ref[0])
            per_block.append((vote, self.stake(certs), b))
        enough = [x for x in per_block if x[1] > self.threshold]
        found = len(leader_blocks)
        if found > MAX_LEADER_BLOCKS:
            vote = cert = 0
        elif len(enough) == 1:
            vote, cert = enough[0][:2]
        else:
            vote, cert = max((x[:2] for x in per_block), default=(0, 0))
        lowest = min((ref[1] for ref, _ in self.records), default=None)
        if lowest is None or rnd < lowest:
            status = UNDECIDED
        elif blame > self.threshold:
            status = SKIP
        elif found > MAX_LEADER_BLOCKS:
            status = OVERFLOW
        elif len(enough) == 1:
            status = COMMIT
        elif len(enough) > 1:
            status = CONFLICT
        else:
            status = UNDECIDED
        return Row(status, enough[0][2] if status == COMMIT else None, found, (blame, vote, cert), len(enough))


def random_dag(rng: random.Random, n_auth, rounds, p_shun=0.4, p_keep=0.95, p_shunned=0.06, p_weak=0.25, p_equiv=0.35,
               p_shuffle=0.5):
    """Blocks (reference, includes) of rounds 0..rounds in a causal order (round by round). Per
    round some authorities are shunned: most blocks of the next round omit them (the omitted leader),
    some of those link to an older block of theirs instead (a weak link); an authority may equivocate
    with a second block of its own includes; include order is own-first or shuffled."""
    by_round = [[(a, 0, rng.randbytes(32)) for a in range(n_auth)]]
    out = [(ref, []) for ref in by_round[0]]
    for r in range(1, rounds + 1):
        prev = by_round[r - 1]
        shunned = {a for a in range(n_auth) if rng.random() < p_shun}
        cur = []
        for a in range(n_auth):
            for _ in range(2 if rng.random() < p_equiv else 1):
                incs = []
                for ref in prev:
                    keep = p_shunned if ref[0] in shunned and ref[0] != a else p_keep
                    if rng.random() < keep:
                        incs.append(ref)
                    elif r >= 2 and rng.random() < p_weak:
                        older = [x for x in by_round[r - 2] if x[0] == ref[0]]
                        incs.append(rng.choice(older))
                incs.sort(key=lambda x: x[0] != a)  # own first (core.rs:264-278)
                if rng.random() < p_shuffle:
                    rng.shuffle(incs)
                ref = (a, r, rng.randbytes(32))
                cur.append(ref)
                out.append((ref, incs))
        by_round.append(cur)
    return out
