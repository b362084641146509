"""The proposer's side of Core, as the reference writes it, and the batch form the kernels use.

Core       ThresholdClockAggregator::add_block (threshold_clock.rs:58-89) over StakeAggregator::add
           (committee.rs:314-320), the loop of Core::add_blocks (core.rs:181-200) with run_block_handler's
           entry (:223-224), the include choice of Core::try_new_block (:232-278) and the own-block
           lines (:307-320, :110-116), line for line: a Python set of references, a list for `pending`.
BatchRule  the same clock and queue over a whole call at once: the rows in segments of equal round,
           per segment the first row at which the stake of first-seen authors passes the quorum, and a
           short chain over the segments (propose.hip: k_pp_seg, k_pp_chain).

A reference is any hashable whose first two items are (authority, round). The block store is `blocks`:
reference -> its includes; what is not in it is a block get_block gives None for."""

IN_ORDER, PAYLOAD = 1, 2
INCOMPLETE, SHORT = 1, 2
NO_ENTRY = 0xFFFFFFFFFFFFFFFF


class Core:
    def __init__(self, stakes, authority):
        self.stakes = list(stakes)
        self.quorum_threshold = 2 * sum(self.stakes) // 3  # committee.rs:56-57
        self.authority = authority
        self.round, self.votes, self.stake = 0, set(), 0  # ThresholdClockAggregator::new(0)
        self.pending = []  # (position, ("include", reference)) | (position, ("payload", token))
        self.own = None    # (reference, includes)
        self.blocks = {}
        self.takes, self.dropped = 0, 0

    # StakeAggregator::add (committee.rs:314-320)
    def _add(self, vote):
        stake = self.stakes[vote]
        if vote not in self.votes:
            self.votes.add(vote)
            self.stake += stake
        return self.stake > self.quorum_threshold

    def _clear(self):
        self.votes, self.stake = set(), 0

    # threshold_clock.rs:58-89
    def add_block(self, ref):
        authority, rnd = ref[0], ref[1]
        if rnd < self.round:
            pass
        elif rnd > self.round:
            self._clear()
            self._add(authority)
            self.round = rnd
        else:
            if self._add(authority):
                self._clear()
                self.round = rnd + 1

    # core.rs:181-200, 223-224; in_order: the loops of Core::open (:90-94, :104-109)
    def add_blocks(self, processed, positions=None, in_order=False, payload=None):
        positions = [0] * len(processed) if positions is None else list(positions)
        rows = list(zip(positions, processed))
        if not in_order:
            rows.sort(key=lambda pr: pr[1][1])  # sorted_by round: stable
        for position, ref in rows:
            self.add_block(ref)
            self.pending.append((position, ("include", ref)))
        if payload is not None:
            self.pending.append((payload, ("payload", payload)))
        return self.clock()

    def clock(self):
        return [self.round, self.stake, len(self.votes), len(self.pending)]

    def last_proposed(self):
        return self.own[0][1]

    # core.rs:232-278; None, or (clock_round, includes without the own last block, payloads, entries
    # taken, flags, next_entry)
    def try_new_block(self):
        clock_round = self.round
        if clock_round <= self.last_proposed():
            return None
        first_include_index = len(self.pending)
        for i, (_, (kind, what)) in enumerate(self.pending):
            if kind == "include" and what[1] >= clock_round:
                first_include_index = i
                break
        taken, self.pending = self.pending[:first_include_index], self.pending[first_include_index:]
        references_in_block = set(self.own[1])
        flags = 0
        for _, (kind, what) in taken:
            if kind == "include":
                if what in self.blocks:
                    references_in_block.update(self.blocks[what])
                elif what[1] != 0:
                    flags |= INCOMPLETE
        includes, statements, entries = [], [], 0
        for _, (kind, what) in taken:
            if kind == "include":
                entries += 1
                if what not in references_in_block:
                    includes.append(what)
            else:
                statements.append(what)
        self.takes += 1
        self.dropped = entries - len(includes)
        self.choice = includes
        next_entry = self.pending[0][0] if self.pending else NO_ENTRY
        return clock_round, includes, statements, len(taken), flags, next_entry

    # core.rs:307-320 (includes None: the own last block, then the choice) and :110-116
    def own_block(self, ref, includes=None):
        if includes is None:
            includes = [self.own[0]] + list(self.choice)
        self.add_block(ref)
        self.own = (ref, list(includes))
        self.blocks[ref] = list(includes)
        return self.clock()

    def stats(self, outstanding):
        return self.clock() + [self.own[0][1] if self.own else 0, int(outstanding), self.takes, self.dropped]


class BatchRule:
    """The clock and the queue of a call at once. State: round, the voters, their stake."""

    def __init__(self, stakes):
        self.stakes = list(stakes)
        self.quorum_threshold = 2 * sum(self.stakes) // 3
        self.round, self.votes, self.stake = 0, set(), 0
        self.pending = []

    def segment(self, rows, lo, hi):
        """k_pp_seg over rows[lo:hi] (one round): first flags, pos0, pos1, the stake of all authors."""
        seen, first, pre, s = set(), [], [], 0
        for a, _ in rows[lo:hi]:
            f = a not in seen
            seen.add(a)
            first.append(f)
            s += self.stakes[a] if f else 0
            pre.append(s)
        hits = [o for o, p in enumerate(pre) if p > self.quorum_threshold]
        pos0 = hits[0] if hits else None
        later = [o for o in hits if o >= 1]
        pos1 = later[0] if later else None
        return first, pos0, pos1, s

    def clock_rows(self, rows):
        """k_pp_chain over the segments of rows ((authority, round) in the order the automaton takes them)."""
        i, n = 0, len(rows)
        while i < n:
            r = rows[i][1]
            e = i
            while e < n and rows[e][1] == r:
                e += 1
            if r >= self.round:
                first, pos0, pos1, stot = self.segment(rows, i, e)
                greater = r > self.round
                if greater or not self.votes:
                    p = pos1 if greater else pos0
                    if p is not None:
                        self.round, self.votes, self.stake = r + 1, set(), 0
                    else:
                        self.votes = {rows[i + o][0] for o in range(e - i) if first[o]}
                        self.round, self.stake = r, stot
                else:
                    s, hit = self.stake, False
                    for o in range(e - i):
                        a = rows[i + o][0]
                        if first[o] and a not in self.votes:
                            s += self.stakes[a]
                            new = True
                        else:
                            new = False
                        if s > self.quorum_threshold:
                            hit = True
                            break
                        if new:
                            self.votes.add(a)
                    if hit:
                        self.round, self.votes, self.stake = r + 1, set(), 0
                    else:
                        self.stake = s
            i = e

    def add(self, processed, positions=None, in_order=False, payload=None):
        positions = [0] * len(processed) if positions is None else list(positions)
        order = list(range(len(processed)))
        if not in_order:
            # the stable sort as k_pp_bit_* run it: a pass for every bit in which two rounds of the call differ
            ones_somewhere = zeros_somewhere = 0
            for p in processed:
                ones_somewhere |= p[1]
                zeros_somewhere |= ~p[1] & (1 << 64) - 1
            for bit in range(64):
                if (ones_somewhere & zeros_somewhere) >> bit & 1:
                    zeros = [j for j in order if not (processed[j][1] >> bit) & 1]
                    ones = [j for j in order if (processed[j][1] >> bit) & 1]
                    order = zeros + ones
        rows = [processed[j] for j in order]
        self.clock_rows([(r[0], r[1]) for r in rows])
        self.pending += [(positions[j], ("include", processed[j])) for j in order]
        if payload is not None:
            self.pending.append((payload, ("payload", payload)))
        return [self.round, self.stake, len(self.votes), len(self.pending)]
