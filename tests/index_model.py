"""Helper (not a test): what mv_accept_blocks and the mv_index_* calls compute, restated twice in
plain Python over sets and dicts, for tests/test_index_model.py (which holds the two to each other)
and tests/test_gpu_index.py (which holds the library to the second).

  Reference     the reference's own structures: BlockManager (block_manager.rs:19-145: blocks_pending,
                block_references_waiting, missing, the store's set of references, the whole of
                add_blocks with its sort, suspend and unlock cascade) under process_blocks
                (net_sync.rs:314-386: the `processed` query, the skip, verify, the early return of
                a message with a rejected block, add_blocks).
  TwoState      the restatement of include/mysti_verify.h: one dict reference -> MV_REF_WANTED /
                MV_REF_HAVE and the five steps of an accept call.

One accept call is one interleaving of the reference's peer tasks: every message's `processed`
query runs before any add_blocks, and the accepted messages' blocks reach BlockManager::add_blocks
as one vector (with one message per call this is process_blocks itself; the header's step 5 -- an
include that is a NEW block of the same call is not missing -- is add_blocks' sort by round over
that vector).

Whether a block decodes and what StatementBlock::verify says of it comes from `verdicts`
(replay_model.oracle_verdicts: the CPU oracle). References are (authority, round, digest) tuples
read with struct.unpack. Nothing here is shared with the library's kernels.

RefTable is a reference hash table for probe lengths: open addressing, linear probing, slot starts
from keyed hashlib.blake2b."""
import hashlib
import struct
from collections import deque

import numpy as np

ABSENT, WANTED, HAVE = 0, 1, 2
REJECTED, NEW, KNOWN, DUP, DROPPED = range(5)
BLOCK_OK, BLOCK_PARSE_ERROR = 0, 1
REF_BYTES = 56


def own_ref(b: bytes):
    """The reference a block claims (bytes 0..56), or None: under 56 bytes, or a length word that is not 32."""
    if len(b) < REF_BYTES:
        return None
    a, r, dl = struct.unpack_from("<QQQ", b, 0)
    return (a, r, bytes(b[24:56])) if dl == 32 else None


def includes(b: bytes):
    """The includes of a block that parsed: u64 count at byte 56, 56 bytes each from byte 64."""
    (k,) = struct.unpack_from("<Q", b, 56)
    out = []
    for j in range(k):
        a, r, dl = struct.unpack_from("<QQQ", b, 64 + 56 * j)
        assert dl == 32
        out.append((a, r, bytes(b[64 + 56 * j + 24:64 + 56 * j + 56])))
    return out


def ref_words(refs) -> np.ndarray:
    out = np.zeros((len(refs), 6), dtype=np.uint64)
    for i, (a, r, d) in enumerate(refs):
        out[i, 0], out[i, 1] = a, r
        out[i, 2:] = np.frombuffer(d, dtype="<u8")
    return out


def words_ref(row):
    return (int(row[0]), int(row[1]), np.asarray(row[2:], dtype="<u8").tobytes())


def run_verdicts(verdicts, blocks):
    """verdicts over a list of byte strings (packed as the tests pack them)."""
    if not blocks:
        return []
    lens = np.array([len(b) for b in blocks], dtype=np.uint64)
    offs = np.zeros(len(blocks), dtype=np.uint64)
    offs[1:] = np.cumsum(lens)[:-1]
    img = np.frombuffer(b"".join(blocks) + b"\0", dtype=np.uint8)
    return [int(v) for v in verdicts(img[:-1], offs, lens)]


def group_slices(n, groups):
    """[(lo, hi)] of the groups of n blocks (groups: non-decreasing words, or None)."""
    if groups is None:
        return [(i, i + 1) for i in range(n)]
    out, lo = [], 0
    for i in range(1, n + 1):
        if i == n or groups[i] != groups[lo]:
            out.append((lo, i))
            lo = i
    return out


class Reference:
    """BlockManager under process_blocks, structure for structure."""

    def __init__(self, n_auth, verdicts, genesis):
        self.verdicts = verdicts
        self.store = set(genesis)  # BlockStore::block_exists
        self.blocks_pending = {}
        self.block_references_waiting = {}
        self.missing = [set() for _ in range(n_auth)]

    def exists_or_pending(self, ref):  # block_manager.rs:142-144
        return ref in self.store or ref in self.blocks_pending

    def add_blocks(self, blocks):  # block_manager.rs:48-136
        blocks = deque(sorted(blocks, key=lambda b: own_ref(b)[1]))  # stable, by round
        newly_processed, missing_references = [], set()
        while blocks:
            block = blocks.popleft()
            ref = own_ref(block)
            if ref in self.store or ref in self.blocks_pending:
                continue
            processed = True
            for inc in includes(block):
                if inc not in self.store:
                    processed = False
                    if inc not in self.block_references_waiting and inc not in self.blocks_pending:
                        missing_references.add(inc)
                    self.block_references_waiting.setdefault(inc, set()).add(ref)
                    if inc not in self.blocks_pending:
                        self.missing[inc[0]].add(inc)
            self.missing[ref[0]].discard(ref)
            if not processed:
                self.blocks_pending[ref] = block
            else:
                self.store.add(ref)  # block_writer.insert_block
                newly_processed.append(ref)
                for waiting in sorted(self.block_references_waiting.pop(ref, ())):
                    pointer = self.blocks_pending[waiting]
                    if all(i not in self.block_references_waiting for i in includes(pointer)):
                        blocks.appendleft(self.blocks_pending.pop(waiting))
        return newly_processed, missing_references

    def accept(self, blocks, groups=None):
        """-> (the `processed` answer per block, the set of missing references returned)."""
        refs = [own_ref(b) for b in blocks]
        processed = [r is not None and self.exists_or_pending(r) for r in refs]  # net_sync.rs:325-328
        todo = [i for i in range(len(blocks)) if not processed[i]]
        verdict = dict(zip(todo, run_verdicts(self.verdicts, [blocks[i] for i in todo])))
        to_process = []
        for lo, hi in group_slices(len(blocks), groups):
            mine = [i for i in range(lo, hi) if not processed[i]]  # :331-336
            if all(verdict[i] == BLOCK_OK for i in mine):  # else: return Err(e), :352-361
                to_process += [blocks[i] for i in mine]
        missing = self.add_blocks(to_process)[1] if to_process else set()
        return processed, missing

    def missing_blocks(self):  # block_manager.rs:138-140
        return [set(s) for s in self.missing]


class Accepted:
    def __init__(self, blk_status, blk_state, missing):
        self.blk_status, self.blk_state, self.missing, self.n_missing = blk_status, blk_state, missing, len(missing)


class TwoState:
    """include/mysti_verify.h: the index as a dict, and the five steps of mv_accept_blocks."""

    def __init__(self, verdicts, genesis=()):
        self.verdicts = verdicts
        self.state = {r: HAVE for r in genesis}

    def lookup(self, ref):
        return self.state.get(ref, ABSENT)

    def insert(self, refs, state):
        """-> the states before the call (every duplicate reports the state before the call)."""
        prior = [self.lookup(r) for r in refs]
        for r in refs:
            self.state[r] = max(self.lookup(r), state)
        return prior

    def counts(self):
        v = list(self.state.values())
        return v.count(HAVE), v.count(WANTED)

    def wanted(self):
        return {r for r, s in self.state.items() if s == WANTED}

    def missing_blocks(self, n_auth):
        out = [set() for _ in range(n_auth)]
        for r in self.wanted():
            out[r[0]].add(r)
        return out

    def accept(self, blocks, groups=None) -> Accepted:
        n = len(blocks)
        refs = [own_ref(b) for b in blocks]
        known = [r is not None and self.lookup(r) == HAVE for r in refs]  # 1. probe
        todo = [i for i in range(n) if not known[i]]
        status = [BLOCK_OK] * n  # 2. verify
        for i, v in zip(todo, run_verdicts(self.verdicts, [blocks[i] for i in todo])):
            status[i] = v
        state = [KNOWN if known[i] else (REJECTED if status[i] != BLOCK_OK else NEW) for i in range(n)]
        for lo, hi in group_slices(n, groups):  # 3. groups
            if any(state[i] == REJECTED for i in range(lo, hi)):
                for i in range(lo, hi):
                    if state[i] == NEW:
                        state[i] = DROPPED
        seen = set()  # 4. own references
        for i in range(n):
            if state[i] == NEW:
                if refs[i] in seen:
                    state[i] = DUP
                else:
                    seen.add(refs[i])
                    self.state[refs[i]] = HAVE
        missing = []  # 5. includes
        for i in range(n):
            if state[i] == NEW:
                for inc in includes(blocks[i]):
                    if self.lookup(inc) == ABSENT:
                        self.state[inc] = WANTED
                        missing.append(inc)
        return Accepted(status, state, missing)


class RefTable:
    """Open addressing with linear probing over `slots` slots (a power of two); a key's first slot
    comes from blake2b keyed with `secret`. insert returns the slots examined."""

    def __init__(self, slots, secret=b"index-model"):
        assert slots & (slots - 1) == 0
        self.slots, self.secret, self.tab = slots, secret, {}
        self.longest = 0

    def start(self, key: bytes) -> int:
        return int.from_bytes(hashlib.blake2b(key, key=self.secret, digest_size=8).digest(), "little") & (self.slots - 1)

    def insert(self, key: bytes) -> int:
        p, probe = self.start(key), 1
        while p in self.tab and self.tab[p] != key:
            p, probe = (p + 1) & (self.slots - 1), probe + 1
            assert probe <= self.slots
        self.tab[p] = key
        self.longest = max(self.longest, probe)
        return probe
