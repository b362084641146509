"""A plain big-integer model of what the batch path's preparation kernel (k_bv_prep, batch.hip)
must produce for given inputs and a given coefficient key: the status of every signature, its
coefficient z_i and the product z_i k_i mod l, the affine rows of R and A, and the per-group sums
of z_i s_i. It restates the rule of ed25519-consensus 2.1.0's batch::Verifier that batch.hip
follows,

    [8]( -[sum z_i s_i]B + sum [z_i]R_i + sum [z_i k_i]A_i ) == O,

with this engine's choice of z_i (a keyed hash of the call and the signature's index) on top of
oracle/zip215.py's point arithmetic. Nothing here looks at the engine.
"""
import hashlib

import zip215 as Z

GROUP_CHUNK = 1024   # groups are whole chunks of this many signatures
MAX_GROUPS = 16


def coefficient(secret: bytes, call: int, i: int) -> int:
    """z_i: the first 16 bytes (little-endian) of BLAKE2b-256(secret || call || i), bit 127 cleared."""
    assert len(secret) == 32
    h = hashlib.blake2b(secret + call.to_bytes(8, "little") + i.to_bytes(8, "little"), digest_size=32).digest()
    return int.from_bytes(h[:16], "little") & ((1 << 127) - 1)


def group_geometry(n: int, want: int):
    """(groups, signatures per group): `want` groups, at most 16 and at most one per chunk, of
    equally many whole chunks (the last group may be shorter, and groups left empty are dropped)."""
    nchunk = -(-n // GROUP_CHUNK)
    g = min(max(want, 1), MAX_GROUPS, nchunk)
    cpg = -(-nchunk // g)
    return -(-nchunk // cpg), cpg * GROUP_CHUNK


def affine_rows(pt):
    """(y+x, y-x, 2dxy) mod p of an affine point (x, y, 1, xy)."""
    x, y = pt[0], pt[1]
    return (y + x) % Z.P, (y - x) % Z.P, 2 * Z.D * x * y % Z.P


class Lane:
    __slots__ = ("status", "z", "zk", "s", "k", "R", "A")


class Prep:
    """lanes[i]; groups, group_sigs; sums[g] = sum of z_i s_i over group g's accepted lanes."""

    def __init__(self, lanes, groups, group_sigs):
        self.lanes, self.groups, self.group_sigs = lanes, groups, group_sigs
        self.sums = [sum(l.z * l.s for l in lanes[g * group_sigs:(g + 1) * group_sigs]) for g in range(groups)]


_decoded = {}


def _decompress(enc: bytes):
    if enc not in _decoded:
        _decoded[enc] = Z.decompress(enc)
    return _decoded[enc]


def prep(msg, sig, pk, secret: bytes, call: int, groups: int = 1, z=None) -> Prep:
    """The model of one preparation over rows msg[i] (bytes), sig[i] (64 bytes), pk[i] (32 bytes).
    z (optional): coefficients to use instead of the keyed hash's (the CPU tests show with it what
    equal coefficients would let through)."""
    lanes = []
    for i, (m, sg, a) in enumerate(zip(msg, sig, pk)):
        m, sg, a = bytes(m), bytes(sg), bytes(a)
        ln = Lane()
        ln.A, ln.R = _decompress(a), _decompress(sg[:32])
        ln.s = int.from_bytes(sg[32:], "little")
        ln.k = Z.sha512_mod_l(sg[:32], a, m)
        ln.status = 2 if ln.A is None else (1 if ln.s >= Z.L or ln.R is None else 0)
        ln.z = (coefficient(secret, call, i) if z is None else z[i]) if ln.status == 0 else 0
        ln.zk = ln.z * ln.k % Z.L
        lanes.append(ln)
    g, gs = group_geometry(len(lanes), groups)
    return Prep(lanes, g, gs)


def equation_holds(p: Prep, g: int = 0) -> bool:
    """[8](-[sum z s]B + sum [z]R + sum [zk]A) == O over group g's accepted lanes."""
    acc = Z.neg(Z.scalarmult(Z.B_POINT, p.sums[g] % Z.L))
    for ln in p.lanes[g * p.group_sigs:(g + 1) * p.group_sigs]:
        if ln.status == 0:
            acc = Z.add(acc, Z.scalarmult(ln.R, ln.z))
            acc = Z.add(acc, Z.scalarmult(ln.A, ln.zk))
    for _ in range(3):
        acc = Z.double(acc)
    return Z.is_identity(acc)


def cancelling_pair(sig, i: int, j: int, delta: int):
    """Copies of the signature rows with s_i + delta and s_j - delta (mod l): each is rejected by
    single verification, and their errors cancel in a sum with equal coefficients."""
    out = [bytes(x) for x in sig]
    for r, d in ((i, delta), (j, -delta)):
        s = (int.from_bytes(out[r][32:], "little") + d) % Z.L
        out[r] = out[r][:32] + s.to_bytes(32, "little")
    return out
