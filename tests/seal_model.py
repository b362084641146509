"""Helper (not a test): mv_seal_blocks in plain Python -- hashlib's Blake2b, the signed pre-image
restated from BlockDigest::digest_without_signature (crypto.rs:85-128; the bincode layout of
types.rs:93-114 with bincode 1.3.3 defaults), Ed25519 signing restated from RFC 8032 5.1.5 / 5.1.6
on Python integers, and the link rule of include/mysti_verify.h. It imports neither the library
nor the project's builders; tests/test_seal_model.py pins it to RFC 8032 7.1 and to blocks.py."""
import hashlib
import struct

OK, PARSE_ERROR, UNKNOWN_AUTHOR, UNLINKED = range(4)


class InvalidArg(Exception):
    """MV_E_INVALID_ARG: a linked call whose blocks are not in non-decreasing round order."""


# ---------------------------------------------------------------- Ed25519 (RFC 8032 5.1)
P = 2**255 - 19
L = 2**252 + 27742317777372353535851937790883648493
D = -121665 * pow(121666, P - 2, P) % P
_BY = 4 * pow(5, P - 2, P) % P


def _recover_x(y, sign):
    x2 = (y * y - 1) * pow(D * y * y + 1, P - 2, P) % P
    x = pow(x2, (P + 3) // 8, P)
    if (x * x - x2) % P:
        x = x * pow(2, (P - 1) // 4, P) % P
    assert (x * x - x2) % P == 0
    return P - x if (x & 1) != sign else x


_BX = _recover_x(_BY, 0)
BASE = (_BX, _BY, 1, _BX * _BY % P)


def _add(p, q):  # extended coordinates, RFC 8032 5.1.4
    a = (p[1] - p[0]) * (q[1] - q[0]) % P
    b = (p[1] + p[0]) * (q[1] + q[0]) % P
    c = 2 * p[3] * q[3] * D % P
    d = 2 * p[2] * q[2] % P
    e, f, g, h = b - a, d - c, d + c, b + a
    return e * f % P, g * h % P, f * g % P, e * h % P


def _mul(s, p):
    q = (0, 1, 1, 0)
    while s:
        if s & 1:
            q = _add(q, p)
        p = _add(p, p)
        s >>= 1
    return q


_BASE_TABLE = []  # [j 16^i]B for i < 64, j < 16, built on first use


def _mul_base(s):
    if not _BASE_TABLE:
        p = BASE
        for _ in range(64):
            row = [(0, 1, 1, 0)]
            for _ in range(15):
                row.append(_add(row[-1], p))
            _BASE_TABLE.append(row)
            p = _add(row[-1], p)
    q = (0, 1, 1, 0)
    for i in range(64):
        q = _add(q, _BASE_TABLE[i][(s >> (4 * i)) & 15])
    return q


def _compress(p):
    zi = pow(p[2], P - 2, P)
    x, y = p[0] * zi % P, p[1] * zi % P
    return (y | ((x & 1) << 255)).to_bytes(32, "little")


def expand(seed):
    """(a, prefix, public key) of a 32-byte seed."""
    h = hashlib.sha512(seed).digest()
    a = int.from_bytes(h[:32], "little")
    a = (a & ((1 << 254) - 8)) | (1 << 254)
    return a, h[32:], _compress(_mul_base(a))


def sign(seed, msg, key=None):
    a, prefix, pk = key or expand(seed)
    r = int.from_bytes(hashlib.sha512(prefix + msg).digest(), "little") % L
    R = _compress(_mul_base(r))
    k = int.from_bytes(hashlib.sha512(R + pk + msg).digest(), "little") % L
    return R + ((r + k * a) % L).to_bytes(32, "little")


# ---------------------------------------------------------------- bincode -> pre-image
def b2(x):
    return hashlib.blake2b(x, digest_size=32).digest()


class Parsed:
    """author, round, includes [(authority, round, offset of the 32 digest bytes)], pre (a function
    of the current bytes: the include digests may be relinked), sig_pos."""


def parse(b):
    """Parsed, or None where bincode::deserialize::<StatementBlock> fails (trailing bytes allowed)."""
    pos = 0

    def take(k):
        nonlocal pos
        if k > len(b) - pos:
            raise ValueError
        pos += k
        return pos - k

    def u(fmt):
        return struct.unpack_from(fmt, b, take(struct.calcsize(fmt)))[0]

    def ref():  # -> (authority, round, digest offset)
        a, r, l = u("<Q"), u("<Q"), u("<Q")
        if l != 32:
            raise ValueError
        return a, r, take(32)

    def ref_pre(t):  # pieces: big-endian authority and round, then the digest where it lies
        return [struct.pack(">QQ", t[0], t[1]), (t[2], 32)]

    try:
        out = Parsed()
        out.author, out.round, _ = ref()
        pieces = [struct.pack(">QQ", out.author, out.round)]
        out.includes = []
        n_inc = u("<Q")
        if n_inc > len(b):
            raise ValueError
        for _ in range(n_inc):
            t = ref()
            out.includes.append(t)
            pieces += ref_pre(t)
        n_st = u("<Q")
        if n_st > len(b):
            raise ValueError
        for _ in range(n_st):
            tag = u("<I")
            if tag == 0:  # Share: 0x00, the raw transaction bytes
                l = u("<Q")
                pieces += [b"\x00", (take(l), l)]
            elif tag == 1:  # Vote(locator, Accept | Reject(None | Some(locator)))
                t, lo, vote = ref(), u("<Q"), u("<I")
                if vote == 0:
                    pieces += [b"\x01"] + ref_pre(t) + [struct.pack(">Q", lo)]
                elif vote == 1:
                    some = u("<B")
                    if some == 0:
                        pieces += [b"\x02"] + ref_pre(t) + [struct.pack(">Q", lo)]
                    elif some == 1:
                        t2, lo2 = ref(), u("<Q")
                        pieces += [b"\x03"] + ref_pre(t) + [struct.pack(">Q", lo)] + ref_pre(t2) + [struct.pack(">Q", lo2)]
                    else:
                        raise ValueError
                else:
                    raise ValueError
            elif tag == 2:  # VoteRange
                t, s0, s1 = ref(), u("<Q"), u("<Q")
                pieces += [b"\x04"] + ref_pre(t) + [struct.pack(">QQ", s0, s1)]
            else:
                raise ValueError
        tlo, thi, marker, ep, sl = u("<Q"), u("<Q"), u("<B"), u("<Q"), u("<Q")
        if marker > 1 or sl != 64:
            raise ValueError
        out.sig_pos = take(64)
        pieces.append(struct.pack(">QQ", thi, tlo) + bytes([marker]) + struct.pack(">Q", ep))
    except (ValueError, struct.error):
        return None
    out.pre = lambda cur: b"".join(p if isinstance(p, bytes) else bytes(cur[p[0]:p[0] + p[1]]) for p in pieces)
    return out


def preimage(b):
    p = parse(b)
    return None if p is None else p.pre(b)


# ---------------------------------------------------------------- the call
def seal(buf, offs, lens, seeds, link=False):
    """mv_seal_blocks on a bytearray, in place: (status list, msg digests, block digests); raises
    InvalidArg (buf untouched) for a linked call with rounds out of order."""
    n = len(offs)
    blocks = [bytes(buf[o:o + l]) for o, l in zip(offs, lens)]
    parsed = [parse(b) for b in blocks]
    status = [PARSE_ERROR if p is None else (UNKNOWN_AUTHOR if p.author >= len(seeds) else OK) for p in parsed]
    md, bd = [bytes(32)] * n, [bytes(32)] * n
    keys = {}
    table = {}
    if link:
        rounds = [p.round for p in parsed if p is not None]
        if any(y < x for x, y in zip(rounds, rounds[1:])):
            raise InvalidArg
        for i, p in enumerate(parsed):
            if status[i] == OK:
                table.setdefault((p.author, p.round), i)  # the lowest index holds the key
    # ascending index is ascending round in a linked call: every linked digest exists when it is read
    for i, p in enumerate(parsed):
        if status[i] != OK:
            continue
        if link and any(r >= p.round and (a, r) in table for a, r, _ in p.includes):
            status[i] = UNLINKED
            continue
        cur = bytearray(blocks[i])
        if link:
            for a, r, at in p.includes:
                j = table.get((a, r))
                if j is not None and status[j] == OK:  # (r < p.round here, so j < i and j is final)
                    cur[at:at + 32] = bd[j]
        pre = p.pre(cur)
        md[i] = b2(pre)
        if p.author not in keys:
            keys[p.author] = expand(seeds[p.author])
        sig = sign(None, md[i], keys[p.author])
        bd[i] = b2(pre + sig)
        cur[p.sig_pos:p.sig_pos + 64] = sig
        cur[24:56] = bd[i]
        buf[offs[i]:offs[i] + lens[i]] = cur
    return status, md, bd


def unseal(blocks):
    """The blocks (bincode, all parsing) as a caller hands them to a linked seal call: own digest and
    signature zeroed, and the digest of every include that names a block of the list."""
    parsed = [parse(b) for b in blocks]
    own = {(p.author, p.round) for p in parsed}
    out = []
    for b, p in zip(blocks, parsed):
        cur = bytearray(b)
        cur[24:56] = bytes(32)
        cur[p.sig_pos:p.sig_pos + 64] = bytes(64)
        for a, r, at in p.includes:
            if (a, r) in own:
                cur[at:at + 32] = bytes(32)
        out.append(bytes(cur))
    return out


def pack(blocks, gaps=None, fill=0xA5):
    """(bytearray, offs, lens): the blocks one after another, gaps[i] guard bytes before block i and
    16 after the last."""
    buf, offs = bytearray(), []
    for i, b in enumerate(blocks):
        buf += bytes([fill]) * (gaps[i] if gaps else 0)
        offs.append(len(buf))
        buf += b
    buf += bytes([fill]) * 16
    return buf, offs, [len(b) for b in blocks]
