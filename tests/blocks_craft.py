"""Burst records that reach the edges of the block path (vdlm2.c:84-161): streams no transmitter makes, flags the hunt has to find
or swallow, nested frame candidates, frames that end on the burst's last bit.  The frames a record is expected to give always come
from oracle.frames_of_block; a builder only says how many it means to produce, and tests/test_blocks_craft.py holds it to that.

Bits are in the order the un-stuffing loop reads them: bit 0 of a byte first."""
import collections
import functools

import numpy as np

from vdlm2dec_amd import synth

FLAG = [0, 1, 1, 1, 1, 1, 1, 0]


def bits_of(data) -> list:
    return [(b >> n) & 1 for b in bytes(data) for n in range(8)]


def bytes_of(bits) -> bytes:
    bits = list(bits) + [0] * (-len(bits) % 8)
    return bytes(sum(bits[i + n] << n for n in range(8)) for i in range(0, len(bits), 8))


def stuff(bits, t: int = 0) -> list:
    """the transmitter's rule: a zero behind every five ones.  t: the run of ones the receiver has counted in front of these bits
    (five: the zero it is about to drop comes first; more than five: it drops nothing until the run has ended)"""
    out = []
    if t == 5:
        out.append(0)
        t = 0
    for b in bits:
        out.append(b)
        if b:
            t += 1
            if t == 5:
                out.append(0)
                t = 0
        else:
            t = 0
    return out


Unstuffed = collections.namedtuple("Unstuffed", "hdata k s t cands")


def _unstuff_bits(bits) -> Unstuffed:
    h, k, s, t, cands = [0], 0, 0, 0, []
    for b in bits:
        if b:
            h[k] |= 1 << s
            t += 1
        else:
            if t == 5:
                t = 0
                continue
            t = 0
        s += 1
        if s == 8:
            s = 0
            if h[k] == 0x7e:
                if k == 0:
                    k += 1
                    h.append(0)
                elif k == 1:
                    h[1] = 0
                else:
                    cands.append(k + 1)
                    k += 1
                    h.append(0)
            elif k > 0:
                k += 1
                h.append(0)
    return Unstuffed(h, k, s, t, cands)


def unstuff_ref(raw) -> Unstuffed:
    """the loop of vdlm2.c:119-152 over all bytes of a burst: hdata[0..k], k, s, t, and the lengths check_frame() was called with"""
    return _unstuff_bits(bits_of(raw))


def block_of(raw: bytes, full_last: bool = False):
    """(nbrow, nlbyte, data) with true parity, as synth.received_rows lays a burst out (FEC shortening included).  full_last: a
    burst of a multiple of 249 bytes as nlbyte == 249 (a length of 1..7 bits less than that many bytes), not as an empty last row"""
    if not full_last:
        return synth.received_rows(bytes(raw))
    assert raw and len(raw) % 249 == 0 and len(raw) <= 8 * 249
    nbrow = len(raw) // 249
    rows = np.zeros((8, 255), np.uint8)
    for r in range(nbrow):
        rows[r, :249] = np.frombuffer(bytes(raw[249 * r:249 * r + 249]), np.uint8)
        rows[r, 249:] = synth.rs_parity(rows[r, :249].tolist())
    return nbrow, 249, rows.tobytes()


def witness(raw_prefix: bytes) -> bytes:
    """raw_prefix begins with a flag and holds at least ten body bytes: append what makes of it one CRC-clean frame -- stuffed zeros
    up to hdata's byte boundary, the stuffed FCS-16 of hdata[1:], a flag"""
    bits = bits_of(raw_prefix)
    u = _unstuff_bits(bits)
    assert raw_prefix[0] == 0x7e and u.k >= 1
    bits += stuff([0] * (-u.s % 8), u.t)
    u = _unstuff_bits(bits)
    assert u.s == 0 and u.k >= 11, "too short for check_frame"
    fcs = synth.fcs16(bytes(u.hdata[1:u.k]))
    bits += stuff(bits_of([fcs & 0xff, fcs >> 8]), u.t) + FLAG
    return bytes_of(bits)


def frame(body: bytes, front: bytes = b"", flags: int = 1) -> bytes:
    """front | `flags` flags | stuffed body and FCS | flag"""
    fcs = synth.fcs16(body)
    return bytes_of(bits_of(front) + FLAG * flags + stuff(bits_of(bytes(body) + bytes([fcs & 0xff, fcs >> 8]))) + FLAG)


def nested(m: int, rng, first: int = 9, more: int = 6, flag_bytes: bool = False) -> bytes:
    """m candidates that share their start: the last two body bytes of candidate i are the FCS of everything from hdata[1] up to
    them, the flags of the candidates before it included.  flag_bytes: every body also holds a data byte 0x7e, which closes a
    candidate of its own (one that fails)"""
    h, bits = [], list(FLAG)
    for i in range(m):
        n = first if i == 0 else int(rng.integers(0, more + 1))
        body = [int(v) for v in rng.integers(0, 256, n)]
        body = [v if v != 0x7e else 0x7d for v in body]
        if flag_bytes and n >= 2:
            body[int(rng.integers(1, n))] = 0x7e       # not the first byte: a flag right behind the first one is swallowed
        h += body
        fcs = synth.fcs16(bytes(h))
        piece = body + [fcs & 0xff, fcs >> 8]
        h += [fcs & 0xff, fcs >> 8, 0x7e]
        bits += stuff(bits_of(piece)) + FLAG
    return bytes_of(bits)


# ------------------------------------------------------------------------------------------------ the sets the tests use
# every entry: (name, (nbrow, nlbyte, data), frames the builder means it to give)
SIZES = (13, 14, 63, 64, 65, 127, 128, 129, 249, 250, 498, 1991, 1992)


def _exact(nby: int, extra: int, seed: int) -> bytes:
    """a frame whose raw stream is 8 * nby + extra bits long: the body's bytes are below 0x10 (no run of five), so only the FCS is
    stuffed -- draw bodies until it takes `extra` bits"""
    rng = np.random.default_rng(seed)
    while True:
        body = bytes(rng.integers(1, 16, nby - 4, dtype=np.uint8).tolist())
        fcs = synth.fcs16(body)
        bits = FLAG + stuff(bits_of(body + bytes([fcs & 0xff, fcs >> 8]))) + FLAG
        if len(bits) == 8 * nby + extra:
            return bytes_of(bits)


@functools.lru_cache(maxsize=None)
def sizes():
    """One frame filling nby bytes to the last bit: the closing flag is the burst's last byte.  And the same kind of frame one bit
    longer, cut to nby bytes -- the flag's last bit is missing: no frame.  A last row of one byte (nby 250) is all the reference
    needs to lose the frame: no parity is transmitted for it, four erasures stand over six missing bytes, and rs() "corrects" the
    lone flag to the nearer all-zero codeword."""
    out = []
    for nby in SIZES:
        raw = _exact(nby, 0, nby)
        cut = _exact(nby, 1, nby)[:nby]
        assert len(raw) == nby and raw[-1] == 0x7e
        lays = [False, True] if nby in (249, 498) else [nby == 1992]
        for full in lays:
            tag = f"{nby}{'f' if full else ''}"
            out.append((f"size{tag}", block_of(raw, full), 0 if nby == 250 else 1))
            out.append((f"size{tag}-1bit", block_of(cut, full), 0))
    return out


@functools.lru_cache(maxsize=None)
def one_runs():
    """bodies of one repeated byte whose stuffed stream drifts through all eight bit alignments, over 130 consecutive lengths; the
    longest 0xff bodies fill the burst's eight rows to within its last 8 bytes"""
    out = []
    for fill in (0x1f, 0x3e, 0xf8, 0xff, 0xdf):
        for n in range(40, 170):
            out.append((f"run{fill:02x}x{n}", block_of(frame(bytes([fill]) * n)), 1))
    n = 1600
    while len(frame(b"\xff" * (n + 1))) <= 1991:
        n += 1
    raw = frame(b"\xff" * n)
    assert 1992 - 8 <= len(raw) <= 1991
    out.append((f"runffx{n}", block_of(raw), 1))
    return out


HEAVY = (0xff, 0x7f, 0xfe, 0x3f, 0xfc, 0xdf, 0xfb, 0x00)


@functools.lru_cache(maxsize=None)
def streams():
    """witness() over raw bytes no transmitter sends: runs of 5, 6, 7, 8..40 and more ones that start and end on byte, lane and row
    boundaries, whole lanes of 0xff"""
    rng = np.random.default_rng(501)
    out = []
    for i in range(300):
        nbrow = 1 + i % 8
        total = int(rng.integers(max(20, 249 * (nbrow - 1) + 3), 249 * nbrow - 8))
        n = total - 1
        pre = np.where(rng.random(n) < 0.7, rng.choice(HEAVY, n), rng.integers(0, 256, n)).astype(np.uint8)
        pre[:10] = rng.integers(0, 0x7e, 10)       # ten body bytes whatever follows
        if i % 10 == 0:
            per = (total + 10 + 63) // 64
            at = int(rng.integers(10, max(11, n - 4 * per)))
            pre[at:at + 3 * per + int(rng.integers(0, per + 1))] = 0xff
        raw = witness(b"\x7e" + pre.tobytes())
        if len(raw) >= 249 * nbrow or len(raw) % 249 in (1, 2):      # (a last row of 1 or 2 bytes: see sizes())
            raw = witness(b"\x7e" + pre[:n - 8].tobytes())
        out.append((f"stream{i}", block_of(raw), 1))
    return out


def _body(seed: int, n: int) -> bytes:
    rng = np.random.default_rng(seed)
    return bytes(v if v != 0x7e else 0x7d for v in rng.integers(0, 256, n).tolist())


@functools.lru_cache(maxsize=None)
def flag_hunt():
    out = []
    b = _body(7, 40)
    for z in (0, 1, 63, 64, 65, 500):
        out.append((f"zeros{z}", block_of(frame(b, bytes(z))), 1))
    out.append(("or3c42", block_of(frame(b, b"\x3c\x42", flags=0)), 1))            # the OR completes without a flag byte
    out.append(("or-bits", block_of(frame(b, b"\x02\x04\x08\x10\x20\x40", flags=0)), 1))
    out.append(("or3c42+flag", block_of(frame(b, b"\x3c\x42")), 1))                # ... and the real flag behind it is swallowed
    for v in (0x01, 0x80):
        out.append((f"stray{v:02x}", block_of(frame(b, bytes([0, v, 0]))), 0))     # a bit outside 0x7e: no flag will ever be seen
        out.append((f"stray{v:02x}-without", block_of(frame(b, bytes([0, 0]))), 1))
    for f in (1, 2, 5, 70):
        out.append((f"flags+{f}", block_of(frame(_body(8, 90), flags=1 + f)), 1))
    # the first flag in the last byte of a lane, the first body byte in the first of the next (about 300 un-stuffed bytes: 5 a lane)
    b = _body(9, 300)
    for z in range(16):
        raw = frame(b, bytes(z))
        u = unstuff_ref(raw)
        nb = z + u.k        # whole un-stuffed bytes of the burst: the zeros, then hdata[0..k)
        per = (nb + 63) // 64
        if per > 1 and z % per == per - 1:
            out.append((f"m0m1-lanes{z}", block_of(raw), 1))
            break
    assert out[-1][0].startswith("m0m1")
    return out


@functools.lru_cache(maxsize=None)
def thresholds():
    """check_frame() refuses l < 13 (vdlm2.c:44): candidates of 12, 13 and 14 bytes with a correct FCS"""
    return [(f"len{l}", block_of(frame(_body(l, l - 4))), 0 if l < 13 else 1) for l in (12, 13, 14)]


NESTED = (2, 3, 12, 13, 14)


@functools.lru_cache(maxsize=None)
def nested_blocks():
    rng = np.random.default_rng(77)
    out = []
    for m in NESTED:
        out.append((f"nested{m}", block_of(nested(m, rng)), m))
        out.append((f"nested{m}-7e", block_of(nested(m, rng, first=12, more=9, flag_bytes=True)), m))
    out.append(("nested3-long", block_of(nested(3, rng, first=700, more=500)), 3))
    return out


def everything():
    return sizes() + one_runs() + streams() + flag_hunt() + thresholds() + nested_blocks()
