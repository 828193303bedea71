"""Crafted bursts for VDL2GPU_F_RAW_FLAGS: frames that hold a data byte 0x7e, at every place where the kernel can go wrong.  What
tests/test_rawflags_model.py holds the CPU model to and tests/test_gpu_rawflags.py the kernel.  A case is (name, (nbrow, nlbyte, data),
sent) as in allframes_cases: `sent` is the hdata of every frame the transmitter put into the burst whole and checking, in stream order --
with this mode all of them come back.  The bursts are built bit by bit (allframes_ref.multi on blocks_craft's pieces).

The un-stuffer's mark for a data byte 0x7e comes from the zero it drops behind the byte's fifth one: several cases put that zero on a
boundary of the raw stream (a raw byte's last or first bit, the row edge, the edge of a lane's span of raw bytes), others put the byte
on a boundary of the un-stuffed bytes (the mark words' edge, the edge of a lane's span in the FCS scan, hdata[1])."""
import functools

import numpy as np

from vdlm2dec_amd import synth

import allframes_cases as Cs
import allframes_ref as A
import blocks_craft as K
import rawflags_ref as R

body = Cs.body


def with_7e(b: bytes, *at) -> bytes:
    b = bytearray(b)
    for i in at:
        b[i] = 0x7e
    return bytes(b)


def _case(name, bodies, sent=None, **kw):
    raw = A.multi(bodies, **kw)
    return name, K.block_of(raw), [A.hdata(b) for b in (bodies if sent is None else sent)]


def _fcs_byte(which: int, n: int = 20) -> bytes:
    """a body without a byte 0x7e whose FCS has 0x7e as its low (0) or high (1) byte, and not as the other"""
    for seed in range(200000):
        b = body(5000 + seed, n)
        fcs = synth.fcs16(b)
        if (fcs >> 8 * which) & 0xff == 0x7e and (fcs >> 8 * (1 - which)) & 0xff != 0x7e:
            return b
    raise AssertionError("no such body")


def data_drops(blk):
    """[(raw bit position of the dropped zero, un-stuffed byte)] of the data bytes 0x7e of a block (as sent: no row needs repair)"""
    nbrow, nlbyte, data = blk
    rows = np.frombuffer(bytes(data), np.uint8).reshape(8, 255)
    src = b"".join(rows[r, :(nlbyte if r == nbrow - 1 else 249)].tobytes() for r in range(nbrow))
    B, _, drops = R.unstuff(src)
    return [(drops[8 * q + 6], q) for q, v in enumerate(B) if v == 0x7e and 8 * q + 6 in drops]


def raw_bytes(blk) -> int:
    return (blk[0] - 1) * 249 + blk[1]


def _shifted(name, ok, n_range, tail: int = 30, second=None):
    """one frame of j bytes 0x1f (each takes one stuffed zero: the bit phase), n low bytes, a data byte 0x7e and `tail` low bytes, then a
    second frame: the first (n, j) at which ok(block, raw bit of the 0x7e's dropped zero) holds"""
    for n in n_range:
        for j in range(9):
            bodies = [b"\x1f" * j + body(300 + n, n, low=True) + b"\x7e" + body(301 + n, tail, low=True), second or body(302, 12)]
            c = _case(name, bodies)
            p = data_drops(c[1])[0][0]        # (the first one: an FCS byte may be another)
            if ok(c[1], p):
                return c
    raise AssertionError(name)


def _lane_edge(blk, p, last: bool) -> bool:
    per = (raw_bytes(blk) + 63) // 64         # k4_lane_span over the raw bytes
    if per < 2:
        return False
    by = p // 8
    return 1 <= by // per < 63 and (by % per == per - 1 and p % 8 == 7 if last else by % per == 0 and p % 8 == 0)


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    out.append(_case("mid", [body(1, 20), with_7e(body(2, 35), 17), body(3, 12)]))
    out.append(_case("first-of-first", [b"\x7e" + body(4, 20), body(5, 15)]))                   # the m1 case
    out.append(_case("first-of-first-flags3", [b"\x7e" + body(4, 20), body(5, 15)], front=b"\0\0", flags_between=3))
    out.append(_case("first-of-later", [body(6, 20), b"\x7e" + body(7, 25), b"\x7e\x7e" + body(8, 12)]))
    out.append(_case("last-of-body", [body(9, 20) + b"\x7e", body(10, 15) + b"\x7e"]))
    out.append(_case("fcs-low", [body(11, 12), _fcs_byte(0), body(12, 12)]))
    out.append(_case("fcs-high", [body(13, 12), _fcs_byte(1), body(14, 12)]))
    out.append(_case("run6", [body(15, 9) + b"\x7e" * 6 + body(16, 9), body(17, 11)]))
    out.append(_case("only-7e", [b"\x7e" * 30, body(18, 9)]))
    out.append(_case("ff7e", [body(19, 12), b"\xff\x7e" * 10, body(20, 12)]))
    out.append(_case("bf7e", [body(21, 12), b"\xbf\x7e" * 9, body(22, 12)]))
    name, blk, sent, _ = Cs.info_7e()
    out.append(("info7e", blk, sent))
    x = body(23, 14)
    fx = synth.fcs16(x)
    out.append(_case("nested", [x + bytes([fx & 0xff, fx >> 8, 0x7e]) + body(24, 20)]))
    # the dropped zero of a data byte 0x7e on the boundaries of the raw stream
    out.append(_shifted("drop-bit7", lambda blk, p: p % 8 == 7, range(20, 21)))
    out.append(_shifted("drop-bit0", lambda blk, p: p % 8 == 0, range(20, 21)))
    out.append(_shifted("drop-row-last", lambda blk, p: p == 8 * 249 - 1, range(225, 250)))
    out.append(_shifted("drop-row-first", lambda blk, p: p == 8 * 249, range(225, 250)))
    long2 = body(303, 200, low=True)
    out.append(_shifted("drop-span-last", lambda blk, p: _lane_edge(blk, p, True), range(100, 140), second=long2))
    out.append(_shifted("drop-span-first", lambda blk, p: _lane_edge(blk, p, False), range(100, 140), second=long2))
    # ... and the byte itself on the boundaries of the un-stuffed bytes: B[0] is the flag, body byte k is B[k + 1]
    out.append(_case("mark31", [with_7e(body(25, 120), 30, 94), body(26, 12)]))
    out.append(_case("mark32", [with_7e(body(27, 120), 31, 95), body(28, 12)]))
    out.append(_case("mark31+32", [with_7e(body(29, 120), 30, 31, 62, 63, 64), body(30, 12)]))
    for where in ("first", "last"):
        for n1 in range(100, 140):
            bodies = [with_7e(body(60, n1), 50), with_7e(body(61, 200), 100)]
            per = (Cs.nb_of(bodies) + 63) // 64
            q = 1 + n1 + 2 + 1 + 100           # the second frame's data byte
            if per > 1 and q % per == (0 if where == "first" else per - 1):
                out.append(_case(f"span-{where}", bodies))
                break
        assert out[-1][0] == f"span-{where}"
    tiny = [with_7e(body(72, 9), 4), body(73, 10), with_7e(body(74, 9), 0, 8)]
    assert Cs.nb_of(tiny) <= 64
    out.append(_case("tiny", tiny))
    full = [with_7e(body(80 + i, 234, low=True), 3 + 29 * i) for i in range(8)]
    name, blk, sent = _case("full8", full)
    assert blk[0] == 8
    out.append((name, blk, sent))
    many = [with_7e(body(100 + i, 9, low=True), i % 9) for i in range(150)]
    assert 1800 <= Cs.nb_of(many) <= 1992
    out.append(_case("many13", many))
    bad = [body(31, 20), with_7e(body(32, 30), 11), body(33, 15)]
    out.append(_case("badfcs", bad, sent=[bad[0], bad[2]], fcs_xor={1: 0x0100}))
    names = [c[0] for c in out]
    assert len(set(names)) == len(names)
    return out


@functools.lru_cache(maxsize=None)
def nested():
    """(block, hdata of the frame sent, hdata of the inner X that was never sent)"""
    c = cases()[[c[0] for c in cases()].index("nested")]
    return c[1], c[2][0], A.hdata(body(23, 14))


@functools.lru_cache(maxsize=None)
def rescue():
    """allframes_cases.rescue() with a data byte 0x7e in the second frame, the one whose row has more errors than rs() repairs: (block
    as received, reliability map that marks the errors, feedback rows that hold the row as sent, frames sent)"""
    import blockrep_ref as BR
    bodies = [body(95, 200), with_7e(body(96, 150), 70, 149)]
    name, blk, sent = _case("rescue", bodies)
    assert blk[0] == 2 and Cs.nb_of(bodies) > 249 + 20
    import feedback_ref as FR
    for seed in range(5, 25):       # (four errors: rs() gives up on most patterns and miscorrects some -- one it gives up on)
        bad, rel = BR.corrupt(blk, np.random.default_rng(seed), 4, row=1)
        if FR.row_rule(bad[2], None, None, 2, blk[1])[1][1] == FR.ROW_FAIL:
            break
    else:
        raise AssertionError("rs() decodes every pattern")
    fb = np.frombuffer(blk[2], np.uint8).reshape(8, 255).copy()
    return bad, rel, fb, sent
