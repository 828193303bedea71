"""Crafted bursts of several HDLC frames for VDL2GPU_F_ALL_FRAMES: what tests/test_allframes_model.py holds the CPU model to and
tests/test_gpu_allframes.py the kernel.  A case is (name, (nbrow, nlbyte, data), sent): `sent` is the hdata of every frame the
transmitter put into the burst whole and checking, in stream order -- what the rule of include/vdl2gpu.h must give back.  The bursts
are built bit by bit (allframes_ref.multi on blocks_craft's pieces), so that a boundary can be put on a chosen byte.

A frame's l is its body + 2 FCS bytes + 2 flags: a body of 9 bytes (an AVLC frame with an empty info field) is the shortest that passes."""
import functools

import numpy as np

from vdlm2dec_amd import synth

import allframes_ref as A
import blocks_craft as K


def body(seed: int, n: int, low: bool = False) -> bytes:
    """n bytes, none of them 0x7e; low: all below 0x10, so that nothing but the FCS is ever stuffed"""
    rng = np.random.default_rng(1000 + seed)
    if low:
        return bytes(rng.integers(1, 16, n, dtype=np.uint8).tolist())
    return bytes(v if v != 0x7e else 0x7d for v in rng.integers(0, 256, n).tolist())


def _case(name, bodies, sent=None, **kw):
    raw = A.multi(bodies, **kw)
    return name, K.block_of(raw), [A.hdata(b) for b in (bodies if sent is None else sent)]


def nb_of(bodies, front: int = 0, flags_between: int = 1) -> int:
    """whole un-stuffed bytes of such a burst"""
    return front + 1 + sum(len(b) + 2 for b in bodies) + len(bodies) + (len(bodies) - 1) * (flags_between - 1)


def _unstuffed_fcs(b: bytes) -> bool:
    """the frame's stuffed stream is as long as the unstuffed one: flags stay on raw byte boundaries"""
    fcs = synth.fcs16(b)
    bits = K.bits_of(b + bytes([fcs & 0xff, fcs >> 8]))
    return len(K.stuff(bits)) == len(bits)


def _plain(seed: int, n: int) -> bytes:
    while True:
        b = body(seed, n, low=True)
        if _unstuffed_fcs(b):
            return b
        seed += 7919


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    out.append(_case("two", [body(1, 20), body(2, 35)]))
    out.append(_case("three", [body(3, 20), body(4, 50), body(5, 11)]))
    out.append(_case("flags2", [body(6, 20), body(7, 35), body(8, 12)], flags_between=2))
    out.append(_case("flags3", [body(9, 20), body(10, 35)], flags_between=3))
    out.append(_case("flags70", [body(9, 20), body(10, 35)], flags_between=70))
    empty = synth.avlc_frame(b"")
    assert len(empty) == 9
    out.append(_case("l13", [body(11, 20), empty, body(12, 15)]))
    short = body(13, 8)
    out.append(_case("l12", [body(14, 20), short, body(15, 15)], sent=[body(14, 20), body(15, 15)]))
    out.append(_case("badmid", [body(16, 20), body(17, 30), body(18, 15)], sent=[body(16, 20), body(18, 15)], fcs_xor={1: 0x0100}))
    out.append(_case("badfirst", [body(19, 20), body(20, 30)], sent=[body(20, 30)], fcs_xor={0: 0x0001}))
    out.append(_case("thirteen", [body(30 + i, 9 + i) for i in range(13)]))
    out.append(_case("ff", [b"\xff" * 40, body(21, 9) + b"\xff" * 25, b"\xff" * 9]))
    # the first frame's closing flag in the last byte of row 0 and in the first byte of row 1 (nothing is stuffed: raw byte = un-stuffed byte)
    for at in (248, 249):
        b1, b2 = _plain(40 + at, at - 3), _plain(50 + at, 30)
        name, blk, sent = _case(f"rowedge{at}", [b1, b2])
        rows = np.frombuffer(blk[2], np.uint8).reshape(8, 255)
        assert blk[0] == 2 and (rows[0, 248] if at == 248 else rows[1, 0]) == 0x7e
        out.append((name, blk, sent))
    # a lane owns per = ceil(nb / 64) bytes: the flag between the two frames in the first and in the last byte of a lane's span
    for where in ("first", "last"):
        for n1 in range(100, 140):
            bodies = [body(60, n1), body(61, 200)]
            per = (nb_of(bodies) + 63) // 64
            q0 = 1 + n1 + 2
            if per > 1 and q0 % per == (0 if where == "first" else per - 1):
                out.append(_case(f"span-{where}", bodies))
                break
        assert out[-1][0] == f"span-{where}"
    # about 1900 bytes of frames of l = 13: two and three closing flags in every span, and many more frames than are kept
    many = [body(100 + i, 9, low=True) for i in range(150)]
    assert 1800 <= nb_of(many) <= 1992 and (nb_of(many) + 63) // 64 >= 26
    out.append(_case("many13", many))
    # a frame of 1500 bytes (some fifty lanes without a flag), then a short one
    out.append(_case("long+short", [body(70, 1500, low=True), body(71, 12)]))
    tiny = [body(72, 9), body(73, 10), body(74, 9)]
    assert nb_of(tiny) <= 64
    out.append(_case("tiny", tiny))
    full = [body(80 + i, 236, low=True) for i in range(8)]
    name, blk, sent = _case("full8", full)
    assert blk[0] == 8
    out.append((name, blk, sent))
    return out


@functools.lru_cache(maxsize=None)
def info_7e():
    """Info bytes of 0x7e.  The un-stuffer hands a stuffed data byte 0x7e on as the byte 0x7e, which the rule (like check_frame's caller,
    vdlm2.c:143) takes for a flag: (name, block, the frames sent, those of them that hold no data byte 0x7e)"""
    bodies = [body(90, 20), body(91, 9) + b"\x7e" * 6 + body(92, 9), body(93, 15), b"\xff\x7e" * 10]
    name, blk, sent = _case("info7e", bodies)
    return name, blk, sent, [A.hdata(b) for b in bodies if 0x7e not in b]


@functools.lru_cache(maxsize=None)
def rescue():
    """Two frames over two rows; the row that carries the second frame has four byte errors, more than rs() repairs.  (block as received,
    reliability map that marks the errors, feedback rows that hold the row as sent, frames sent)"""
    import blockrep_ref as BR
    bodies = [body(95, 200), body(96, 150)]
    name, blk, sent = _case("rescue", bodies)
    assert blk[0] == 2 and nb_of(bodies) > 249 + 20
    rng = np.random.default_rng(5)
    bad, rel = BR.corrupt(blk, rng, 4, row=1)
    fb = np.frombuffer(blk[2], np.uint8).reshape(8, 255).copy()
    return bad, rel, fb, sent
