"""CPU model of VDL2GPU_F_ALL_FRAMES / VDL2GPU_BLK_ALL_FRAMES (the rule is in include/vdl2gpu.h): every frame of a burst, not only the
first.  Built from pinned pieces: feedback_ref.row_rule for the rows (the reference's rs(), then the feedback row, then the soft trials),
blockrep_ref's bit loop for the un-stuffing and its FCS table; the rest is the rule restated in plain Python -- the first flag by a prefix
OR, m1 behind the flags that follow it, then one segment per 0x7e with the FCS run from 0xffff behind every flag.
tests/test_allframes_model.py holds it to the transmitter (synth.hdlc_payload_multi) and, for the first frame, to oracle.frames_of_block.

    model(nbrow, nlbyte, data, rel=None, fb=None) -> (frames, counts)
        frames: hdata of every segment that passes, in stream order (all of them: the library keeps the first NCAND)
        counts: dict(cand, too_short, bad_fcs, frames) as vdl2gpu_blockrep_t counts them in this mode
    multi(bodies, flags_between=1, front=b"") -> raw burst bytes: front | flag | stuffed body + FCS | flags | ... | flag
    hdata(body) -> the frame out() is handed for `body`
"""
from __future__ import annotations

import numpy as np

from vdlm2dec_amd import synth

import blockrep_ref as BR
import blocks_craft as K
import feedback_ref as FR

NCAND = 12          # K4_NCAND: passing frames of one burst the library keeps


def unstuffed_bytes(nbrow: int, nlbyte: int, data, rel=None, fb=None) -> list:
    """the whole un-stuffed bytes B[0..nb) behind the row rule"""
    rows, _ = FR.row_rule(bytes(data)[:2040].ljust(2040, b"\0"), fb, rel, nbrow, nlbyte)
    src = b"".join(rows[r, :(nlbyte if r == nbrow - 1 else 249)].tobytes() for r in range(nbrow))
    kept, _ = BR._unstuff(src)
    return [sum(kept[8 * i + n] << n for n in range(8)) for i in range(len(kept) // 8)]


def segments(B: list):
    """[(s_j, q_j)] of the rule, or [] without hdata[1]"""
    acc, flag_at = 0, -1
    for i, v in enumerate(B):
        acc |= v
        if acc == 0x7e:
            flag_at = i
            break
        if acc & ~0x7e:
            break
    if flag_at < 0:
        return []
    m1 = next((i for i in range(flag_at + 1, len(B)) if B[i] != 0x7e), None)
    if m1 is None:
        return []
    out, s = [], m1
    for q in range(m1, len(B)):
        if B[q] == 0x7e:
            out.append((s, q))
            s = q + 1
    return out


def model(nbrow: int, nlbyte: int, data, rel=None, fb=None):
    counts = dict(cand=0, too_short=0, bad_fcs=0, frames=0)
    frames = []
    if not (1 <= nbrow <= 8 and 0 <= nlbyte <= 249):
        return frames, counts
    B = unstuffed_bytes(nbrow, nlbyte, data, rel, fb)
    for s, q in segments(B):
        counts["cand"] += 1
        l = q - s + 2
        if l < 13:
            counts["too_short"] += 1
            continue
        c = 0xffff
        for v in B[s:q]:
            c = (c >> 8) ^ BR._FCS[(c ^ v) & 0xff]
        if c != 0xf0b8:
            counts["bad_fcs"] += 1
            continue
        counts["frames"] += 1
        frames.append(bytes([0x7e] + B[s:q + 1]))
    return frames, counts


def hdata(body: bytes) -> bytes:
    return synth.hdlc_frame(bytes(body))


def multi(bodies, flags_between: int = 1, front: bytes = b"", fcs_xor=None) -> bytes:
    """the raw bytes of a burst of several frames, bit by bit as blocks_craft builds one.  fcs_xor: {index of a body: mask xored into its
    FCS before stuffing} -- a frame that does not check"""
    bits = K.bits_of(front) + list(K.FLAG)
    for j, body in enumerate(bodies):
        if j:
            bits += list(K.FLAG) * (flags_between - 1)
        fcs = synth.fcs16(bytes(body)) ^ ((fcs_xor or {}).get(j, 0))
        bits += K.stuff(K.bits_of(bytes(body) + bytes([fcs & 0xff, fcs >> 8]))) + list(K.FLAG)
    return K.bytes_of(bits)
