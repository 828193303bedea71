"""CPU model of VDL2GPU_F_RAW_FLAGS / VDL2GPU_BLK_RAW_FLAGS (the rule is in include/vdl2gpu.h): every frame of a burst, a flag being six
adjacent ones of the stuffed bit stream, so that a stuffed data byte 0x7e is data.  Built like allframes_ref: feedback_ref.row_rule for the
rows, then blockrep_ref's bit loop (vdlm2.c:119-133) -- here carrying t out of it -- and the rule restated in plain Python.

    unstuff(src) -> (B, t7, drops): the whole un-stuffed bytes, t as the loop has it when it reads each byte's bit 7, and the un-stuffed
        bit offsets in front of which a zero was dropped (with the raw bit that was dropped: drops[offset] = raw bit position)
    true_flags(B, t7) / true_flags_by_drop(B, drops) -> F[q], in the header's form and in the equivalent one
    model(nbrow, nlbyte, data, rel=None, fb=None) -> (frames, counts), as allframes_ref.model gives them
    has_data_7e(nbrow, nlbyte, data, rel=None, fb=None): some un-stuffed byte 0x7e has a dropped zero inside
"""
from __future__ import annotations

import allframes_ref as A
import blockrep_ref as BR
import feedback_ref as FR

NCAND = A.NCAND


def unstuff(src: bytes):
    kept, t, t_at, drops = [], 0, [], {}
    for i, v in enumerate(src):
        for n in range(8):
            if v >> n & 1:
                t_at.append(t)
                kept.append(1)
                t += 1
            else:
                if t == 5:
                    t = 0
                    drops[len(kept)] = 8 * i + n
                    continue
                t_at.append(t)
                t = 0
                kept.append(0)
    nb = len(kept) // 8
    B = [sum(kept[8 * q + n] << n for n in range(8)) for q in range(nb)]
    return B, [t_at[8 * q + 7] for q in range(nb)], drops


def true_flags(B, t7):
    return [v == 0x7e and t == 6 for v, t in zip(B, t7)]


def true_flags_by_drop(B, drops):
    return [v == 0x7e and 8 * q + 6 not in drops for q, v in enumerate(B)]


def source(nbrow, nlbyte, data, rel, fb) -> bytes:
    rows, _ = FR.row_rule(bytes(data)[:2040].ljust(2040, b"\0"), fb, rel, nbrow, nlbyte)
    return b"".join(rows[r, :(nlbyte if r == nbrow - 1 else 249)].tobytes() for r in range(nbrow))


def segments(B, F):
    """[(s_j, q_j)] of the rule, or [] without hdata[1]"""
    acc, flag_at = 0, -1
    for i, v in enumerate(B):       # flag_at keeps the reference's definition
        acc |= v
        if acc == 0x7e:
            flag_at = i
            break
        if acc & ~0x7e:
            break
    if flag_at < 0:
        return []
    m1 = next((q for q in range(flag_at + 1, len(B)) if not F[q]), None)
    if m1 is None:
        return []
    out, s = [], m1
    for q in range(m1, len(B)):
        if F[q]:
            out.append((s, q))
            s = q + 1
    return out


def model(nbrow: int, nlbyte: int, data, rel=None, fb=None, by_drop: bool = False):
    counts = dict(cand=0, too_short=0, bad_fcs=0, frames=0)
    frames = []
    if not (1 <= nbrow <= 8 and 0 <= nlbyte <= 249):
        return frames, counts
    B, t7, drops = unstuff(source(nbrow, nlbyte, data, rel, fb))
    F = true_flags_by_drop(B, drops) if by_drop else true_flags(B, t7)
    for s, q in segments(B, F):
        counts["cand"] += 1
        if q - s + 2 < 13:
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


def has_data_7e(nbrow: int, nlbyte: int, data, rel=None, fb=None) -> bool:
    if not (1 <= nbrow <= 8 and 0 <= nlbyte <= 249):
        return False
    B, _, drops = unstuff(source(nbrow, nlbyte, data, rel, fb))
    return any(v == 0x7e and any(8 * q + n in drops for n in range(1, 8)) for q, v in enumerate(B))
