"""CPU model of the block report (vdl2gpu_blockrep_t, VDL2GPU_F_BLOCK_REPORT; the definitions are in include/vdl2gpu.h), built from
pinned pieces only: soft_ref.row_params / rs_decode (the oracle's rs()) / syndromes_zero / rescue_row for the rows, a plain bit loop for
the un-stuffing (vdlm2.c:119-133), a prefix OR for the first flag (vdlm2.c:136-139) and the reflected 0x8408 table for the running FCS
from 0xffff at hdata[1] (check_frame, vdlm2.c:38-61).  tests/test_blockrep_model.py holds it to oracle.frames_of_block,
soft_ref.soft_frames and blocks_craft.unstuff_ref.

    model(nbrow, nlbyte, data, rel=None)  -> demod.BlockReport (rel: the (8, 255) reliability map: soft mode)
    variants() -> [(name, (nbrow, nlbyte, data), rel, nerr)]: crafted blocks with byte errors in one row and a map that marks them
    soft_fail_cases() -> the same shape: rows the soft rule cannot rescue
    many_flags() -> [(name, (nbrow, nlbyte, data))]: bursts of almost nothing but flags, a thousand and more candidates
"""
from __future__ import annotations

import functools

import numpy as np

from vdlm2dec_amd import synth
from vdlm2dec_amd.demod import BlockReport

import blocks_craft as K
import soft_ref as R

NONE, CLEAN, REF, SOFT2, SOFT4, FAIL = range(6)          # VDL2GPU_ROW_*
_HOW = {"s2": SOFT2, "s4": SOFT4, "fail": FAIL}

_FCS = []
for _v in range(256):
    _c = _v
    for _ in range(8):
        _c = (_c >> 1) ^ 0x8408 if _c & 1 else _c >> 1
    _FCS.append(_c)


@functools.lru_cache(maxsize=None)
def _clean(row: bytes) -> bool:
    return R.syndromes_zero(np.frombuffer(row, np.uint8))


def _zero(status: int) -> BlockReport:
    z = (0,) * 8
    return BlockReport(z, z, z, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, status)


def _rows(nbrow, nlbyte, rows, rel):
    """(rows the un-stuffer reads, row_roots, row_how, row_changed)"""
    out = rows.copy()
    roots, how, changed = [0] * 8, [NONE] * 8, [0] * 8
    for r in range(nbrow):
        by, eras, p = R.row_params(r, nbrow, nlbyte)
        recv = rows[r].copy()
        final = recv.copy()
        roots[r] = R.rs_decode(final, eras)              # what the reference leaves, and what it returns
        if roots[r] == 0 and _clean(recv.tobytes()):     # (zero syndromes: rs() returns 0 at once, rs.c:118-123)
            how[r] = CLEAN
        elif roots[r] >= 0:
            how[r] = REF
        elif rel is None:
            how[r] = FAIL
        else:
            final, h = R.rescue_row(recv.copy(), rel[r], by, eras, p)
            how[r] = _HOW[h]
        sent = list(range(by)) + list(range(249, 249 + p))
        changed[r] = int(np.count_nonzero(final[sent] != recv[sent]))
        out[r] = final
    return out, roots, how, changed


def _unstuff(src: bytes):
    """(kept bits, zeros dropped): the loop of vdlm2.c:119-133 without its byte bookkeeping"""
    kept, t, dropped = [], 0, 0
    for v in src:
        for n in range(8):
            if v >> n & 1:
                kept.append(1)
                t += 1
            else:
                if t == 5:
                    t = 0
                    dropped += 1
                    continue
                t = 0
                kept.append(0)
    return kept, dropped


def model(nbrow: int, nlbyte: int, data, rel=None) -> BlockReport:
    return _model(nbrow, nlbyte, bytes(data), None if rel is None else np.asarray(rel, np.uint8).tobytes())


@functools.lru_cache(maxsize=None)
def _model(nbrow, nlbyte, data, relb) -> BlockReport:
    if not (1 <= nbrow <= 8 and 0 <= nlbyte <= 249):
        return _zero(1)
    rows = np.frombuffer(data[:2040].ljust(2040, b"\0"), np.uint8).reshape(8, 255).copy()
    rel = None if relb is None else np.frombuffer(relb, np.uint8).reshape(8, 255)
    out, roots, how, changed = _rows(nbrow, nlbyte, rows, rel)
    src = b"".join(out[r, :(nlbyte if r == nbrow - 1 else 249)].tobytes() for r in range(nbrow))
    kept, stuffed = _unstuff(src)
    nbytes = len(kept) // 8
    B = [sum(kept[8 * i + n] << n for n in range(8)) for i in range(nbytes)]
    flag_at, acc = -1, 0
    for i, v in enumerate(B):                            # hdata[0] is never cleared: the OR of all bytes so far
        acc |= v
        if acc == 0x7e:
            flag_at = i
            break
    cand = short = bad = frames = 0
    if flag_at >= 0:
        m1 = next((i for i in range(flag_at + 1, nbytes) if B[i] != 0x7e), None)     # hdata[1]: flags right behind the first are swallowed
        if m1 is not None:
            c = 0xffff
            for q in range(m1, nbytes):
                v = B[q]
                if v == 0x7e:                            # check_frame(hdata, l), hdata[l - 1] this byte
                    cand += 1
                    if q - m1 + 2 < 13:
                        short += 1
                    elif c != 0xf0b8:
                        bad += 1
                    else:
                        frames += 1
                c = (c >> 8) ^ _FCS[(c ^ v) & 0xff]
    return BlockReport(tuple(roots), tuple(how), tuple(changed), sum(changed), how.count(FAIL), how.count(SOFT2) + how.count(SOFT4),
                       stuffed, nbytes, flag_at, cand, short, bad, frames, 0)


# -------------------------------------------------------------------------------------------------------- the counters' far end
@functools.lru_cache(maxsize=None)
def many_flags():
    """Idle flags fill the burst: every 0x7e behind hdata[1] is a candidate, the first ten of them too short, the others with a wrong FCS -- counts
    of 1024 and more, up to what eight rows hold (1990 bytes: a last row of 1 or 2 bytes has no parity sent and does not survive
    rs(), see blocks_craft.sizes()).  One with a frame that checks in front of the flags: every counter is non-zero."""
    out = [(f"flags{n}", K.block_of(b"\x7e\x01" + b"\x7e" * n)) for n in (1022, 1023, 1034, 1035, 1980, 1988)]
    body = bytes(range(1, 40))
    fcs = synth.fcs16(body)       # (the flags follow in the bit stream, not at the next raw byte: they stay whole un-stuffed bytes)
    out.append(("frame+flags", K.block_of(K.bytes_of(K.FLAG + K.stuff(K.bits_of(body + bytes([fcs & 0xff, fcs >> 8]))) + K.FLAG * 1501))))
    return out


# ---------------------------------------------------------------------------------------------------------------- corrupted blocks
NERR = (1, 3, 4, 5, 9)
STEP = 7             # every STEP-th block of blocks_craft.everything() gets one variant per NERR


def _rel_map(rng, nbrow, nlbyte):
    rel = np.full((8, 255), 255, np.uint8)
    for r in range(nbrow):
        by, _, p = R.row_params(r, nbrow, nlbyte)
        rel[r, :by] = rng.integers(120, 256, by)
        rel[r, 249:249 + p] = rng.integers(120, 256, p)
    return rel


def corrupt(block, rng, nerr: int, row=None):
    """nerr byte errors at transmitted positions of one row (the one with the most of them unless given), and a reliability map whose
    least reliable bytes of that row are the errors.  None when the row has fewer positions than that."""
    nbrow, nlbyte, data = block
    rows = np.frombuffer(bytes(data), np.uint8).reshape(8, 255).copy()
    r = int(rng.integers(0, nbrow)) if row is None else row
    by, _, p = R.row_params(r, nbrow, nlbyte)
    sent = list(range(by)) + list(range(249, 249 + p))
    if len(sent) < nerr:
        return None
    rel = _rel_map(rng, nbrow, nlbyte)
    for j, c in enumerate(rng.choice(sent, size=nerr, replace=False)):
        rows[r, c] ^= int(rng.integers(1, 256))
        rel[r, c] = 5 + 3 * j
    return (nbrow, nlbyte, rows.tobytes()), rel


@functools.lru_cache(maxsize=None)
def variants():
    rng = np.random.default_rng(4242)
    out = []
    for i, (name, block, _) in enumerate(K.everything()):
        if i % STEP:
            continue
        for nerr in NERR:
            v = corrupt(block, rng, nerr)
            if v is not None:
                out.append((f"{name}/e{nerr}", v[0], v[1], nerr))
    return out


@functools.lru_cache(maxsize=None)
def soft_fail_cases():
    """rows the soft rule cannot rescue: a short last row (nlbyte <= 30: four fixed erasures, no trial is made) with errors, and rows
    with 20 and more errors under uniform reliabilities (every trial fails)"""
    rng = np.random.default_rng(99)
    out = []
    body = bytes(v if v != 0x7e else 0x7d for v in rng.integers(0, 256, 249 + 12).tolist())
    short = K.block_of(K.frame(body))               # two rows, the last one short
    assert short[0] == 2 and 3 <= short[1] <= 30
    # (with four erasures rs() has two roots left and finds a single "error" that explains almost any pattern -- REF, a miscorrection;
    # the oracle's rs() picks the patterns it gives up on)
    found = 0
    for _ in range(400):
        nerr = int(rng.integers(2, 7))
        block, rel = corrupt(short, rng, nerr, row=1)
        row = np.frombuffer(block[2], np.uint8).reshape(8, 255)[1].copy()
        if R.rs_decode(row, R.row_params(1, 2, short[1])[1]) < 0:
            out.append((f"shortlast{found}/e{nerr}", block, rel, nerr))
            found += 1
            if found == 2:
                break
    assert found == 2
    full = K.block_of(K.frame(bytes(v if v != 0x7e else 0x7d for v in rng.integers(0, 256, 600).tolist())))
    # (a trial with four erasures is in the same position: soft_ref.rescue_row picks the patterns no trial explains)
    uniform = np.full((8, 255), 200, np.uint8)
    found = 0
    for _ in range(400):
        nerr = int(rng.integers(20, 41))
        block, _ = corrupt(full, rng, nerr, row=1)
        row = np.frombuffer(block[2], np.uint8).reshape(8, 255)[1].copy()
        if R.rescue_row(row, uniform[1], *R.row_params(1, full[0], full[1]))[1] == "fail":
            out.append((f"uniform{found}/e{nerr}", block, uniform, nerr))
            found += 1
            if found == 2:
                break
    assert found == 2
    return out
