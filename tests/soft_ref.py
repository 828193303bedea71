"""numpy restatement of soft-decision RS erasures (VDL2GPU_F_SOFT_RS; the definitions are in include/vdl2gpu.h), built from pinned
pieces only: the oracle's 84 kS/s tap, mflt[] and the Grey tables as the library holds them (csrc/vdl2_tables.inc), the oracle's
atan2f, descrambler and rs(), and its trigger's clk.

    soft_block(x, block, trig, pn)   -> (hard bytes, reliability map), both (8, 255) uint8
    row_rule(data, rel, nbrow, nlbyte) -> the block after the row rule (what k4_frames decodes in soft mode)
    channel_maps(raw, fmt, rate, fo, fc) -> [(oracle Block, hard, rel)] of one channel
"""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np

from levels_ref import mflt_taps

ROWS, ROWLEN = 8, 255
_TAB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vdlm2dec_amd", "csrc", "vdl2_tables.inc")


def _table(name: str, n: int) -> np.ndarray:
    text = open(_TAB).read()
    body = text[text.index(f"VDL2_TABLE_BEGIN({name}, {n})"):]
    body = body[:body.index("VDL2_TABLE_END")]
    words = [int(w, 16) for w in re.findall(r"VDL2_F32\((0x[0-9a-f]+)u\)", body)]
    assert len(words) == n
    return np.array(words, np.uint32).view(np.float32)


GREY = np.stack([_table(f"grey{w}", 257) for w in (1, 2, 3)])          # (3, 257) float32
# R(w, idx) = min(255, floor(|Grey_w[idx] - 0.5| * 512))
REL = np.minimum(255, np.floor(np.abs(GREY.astype(np.float64) - 0.5) * 512)).astype(np.uint8)
MFLT = mflt_taps()


def geom(nbrow: int, nlbyte: int):
    """burst_geom (vdl2gpu_machine.h): nd_rows, nd_last, nf_rows, nf_last, ND, NF, nsym"""
    nd_last = nlbyte if nlbyte else 249
    ND = (nbrow - 1) * 249 + nd_last
    if nlbyte <= 2:
        nf_rows, nf_last = nbrow - 1, 6
    else:
        nf_rows, nf_last = nbrow, (2 if nlbyte <= 30 else (4 if nlbyte <= 67 else 6))
    NF = (nf_rows - 1) * 6 + nf_last if nf_rows > 0 else 0
    return nbrow, nd_last, nf_rows, nf_last, ND, NF, (25 + 8 * (ND + NF) + 2) // 3


def scatter(b: int, g) -> tuple:
    """(row, col) of payload byte b: the receiver's column-major walk (d8psk.c:117-206) in closed form"""
    nd_rows, nd_last, nf_rows, nf_last, ND, _, _ = g
    if b < ND:
        rows, last, bb, base = nd_rows, nd_last, b, 0
    else:
        rows, last, bb, base = nf_rows, nf_last, b - ND, 249
    full = last * rows
    if bb < full:
        return bb % rows, base + bb // rows
    bb -= full
    return bb % (rows - 1), base + last + bb // (rows - 1)


def timing(clk0: int):
    """burst_timing: (j0, rb) -- first symbol at trigger + j0, filter sub-phase rb"""
    j = max(1, int((32 - clk0 + 3) / 4))
    return j, clk0 + 4 * j - 32


def phases(x: np.ndarray, n: np.ndarray, c: int) -> np.ndarray:
    """filteredphase (d8psk.c:219-230) at stream times n, sub-phase c: float32 sum, oldest sample first, then atan2f"""
    from oracle import oracle as O
    taps = MFLT[c::4]
    sr = np.zeros(len(n), np.float32)
    si = np.zeros(len(n), np.float32)
    for j, m in enumerate(taps):
        v = x[n - 16 + j]
        sr = (sr + (v.real * m).astype(np.float32)).astype(np.float32)
        si = (si + (v.imag * m).astype(np.float32)).astype(np.float32)
    at = O.lib().vo_atan2f
    return np.array([at(float(a), float(b)) for a, b in zip(si, sr)], np.float32)


def grey_index(p: np.ndarray, pprev: np.ndarray, df: float) -> np.ndarray:
    d = ((p - pprev).astype(np.float32) - np.float32(df)).astype(np.float32)
    dd = d.astype(np.float64)
    d = np.where(dd > np.pi, (dd - 2 * np.pi).astype(np.float32), d)
    dd = d.astype(np.float64)
    d = np.where(dd < -np.pi, (dd + 2 * np.pi).astype(np.float32), d)
    v = (128.0 * d.astype(np.float64) / np.pi + 128.0).astype(np.float32).astype(np.float64)
    return np.clip(np.floor(v + 0.5), 0, 256).astype(np.int64)      # roundf of a non-negative value


def soft_block(x: np.ndarray, nbrow: int, nlbyte: int, df: float, trig_dec: int, clk0: int, pn: np.ndarray):
    """(hard bytes, reliability map) of one accepted burst: x is the channel's 84 kS/s tap (complex64, x[n] = stream time n)"""
    g = geom(nbrow, nlbyte)
    j0, rb = timing(clk0)
    nbytes = g[4] + g[5]
    kmax = (25 + 8 * nbytes - 1) // 3
    ks = np.arange(7, kmax + 1)
    ph = phases(x, trig_dec + j0 + 8 * ks, rb)
    idx = grey_index(ph[1:], ph[:-1], df)               # symbol k = 8 .. kmax
    q = 25 + np.arange(8 * nbytes)
    k, w = q // 3, q % 3
    i = idx[k - 8]
    v = GREY[w, i]
    v = np.where(pn[q] == 1, (1.0 - v.astype(np.float64)).astype(np.float32), v)
    bits = (v.astype(np.float64) > 0.5).astype(np.uint32).reshape(nbytes, 8)
    byte = (bits << np.arange(8, dtype=np.uint32)).sum(axis=1).astype(np.uint8)
    rbyte = REL[w, i].reshape(nbytes, 8).min(axis=1)
    data = np.zeros((ROWS, ROWLEN), np.uint8)
    rel = np.full((ROWS, ROWLEN), 255, np.uint8)
    for b in range(nbytes):
        r, c = scatter(b, g)
        data[r, c] = byte[b]
        rel[r, c] = rbyte[b]
    return data, rel


def pn_bits(n: int = 25 + 8 * 2100) -> np.ndarray:
    from oracle import oracle as O
    out = np.zeros(n, np.uint8)
    O.lib().vo_pn_bits(out.ctypes.data_as(C.c_void_p), n)
    return out


def channel_maps(raw: np.ndarray, fmt: str, rate: int, fo: int, fc: int, chn: int = 0):
    """[(oracle Block, hard, rel)] for every record of one channel; hard must equal Block.data"""
    from oracle import oracle as O
    ch = O.OracleChannel(rate, fo, fc + fo, chn=chn, tap_dec=True)
    ch.feed(raw, fmt)
    x, trigs, blocks = ch.dec(), ch.triggers(), ch.blocks()
    ch.close()
    clk = {t["dec_index"]: t["clk"] for t in trigs if t["accepted"] == 1}
    pn = pn_bits()
    out = []
    for b in blocks:
        hard, rel = soft_block(x, b.nbrow, b.nlbyte, b.df, b.trig_dec, clk[b.trig_dec], pn)
        out.append((b, hard, rel))
    return out


# ------------------------------------------------------------------------------------------------------------- the row rule
_EXP = np.zeros(512, np.int64)
_LOG = np.zeros(256, np.int64)
_x = 1
for _i in range(255):
    _EXP[_i], _LOG[_x] = _x, _i
    _x <<= 1
    if _x & 0x100:
        _x ^= 0x187
_EXP[255:510] = _EXP[:255]


def syndromes_zero(row: np.ndarray) -> bool:
    """all six syndromes (roots alpha^(120 + i)) of a 255-byte row are zero"""
    for i in range(6):
        s = 0
        for v in row:
            s = (_EXP[(_LOG[s] + 120 + i) % 255] if s else 0) ^ int(v)
        if s:
            return False
    return True


def rs_decode(row: np.ndarray, eras) -> int:
    """rs() (rs.c:81) in place on a uint8 row of 255"""
    from oracle import oracle as O
    buf = (C.c_uint8 * 255).from_buffer(row)
    e = (C.c_int * 6)(*eras)
    return O.lib().vo_rs_decode(buf, e, len(eras))


def row_params(r: int, nbrow: int, nlbyte: int):
    """(data bytes by, fixed erasures, transmitted parity p_r) of row r (vdlm2.c:63-82 set_eras; burst_geom)"""
    by, eras = 249, []
    if r == nbrow - 1:
        by = nlbyte
        if by <= 67:
            eras = [253, 254]
        if by <= 30:
            eras = [251, 252, 253, 254]
    g = geom(nbrow, nlbyte)
    p = 6 if r < g[2] - 1 else (g[3] if r == g[2] - 1 else 0)
    return by, eras, p


def rescue_row(row: np.ndarray, rel: np.ndarray, by: int, eras, p: int, trials=(2, 4)) -> tuple:
    """the row rule on one row: returns (decoded row, how): how = 'ref' (reference decode kept), 's2'/'s4' (rescued), 'fail'"""
    saved = row.copy()
    out = row.copy()
    if rs_decode(out, eras) >= 0:
        return out, "ref"
    cand = list(range(by)) + list(range(249, 249 + p))
    cand.sort(key=lambda c: (int(rel[c]), c))
    for s in trials:
        if len(eras) + s > 4 or s > len(cand):
            continue
        t = saved.copy()
        if rs_decode(t, list(eras) + cand[:s]) >= 0 and syndromes_zero(t):
            return t, f"s{s}"
    return out, "fail"


def row_rule(data: np.ndarray, rel: np.ndarray, nbrow: int, nlbyte: int, trials=(2, 4)):
    """(block after the row rule, per-row outcome)"""
    out = np.array(data, np.uint8).reshape(ROWS, ROWLEN).copy()
    rel = np.asarray(rel, np.uint8).reshape(ROWS, ROWLEN)
    how = []
    for r in range(nbrow):
        by, eras, p = row_params(r, nbrow, nlbyte)
        out[r], h = rescue_row(out[r], rel[r], by, eras, p, trials)
        how.append(h)
    return out, how


def soft_frames(data, rel, nbrow: int, nlbyte: int, trials=(2, 4)):
    """frames of one record in soft mode: the row rule, then the host block path (its rs() leaves a zero-syndrome row as it is)"""
    from oracle import oracle as O
    blk, _ = row_rule(data, rel, nbrow, nlbyte, trials)
    return O.frames_of_block(nbrow, nlbyte, blk.tobytes())
