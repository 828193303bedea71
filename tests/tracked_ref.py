"""numpy restatement of the timing-tracked rows (VDL2GPU_F_TRACKED; the definitions are in include/vdl2gpu.h, vdl2gpu_trk_t) and of the
block path's second attempt, on top of tests/soft_ref.py and tests/feedback_ref.py: the oracle's 84 kS/s tap, the filter, atan2f, slicer,
Grey tables, rs() and frames_of_block as they state them.

    choose(costs)                                        -> index of the winning candidate: a later one only with a strictly smaller cost
    track(idx_of, n, forced=None)                        -> (idx (n,), [d_s]): the segments' choice over idx_of(d, i0, i1)
    phase_at(xz, u)                                      -> P(u) for quarter-sample positions u
    burst_track(x, nbrow, nlbyte, df, end_dec, forced=None) -> (idx, [d_s])
    burst_column(x, nbrow, nlbyte, df, end_dec, pn)      -> dict(data=(8, 255) uint8, d_first, d_last, d_min, d_max, nseg)
    column_bytes(col)                                    -> the 2048 bytes of vdl2gpu_trk_t
    second_attempt(data, trk, fb, rel, nbrow, nlbyte)    -> (frames, report dict or None, taken rows): the rule of attempts A and B
"""
from __future__ import annotations

import numpy as np

import feedback_ref as F
import soft_ref as R

SEG, SEGS = 256, 22
ROW_TRACKED = 7


def choose(costs) -> int:
    best = 0
    for j in range(1, len(costs)):
        if costs[j] < costs[best]:
            best = j
    return best


def cost(idx) -> int:
    e = (np.asarray(idx, np.int64) & 31) - 16
    return int((e * e).sum())


def track(idx_of, n: int, forced=None):
    """idx_of(d, i0, i1): the table indices of symbols i0 .. i1 - 1 (i = k - 8) under hypothesis d.  forced: d for every segment"""
    out = np.zeros(n, np.int64)
    ds = []
    for s in range((n + SEG - 1) // SEG):
        i0, i1 = SEG * s, min(n, SEG * s + SEG)
        cands = [forced] if forced is not None else ([0, -1, -2, -3] if s == 0 else [ds[-1], ds[-1] - 1, ds[-1] + 1])
        idxs = [idx_of(d, i0, i1) for d in cands]
        w = choose([cost(v) for v in idxs])
        ds.append(cands[w])
        out[i0:i1] = idxs[w]
    return out, ds


def phase_at(xz: np.ndarray, u: np.ndarray) -> np.ndarray:
    """P(u): filteredphase at stream time m = ceil(u / 4), sub-phase c = 4 m - u; xz already holds zeros past end_dec"""
    u = np.asarray(u, np.int64)
    m = -((-u) // 4)
    c = 4 * m - u
    out = np.zeros(len(u), np.float32)
    for cc in range(4):
        sel = np.nonzero(c == cc)[0]
        if len(sel):
            out[sel] = R.phases(xz, m[sel], cc)
    return out


def zeroed(x: np.ndarray, end_dec: int) -> np.ndarray:
    """the stream with every sample at a stream time greater than end_dec counting as 0"""
    xz = np.zeros(end_dec + 1 + 64, np.complex64)
    xz[:end_dec + 1] = x[:end_dec + 1]
    return xz


def burst_track(x: np.ndarray, nbrow: int, nlbyte: int, df: float, end_dec: int, forced=None):
    g = R.geom(nbrow, nlbyte)
    kmax = (25 + 8 * (g[4] + g[5]) - 1) // 3
    n = kmax - 7
    xz = zeroed(x, end_dec)
    t = end_dec - 8 * (kmax - np.arange(7, kmax + 1))      # t_7 .. t_kmax

    def idx_of(d, i0, i1):
        ph = phase_at(xz, 4 * t[i0:i1 + 1] + d)            # symbols k - 1 = 7 + i0 .. kmax' : one more in front
        return R.grey_index(ph[1:], ph[:-1], df)

    return track(idx_of, n, forced)


def burst_column(x: np.ndarray, nbrow: int, nlbyte: int, df: float, end_dec: int, pn: np.ndarray, forced=None) -> dict:
    idx, ds = burst_track(x, nbrow, nlbyte, df, end_dec, forced)
    return dict(data=F.rows_of(idx, nbrow, nlbyte, pn), d_first=ds[0], d_last=ds[-1], d_min=min(ds), d_max=max(ds), nseg=len(ds), d=ds)


def column_bytes(col) -> bytes:
    if col is None:
        return bytes(2048)
    tail = np.array([col["d_first"], col["d_last"], col["d_min"], col["d_max"]], np.int8).tobytes() + bytes([col["nseg"], 0, 0, 0])
    return np.asarray(col["data"], np.uint8).tobytes() + tail


def tap_columns(x: np.ndarray, blocks, pn=None):
    pn = R.pn_bits() if pn is None else pn
    return [(b, burst_column(x, b.nbrow, b.nlbyte, b.df, b.end_dec, pn)) for b in blocks]


def channel_columns(raw: np.ndarray, fmt: str, rate: int, fo: int, fc: int, chn: int = 0):
    from oracle import oracle as O
    ch = O.OracleChannel(rate, fo, fc + fo, chn=chn, tap_dec=True)
    ch.feed(raw, fmt)
    x, blocks = ch.dec(), ch.blocks()
    ch.close()
    return tap_columns(x, blocks)


def stream_columns(raw: np.ndarray, fmt: str, rate: int, fo, fc: int, stream: int = 0) -> dict:
    out = {}
    for c, f in enumerate(fo):
        for b, col in channel_columns(raw, fmt, rate, f, fc, c):
            out[(stream, c, b.trig_dec)] = (b, col)
    return out


# ------------------------------------------------------------------------------------------------ the block path's second attempt
def _rec(data) -> np.ndarray:
    return np.array(np.frombuffer(bytes(data), np.uint8) if isinstance(data, (bytes, bytearray)) else data, np.uint8).reshape(R.ROWS, R.ROWLEN)


def second_attempt(data, trk, fb, rel, nbrow: int, nlbyte: int, frames_of=None):
    """(frames, report of the rows, rows taken from trk): attempt A is feedback_ref's row rule (fb, rel as the handle has them) and
    frames_of (default: the reference's block path on the corrected block); attempt B only when A gave nothing and trk is given"""
    from oracle import oracle as O
    frames_of = frames_of or (lambda blk: O.frames_of_block(nbrow, nlbyte, blk.tobytes()))
    rec = _rec(data)
    blkA, howA = F.row_rule(rec, fb, rel, nbrow, nlbyte)
    frA = frames_of(blkA)
    repA = rows_report(rec, blkA, howA, nbrow, nlbyte)
    if frA or trk is None:
        return frA, repA, []
    trk = _rec(trk)
    blkB, howB, taken = blkA.copy(), list(howA), []
    for r in range(nbrow):
        _, eras, _ = R.row_params(r, nbrow, nlbyte)
        t = trk[r].copy()
        if R.rs_decode(t, eras) >= 0 and R.syndromes_zero(t):
            blkB[r] = t
            howB[r] = ROW_TRACKED
            taken.append(r)
    if not taken:
        return frA, repA, []
    frB = frames_of(blkB)
    if frB:
        return frB, rows_report(rec, blkB, howB, nbrow, nlbyte), taken
    return frA, repA, []


def rows_report(rec, out, how, nbrow: int, nlbyte: int) -> dict:
    """the rows' part of vdl2gpu_blockrep_t for the block `out` that the rule made of the received `rec`"""
    roots, changed = [0] * 8, [0] * 8
    for r in range(nbrow):
        by, eras, p = R.row_params(r, nbrow, nlbyte)
        roots[r] = R.rs_decode(rec[r].copy(), eras)
        sent = [j for j in range(255) if j < by or 249 <= j < 249 + p]
        changed[r] = int((out[r][sent] != rec[r][sent]).sum())
    how = list(how) + [F.ROW_NONE] * (8 - nbrow)
    return dict(row_roots=tuple(roots), row_how=tuple(how), row_changed=tuple(changed), bytes_changed=sum(changed),
                rows_failed=how.count(F.ROW_FAIL),
                rows_rescued=sum(h in (F.ROW_SOFT2, F.ROW_SOFT4, F.ROW_FEEDBACK, ROW_TRACKED) for h in how))
