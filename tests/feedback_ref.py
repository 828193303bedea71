"""numpy restatement of the decision-feedback rows (VDL2GPU_F_FEEDBACK; the definitions are in include/vdl2gpu.h), on top of
tests/soft_ref.py: the oracle's 84 kS/s tap, its trigger's clk, the filter, atan2f, slicer, Grey tables and rs() as soft_ref states them.

    recursion(idx)                                       -> (mbar, o, r): the rule on a sequence of table indices, plain integers
    rows_of(idx, nbrow, nlbyte, pn)                      -> (8, 255) uint8: descrambled hard decisions of the indices, scattered like data[]
    burst_rows(x, nbrow, nlbyte, df, trig_dec, clk0, pn) -> (hard rows from idx_k, feedback rows from o_k)
    tap_rows(x, triggers, blocks) / channel_rows(..)     -> [(oracle Block, fb rows)]; asserts hard == Block.data first
    stream_rows(raw, fmt, rate, fo, fc)                  -> {(stream, chn, trig_dec): (Block, fb rows)}
    row_rule(data, fb, rel, nbrow, nlbyte)               -> (block after the row rule of K4Params.fb, how per row)
    report(data, fb, rel, nbrow, nlbyte)                 -> the rows' part of vdl2gpu_blockrep_t under that rule
    fb_frames(data, fb, rel, nbrow, nlbyte)              -> the frames of one record

Every caller that takes phases goes through burst_rows, which forms the hard rows from the same indices without the recursion;
tap_rows holds them against the oracle's Block.data.  That pins the model: an index off by a sector, a symbol or a sample would not
decode the burst."""
from __future__ import annotations

import numpy as np

import soft_ref as R

ROW_NONE, ROW_CLEAN, ROW_REF, ROW_SOFT2, ROW_SOFT4, ROW_FAIL, ROW_FEEDBACK = range(7)


def recursion(idx):
    """(mbar, [o_k], [r_k]) for idx_k, k = 8 .. kmax (Python integers: // and % floor towards minus infinity, as the header asks)"""
    idx = [int(v) for v in idx]
    n = len(idx)
    S = sum((v & 31) - 16 for v in idx)
    mbar = (2 * S + n) // (2 * n)
    r1 = r2 = r3 = 0
    o, rr = [], []
    for v in idx:
        c = 3 * r1 + 2 * r2 + r3
        ok = (v - mbar + (c + 2) // 4) % 256
        rk = ((v - 16 - 32 * (ok >> 5) - mbar + 128) % 256) - 128
        o.append(ok)
        rr.append(rk)
        r1, r2, r3 = rk, r1, r2
    return mbar, o, rr


def rows_of(idx: np.ndarray, nbrow: int, nlbyte: int, pn: np.ndarray) -> np.ndarray:
    """the hard decisions of table indices idx (symbols 8 .. kmax), descrambled, assembled and scattered as the record's data[]"""
    g = R.geom(nbrow, nlbyte)
    nbytes = g[4] + g[5]
    idx = np.asarray(idx, np.int64)
    q = 25 + np.arange(8 * nbytes)
    k, w = q // 3, q % 3
    v = R.GREY[w, idx[k - 8]]
    v = np.where(pn[q] == 1, (1.0 - v.astype(np.float64)).astype(np.float32), v)
    bits = (v.astype(np.float64) > 0.5).astype(np.uint32).reshape(nbytes, 8)
    byte = (bits << np.arange(8, dtype=np.uint32)).sum(axis=1).astype(np.uint8)
    data = np.zeros((R.ROWS, R.ROWLEN), np.uint8)
    for b in range(nbytes):
        r, c = R.scatter(b, g)
        data[r, c] = byte[b]
    return data


def burst_indices(x: np.ndarray, nbrow: int, nlbyte: int, df: float, trig_dec: int, clk0: int) -> np.ndarray:
    g = R.geom(nbrow, nlbyte)
    j0, rb = R.timing(clk0)
    kmax = (25 + 8 * (g[4] + g[5]) - 1) // 3
    ks = np.arange(7, kmax + 1)
    ph = R.phases(x, trig_dec + j0 + 8 * ks, rb)
    return R.grey_index(ph[1:], ph[:-1], df)               # symbol k = 8 .. kmax


def burst_rows(x: np.ndarray, nbrow: int, nlbyte: int, df: float, trig_dec: int, clk0: int, pn: np.ndarray):
    idx = burst_indices(x, nbrow, nlbyte, df, trig_dec, clk0)
    _, o, _ = recursion(idx)
    return rows_of(idx, nbrow, nlbyte, pn), rows_of(o, nbrow, nlbyte, pn)


def tap_rows(x: np.ndarray, triggers, blocks, pn=None):
    clk = {t["dec_index"]: t["clk"] for t in triggers if t["accepted"] == 1}
    pn = R.pn_bits() if pn is None else pn
    out = []
    for b in blocks:
        hard, fb = burst_rows(x, b.nbrow, b.nlbyte, b.df, b.trig_dec, clk[b.trig_dec], pn)
        assert hard.tobytes() == b.data, (b.chn, b.trig_dec)      # the same indices without the recursion are the oracle's bytes
        out.append((b, fb))
    return out


def channel_rows(raw: np.ndarray, fmt: str, rate: int, fo: int, fc: int, chn: int = 0):
    from oracle import oracle as O
    ch = O.OracleChannel(rate, fo, fc + fo, chn=chn, tap_dec=True)
    ch.feed(raw, fmt)
    x, trigs, blocks = ch.dec(), ch.triggers(), ch.blocks()
    ch.close()
    return tap_rows(x, trigs, blocks)


def stream_rows(raw: np.ndarray, fmt: str, rate: int, fo, fc: int, stream: int = 0) -> dict:
    out = {}
    for c, f in enumerate(fo):
        for b, fb in channel_rows(raw, fmt, rate, f, fc, c):
            out[(stream, c, b.trig_dec)] = (b, fb)
    return out


# ------------------------------------------------------------------------------------------------------------- the row rule
def row_rule(data, fb, rel, nbrow: int, nlbyte: int):
    """(block after the row rule, how per row): rel None is hard mode; fb None is soft_ref.row_rule / the reference"""
    rec = np.array(np.frombuffer(bytes(data), np.uint8) if isinstance(data, (bytes, bytearray)) else data, np.uint8).reshape(R.ROWS, R.ROWLEN)
    out = rec.copy()
    fb = None if fb is None else np.asarray(fb, np.uint8).reshape(R.ROWS, R.ROWLEN)
    rel = None if rel is None else np.asarray(rel, np.uint8).reshape(R.ROWS, R.ROWLEN)
    how = []
    for r in range(nbrow):
        by, eras, p = R.row_params(r, nbrow, nlbyte)
        ref = rec[r].copy()
        clean = R.syndromes_zero(ref)
        if R.rs_decode(ref, eras) >= 0:                         # 1. the reference's decode is kept
            out[r] = ref
            how.append(ROW_CLEAN if clean else ROW_REF)
            continue
        if fb is not None:                                      # 2. the feedback row, same fixed erasures
            t = fb[r].copy()
            if R.rs_decode(t, eras) >= 0 and R.syndromes_zero(t):
                out[r] = t
                how.append(ROW_FEEDBACK)
                continue
        if rel is not None:                                     # 3. the soft trials, on the received row
            t, h = R.rescue_row(rec[r].copy(), rel[r], by, eras, p)
            out[r] = t
            how.append({"s2": ROW_SOFT2, "s4": ROW_SOFT4, "fail": ROW_FAIL}[h])
            continue
        out[r] = ref                                            # 4. what the reference left
        how.append(ROW_FAIL)
    return out, how


def report(data, fb, rel, nbrow: int, nlbyte: int) -> dict:
    """row_roots / row_how / row_changed / bytes_changed / rows_failed / rows_rescued as vdl2gpu_blockrep_t defines them with fb given"""
    rec = np.array(np.frombuffer(bytes(data), np.uint8) if isinstance(data, (bytes, bytearray)) else data, np.uint8).reshape(R.ROWS, R.ROWLEN)
    out, how = row_rule(rec, fb, rel, nbrow, nlbyte)
    roots, changed = [0] * 8, [0] * 8
    for r in range(nbrow):
        by, eras, p = R.row_params(r, nbrow, nlbyte)
        roots[r] = R.rs_decode(rec[r].copy(), eras)
        sent = [j for j in range(255) if j < by or 249 <= j < 249 + p]
        changed[r] = int((out[r][sent] != rec[r][sent]).sum())
    how = how + [ROW_NONE] * (8 - nbrow)
    return dict(row_roots=tuple(roots), row_how=tuple(how), row_changed=tuple(changed), bytes_changed=sum(changed),
                rows_failed=how.count(ROW_FAIL), rows_rescued=sum(h in (ROW_SOFT2, ROW_SOFT4, ROW_FEEDBACK) for h in how))


def fb_frames(data, fb, rel, nbrow: int, nlbyte: int):
    """frames of one record under the row rule (the host block path leaves a zero-syndrome row as it is)"""
    from oracle import oracle as O
    blk, _ = row_rule(data, fb, rel, nbrow, nlbyte)
    return O.frames_of_block(nbrow, nlbyte, blk.tobytes())


def scenario_frames(spec, raw, fo, fc, rate=2_000_000, soft=False):
    """One pass over a ber_curve scenario: (sent, hard, feedback, taken, per-record list) with sent / hard / feedback sets of
    (chn, frame), taken the number of rows the rule took from the feedback rows, and records [(Block, fb rows, rel or None)] in
    channel order."""
    from oracle import oracle as O
    from vdlm2dec_amd import synth
    sent = set()
    for b in spec.bursts:
        nbrow, nlbyte, rows = synth.received_rows(b.payload())
        sent.update((b.chan, f) for f in O.frames_of_block(nbrow, nlbyte, rows))
    hard, feed, taken, recs = set(), set(), 0, []
    pn = R.pn_bits()
    for c, f in enumerate(fo):
        ch = O.OracleChannel(rate, f, fc + f, chn=c, tap_dec=True)
        ch.feed(raw, "cs16")
        x, trigs, blocks = ch.dec(), ch.triggers(), ch.blocks()
        ch.close()
        clk = {t["dec_index"]: t["clk"] for t in trigs if t["accepted"] == 1}
        for (b, fb) in tap_rows(x, trigs, blocks, pn):
            rel = R.soft_block(x, b.nbrow, b.nlbyte, b.df, b.trig_dec, clk[b.trig_dec], pn)[1] if soft else None
            hard.update((c, fr) for fr in O.frames_of_block(b.nbrow, b.nlbyte, b.data))
            blk, how = row_rule(b.data, fb, rel, b.nbrow, b.nlbyte)
            taken += how.count(ROW_FEEDBACK)
            feed.update((c, fr) for fr in O.frames_of_block(b.nbrow, b.nlbyte, blk.tobytes()))
            recs.append((b, fb, rel))
    return sent, hard, feed, taken, recs
