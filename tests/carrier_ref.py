"""numpy restatement of the carrier record (VDL2GPU_F_CARRIER; the definitions are in include/vdl2gpu.h), on top of tests/soft_ref.py:
the oracle's 84 kS/s tap, its trigger's clk, the filter, atan2f and slicer as soft_ref states them.

    burst_sums(x, nbrow, nlbyte, df, trig_dec, clk0, pn) -> (hard bytes (8, 255), (nsym, sum_e, sum_e2))
    derived(df, Fr, nsym, sum_e, sum_e2)                 -> (dphi, freq_hz, ppm, rms_rad), float32, by the header's formulas in float64
    channel_sums(raw, fmt, rate, fo, fc, chn)            -> [(oracle Block, (nsym, sum_e, sum_e2))] of one channel
    tap_sums(x, triggers, blocks)                        -> the same from a tap the caller already has

The hard bytes come from the same table indices as the sums; every caller holds them against the oracle's Block.data (channel_sums and
tap_sums do), which is what pins the model: an index off by one sector, symbol or sample would not decode the burst."""
from __future__ import annotations

import numpy as np

import soft_ref as R


def burst_sums(x: np.ndarray, nbrow: int, nlbyte: int, df: float, trig_dec: int, clk0: int, pn: np.ndarray):
    g = R.geom(nbrow, nlbyte)
    j0, rb = R.timing(clk0)
    nbytes = g[4] + g[5]
    kmax = (25 + 8 * nbytes - 1) // 3
    ks = np.arange(7, kmax + 1)
    ph = R.phases(x, trig_dec + j0 + 8 * ks, rb)
    idx = R.grey_index(ph[1:], ph[:-1], df)               # symbol k = 8 .. kmax
    e = (idx & 31) - 16
    sums = (int(kmax - 7), int(e.sum()), int((e * e).sum()))
    # the hard decisions of the same indices (soft_ref.soft_block's, without the reliabilities)
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
    return data, sums


def derived(df, Fr: int, nsym: int, sum_e: int, sum_e2: int):
    """(dphi, freq_hz, ppm, rms_rad) as float32, the formulas of include/vdl2gpu.h in float64"""
    m = np.float64(sum_e) / nsym
    dphi = np.float64(np.float32(df)) + np.pi / 8 + m * np.pi / 128
    var = np.float64(sum_e2) / nsym - m * m
    return (np.float32(dphi), np.float32(10500.0 * dphi / (2 * np.pi)), np.float32(10500.0 * dphi / (2 * np.pi * np.float64(Fr)) * 1e6),
            np.float32(np.sqrt(max(0.0, var)) * np.pi / 128))


def tap_sums(x: np.ndarray, triggers, blocks, pn=None):
    clk = {t["dec_index"]: t["clk"] for t in triggers if t["accepted"] == 1}
    pn = R.pn_bits() if pn is None else pn
    out = []
    for b in blocks:
        hard, sums = burst_sums(x, b.nbrow, b.nlbyte, b.df, b.trig_dec, clk[b.trig_dec], pn)
        assert hard.tobytes() == b.data, (b.chn, b.trig_dec)
        out.append((b, sums))
    return out


def channel_sums(raw: np.ndarray, fmt: str, rate: int, fo: int, fc: int, chn: int = 0):
    from oracle import oracle as O
    ch = O.OracleChannel(rate, fo, fc + fo, chn=chn, tap_dec=True)
    ch.feed(raw, fmt)
    x, trigs, blocks = ch.dec(), ch.triggers(), ch.blocks()
    ch.close()
    return tap_sums(x, trigs, blocks)


def stream_sums(raw: np.ndarray, fmt: str, rate: int, fo, fc: int, stream: int = 0) -> dict:
    """{(stream, chn, trig_dec): (oracle Block, (nsym, sum_e, sum_e2))} of every channel of a stream"""
    out = {}
    for c, f in enumerate(fo):
        for b, sums in channel_sums(raw, fmt, rate, f, fc, c):
            out[(stream, c, b.trig_dec)] = (b, sums)
    return out


# ------------------------------------------------------------------------------------------------------- the physics scenario
RATE = 2_000_000
PHYS_FO = (-350_000, -50_000, 250_000, 550_000)


def physics_spec(cfo=None, seed=7, n=1 << 20):
    """Bursts with known carrier offsets at noise 1.7: 4 channels, 2 MS/s, about 25 bursts.  cfo None: uniform in +-400 Hz (synth's own
    draw); a number: every burst at that offset."""
    from vdlm2dec_amd import synth
    spec = synth.random_scenario(RATE, PHYS_FO, n, seed=seed, bursts_per_s=14.0, info_max=200, noise=1.7)
    if cfo is not None:
        for b in spec.bursts:
            b.cfo = float(cfo)
    return spec


def truth_cfo(spec, chn: int, trig_dec: int) -> float:
    """the offset the burst behind a record was transmitted with: the one burst of the channel that is on the air at the trigger"""
    t = trig_dec / 84000.0
    cands = [b for b in spec.bursts if b.chan == chn and b.t0 <= t <= b.t0 + b.duration()]
    assert len(cands) == 1, (chn, trig_dec, len(cands))
    return cands[0].cfo
