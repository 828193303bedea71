"""Yardsticks for sample rates off the 25 kHz grid (tests/test_offgrid_rates.py, tests/test_gpu_offgrid_rates.py).

The oracle takes its LO table as SDRINRATE / 25000 entries, which is no whole period of the oscillator off the grid, so it cannot
judge an off-centre channel there.  Two pieces replace it, each pinned to the oracle where the oracle is valid (test_offgrid_rates.py):

channelise()   a numpy float32 restatement of the mixer and the integrate-and-dump (d8psk.c:366-381): every product and every sum
               rounded on its own, in stream order; the table from vdl2gpu_lo_table, the schedule from vdl2gpu_plan.
demod_blocks() the oracle itself behind the channeliser: created at 84 kS/s with SDRCLK 21 and Fo = 0 it dumps every sample it is
               fed unchanged (nf = 1, LO = 1 - 0j), so a channel's 84 kS/s plane fed as cf32 runs through its demodulator alone."""
import numpy as np

from vdlm2dec_amd import demod

REAL = ("f32", "s16")


def to_float(raw, fmt):
    """raw samples -> (re, im) float32 as the channeliser's ingest converts them (im None for real input)"""
    if fmt == "cu8":
        v = np.asarray(raw, np.uint8).astype(np.float32) - np.float32(127.37)
    elif fmt in ("cs16", "s16"):
        v = np.asarray(raw, np.int16).astype(np.float32)
    elif fmt == "cs8":
        v = np.asarray(raw).view(np.int8).astype(np.float32)
    else:
        v = np.asarray(raw, np.float32)
    return (v, None) if fmt in REAL else (v[0::2].copy(), v[1::2].copy())


def oracle_input(raw, fmt):
    """(array, format) the oracle accepts for the same sample values: cs8 and s16 as the floats they convert to, exactly"""
    if fmt == "cs8":
        return np.asarray(raw).view(np.int8).astype(np.float32), "cf32"
    if fmt == "s16":
        return np.asarray(raw, np.int16).astype(np.float32), "f32"
    return raw, fmt


def window_ends(n, sdrclk, lo_len):
    """index of the last input of every output that completes within n inputs from the start of the stream"""
    c0, _, _, nout = demod.plan(0, n, sdrclk, lo_len)
    assert c0 == 0
    j = np.arange(nout, dtype=np.int64)
    ends = ((j + 1) * sdrclk + 20) // 21 - 1
    for k in ([0, 1, nout // 2, nout - 2] if nout > 3 else []):       # the closed form is vdl2gpu_plan's: an output ends where
        c, no0, nf0, _ = demod.plan(int(ends[k]) + 1, 0, sdrclk, lo_len)   # the next window has consumed nothing
        assert nf0 == 0 and c < 21 and no0 == (int(ends[k]) + 1) % lo_len, (k, c, nf0)
        assert demod.plan(int(ends[k]), 0, sdrclk, lo_len)[2] == ends[k] - (ends[k - 1] + 1 if k else 0)
    return ends


def channelise(raw, fmt, rate, fo, sdrclk=0):
    """the 84 kS/s plane of one channel: complex64, one entry per completed output"""
    sdrclk = sdrclk or rate // 4000
    w = demod.lo_table(rate, fo)
    xr, xi = to_float(raw, fmt)
    n = len(xr)
    ends = window_ends(n, sdrclk, len(w))
    idx = np.arange(n, dtype=np.int64) % len(w)
    wr, wi = w.real[idx], w.imag[idx]
    if xi is None:
        pr, pi = xr * wr, xr * wi
    else:
        pr = xr * wr - xi * wi          # numpy rounds each float32 operation on its own
        pi = xr * wi + xi * wr
    starts = np.concatenate([[0], ends[:-1] + 1])
    lens = ends - starts + 1
    dre, dim = np.zeros(len(ends), np.float32), np.zeros(len(ends), np.float32)
    for t in range(int(lens.max()) if len(lens) else 0):
        m = lens > t
        dre[m] += pr[starts[m] + t]
        dim[m] += pi[starts[m] + t]
    nf = lens.astype(np.float32)
    out = np.empty(len(ends), np.complex64)
    out.real, out.imag = dre / nf, dim / nf
    return out


def demod_blocks(O, plane, fr, chn=0):
    """the oracle's burst records for one 84 kS/s plane"""
    ch = O.OracleChannel(84_000, 0, fr, chn=chn, sdrclk=21)
    ch.feed(np.ascontiguousarray(plane, np.complex64).view(np.float32), "cf32")
    b = ch.blocks()
    ch.close()
    return b


def block_fields(b):
    return (b.chn, b.nbrow, b.nlbyte, int(np.float32(b.df).view(np.uint32)), int(np.float32(b.ppm).view(np.uint32)), b.trig_dec, b.end_dec, b.data)


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)
