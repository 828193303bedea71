"""Yardstick for VDL2GPU_F_EXACT_FO (tests/test_exact_fo.py, tests/test_gpu_exact_fo.py): channel offsets off the 25 kHz grid.

channelise()   the definition of include/vdl2gpu.h in numpy float32: offgrid_model.channelise with the table of the grid point
               Fg next to Fo, then every output rotated by r_m = T_hi[k_m >> 12] (x) T_lo[k_m & 4095], k_m from the window bounds of
               offgrid_model.window_ends in Python integers, the tables from vdl2gpu_exact_fo_tables; (x) rounds each product and
               each sum on its own.  A channel with Fd == 0 is offgrid_model.channelise's plane, untouched.
ROWS           the scenarios both test files run: one short burst per channel, seeds with which every channel decodes."""
import numpy as np

import offgrid_model as M
import scenarios as S
from vdlm2dec_amd import demod, synth

# rate, format, channel offsets in Hz
ROWS = [
    (2_000_000, "cs16", (-295_900, 12_500, 237_500, 100_000)),     # k1_fast; the last channel lies on the grid
    (2_048_000, "cu8", (-195_900, 312_500)),                       # k1_pp; the general kernel with its table in LDS
    (10_000_000, "cs16", (-2_987_500, 1_004_100)),                 # k1_pp
    (15_360_000, "cs16", (4_100,)),                                # the general kernel with its table in global memory
    (3_000_000, "f32", (362_500, 1_204_100)),                      # real input, k1_pp
    (100_000, "cs16", (12_500, -24_999)),                          # nf in {1, 2}: the smallest window
]
IDS = [f"{r // 1000}k-{f}" for r, f, _ in ROWS]
PER = {"cu8": 2, "cs16": 2, "cf32": 2, "f32": 1, "cs8": 2, "s16": 1}
# seeds of the rows' recordings: every channel decodes a CRC-clean frame through the model, none through the jumping table
# on the channels with Fd = +-12500 (tests/test_exact_fo.py::test_rows_decode_with_the_flag_and_not_without checks both)
SEEDS = {2_000_000: 2, 2_048_000: 1, 10_000_000: 1, 15_360_000: 1, 3_000_000: 1, 100_000: 1}


def split(fo):
    """(Fg, Fd): Fg = 25000 * floor((Fo + 12500) / 25000), Fd = Fo - Fg in [-12500, 12500)"""
    fg = 25_000 * ((fo + 12_500) // 25_000)
    return fg, fo - fg


def cmul(x, y):
    """(xr yr - xi yi, xr yi + xi yr) on complex64 arrays, every float32 operation rounded on its own"""
    xr, xi, yr, yi = (np.asarray(v, np.float32) for v in (x.real, x.imag, y.real, y.imag))
    out = np.empty(np.broadcast(xr, yr).shape, np.complex64)
    out.real = xr * yr - xi * yi
    out.imag = xr * yi + xi * yr
    return out


def indices(n, rate, fd, sdrclk=0, first=0):
    """k_m of every output that completes within n inputs, in Python integers; the n inputs are samples first .. first + n - 1 of the
    stream, where `first` is a sample at which the dump schedule begins anew (a multiple of SDRCLK)"""
    sdrclk = sdrclk or rate // 4000
    assert first % sdrclk == 0
    ends = [int(e) for e in M.window_ends(n, sdrclk, demod._lib.load().vdl2gpu_lo_len(rate))]
    starts = [0] + [e + 1 for e in ends[:-1]]
    m2 = 2 * rate
    f = fd % m2
    return np.array([(f * ((a + e + 2 * first) % m2)) % m2 for a, e in zip(starts, ends)], np.int64)


def rotate(plane, n, rate, fd, sdrclk=0, first=0):
    if fd == 0:
        return plane
    hi, lo = demod.exact_fo_tables(rate)
    k = indices(n, rate, fd, sdrclk, first)
    assert len(k) == len(plane)
    return cmul(plane, cmul(hi[k >> 12], lo[k & 4095]))


def channelise(raw, fmt, rate, fo, sdrclk=0, first=0):
    """the 84 kS/s plane of one channel of a handle with VDL2GPU_F_EXACT_FO; first: the stream index of raw's first sample, a multiple
    of the schedule's period and of the mixer's table (the mixer and the dump are then those of a stream that begins there)"""
    fg, fd = split(fo)
    assert first % (sdrclk or rate // 4000) == 0 and first % demod._lib.load().vdl2gpu_lo_len(rate) == 0
    return rotate(M.channelise(raw, fmt, rate, fg, sdrclk), np.asarray(raw).size // PER[fmt], rate, fd, sdrclk, first)


def scenario(rate, fmt, fos, seed=None):
    infos = (3, 40, 9, 28)[:max(len(fos), 1)]
    spec = S.regimes(rate=rate, fo=fos, seed=SEEDS[rate] if seed is None else seed, infos=infos, gap=0.001)
    return spec, synth.synth_stream(spec, fmt)


def sent_frames(spec):
    """per channel, the AVLC frames synth transmitted"""
    out = [[] for _ in spec.fo]
    for b in spec.bursts:
        out[b.chan].append(synth.avlc_frame(b.info, src=(1 << 24) | (0x400000 + b.chan * 0x111 + len(b.info))))
    return out


def frames_of(O, blocks):
    return [f for b in sorted(blocks, key=lambda b: b.end_dec) for f in O.frames_of_block(b.nbrow, b.nlbyte, b.data)]


_cache = {}


def expected(O, row):
    """planes, the demodulator-only oracle's records over them and their frames, per channel of a row; computed once"""
    if row not in _cache:
        rate, fmt, fos = ROWS[row]
        spec, raw = scenario(rate, fmt, fos)
        planes = [channelise(raw, fmt, rate, fo) for fo in fos]
        blocks = [M.demod_blocks(O, p, S.FC + fo, chn=c) for c, (p, fo) in enumerate(zip(planes, fos))]
        for p in planes:
            p.setflags(write=False)
        _cache[row] = {"spec": spec, "raw": raw, "planes": planes, "blocks": blocks, "frames": [frames_of(O, b) for b in blocks]}
    return _cache[row]
