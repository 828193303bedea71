"""The stream epoch of the test build (VDL2GPU_TEST_EPOCH, include/vdl2gpu.h) in Python integers: which T0 a handle accepts, how far
it moves every stamp, and how a test chooses the T0 that puts a boundary of the time axis inside a burst (CPU only, no GPU import).

A handle created with epoch T0 begins as if T0 input samples per stream had already been pushed and had left the canonical start
state behind: the stream is exactly shift-invariant only where the dump schedule (16 SDRCLK inputs = 336 outputs), the LO table and
-- with VDL2GPU_F_RTL_QUIRK -- the 32768-sample hand-off blocks all begin anew, and the residual oscillator of VDL2GPU_F_EXACT_FO
only every 2 SDRINRATE inputs."""
from __future__ import annotations

from math import gcd

EINVAL = -1
BOUNDARIES = {"in31": ("in", 1 << 31), "in32": ("in", 1 << 32), "dec31": ("dec", 1 << 31), "dec32": ("dec", 1 << 32),
              "big40": ("in", 1 << 40)}        # big40: nothing crosses, the epoch is the first admissible one from 2^40 on


def lcm(*v):
    out = 1
    for x in v:
        out = out * x // gcd(out, x)
    return out


def lo_len(rate):
    from vdlm2dec_amd import lib
    return int(lib.load().vdl2gpu_lo_len(rate))


def quantum(rate, sdrclk=0, quirk=False, pure_shift=False):
    """every admissible T0 is a multiple of this; pure_shift: the T0 at which an exact-Fo handle is shift-invariant as well"""
    clk = sdrclk or rate // 4000
    return lcm(16 * clk, lo_len(rate), 32768 if quirk else 1, 2 * rate if pure_shift else 1)


def admissible(t0, rate, sdrclk=0, quirk=False):
    return 0 <= t0 <= 1 << 56 and t0 % quantum(rate, sdrclk, quirk) == 0


def d0(t0, clk):
    """84 kS/s frames completed within t0 input samples: exact at an admissible T0 (21 T0 / SDRCLK is whole)"""
    assert (21 * t0) % clk == 0
    return 21 * t0 // clk


def dec_to_sample(m, clk):
    """index of the input sample that completes frame m (include/vdl2gpu.h: trig_sample, end_sample)"""
    return ((m + 1) * clk + 20) // 21 - 1


def epoch_for(boundary, trig_dec, clk, q):
    """the largest admissible T0 at which `boundary` = (axis, value) lies behind the trigger of the burst that the oracle, from
    sample 0, triggers at frame trig_dec; big40: the first one from the value on"""
    axis, value = boundary
    if value == 1 << 40:
        return -(-value // q) * q
    if axis == "in":
        return (value - dec_to_sample(trig_dec, clk) - 1) // q * q
    qd = d0(q, clk)
    return (value - trig_dec - 1) // qd * qd * clk // 21


def crossing(boundary, t0, clk, blocks):
    """(before, across, after): the oracle's blocks that end before the boundary, that are in flight across it (trigger before, last
    symbol at or after it) and that trigger at or after it, at epoch t0"""
    axis, value = boundary
    pos = (lambda m: t0 + dec_to_sample(m, clk)) if axis == "in" else (lambda m: d0(t0, clk) + m)
    before = [b for b in blocks if pos(b.end_dec) < value]
    across = [b for b in blocks if pos(b.trig_dec) < value <= pos(b.end_dec)]
    after = [b for b in blocks if pos(b.trig_dec) >= value]
    return before, across, after
