"""The channeliser at every kind of accepted (sdrinrate, sdrclk) pair and device-resident input layout.

vdl2gpu_create accepts any multiple of 25 kHz from 100 kHz on and any SDRCLK in (21, 1e6] whose general-channeliser LDS fits
(include/vdl2gpu.h), and vdl2gpu_push any sample-aligned device pointer and stream stride.  Which of the three K1 kernels runs
depends on exactly these (vdl2gpu.hip, push_impl): k1_fast at SDRCLK 500 with L = 80 only; k1_pp where whole periods of the dump
schedule (4 * SDRCLK inputs) are whole LO tables and whole 16-byte pieces, at a pointer and stride on the 16-byte grid; the general
k1_channelise everywhere else.  Every row below pins the 84 kS/s planes, the bursts and their sample stamps to the oracle at its
SDRCLK, and asserts which kernel ran (timing()["fast_pushes"] counts the k1_fast / k1_pp launches of staged pushes)."""
import numpy as np
import pytest

import scenarios as S
from vdlm2dec_amd import synth

pytestmark = pytest.mark.gpu

BYTES = {"cu8": 2, "cs16": 4, "cf32": 8, "f32": 4}
NP = {"cu8": np.uint8, "cs16": np.int16, "cf32": np.float32, "f32": np.float32}
PER = {"cu8": 2, "cs16": 2, "cf32": 2, "f32": 1}             # array elements per sample
POISON = {"cu8": (0x00, 0xFF), "cs16": (-32767, 32767), "cf32": (-1e30, 1e30), "f32": (-1e30, 1e30)}
GUARD = 4096                                                   # poison bytes (at least) in front of and behind every stream's samples


def _rx(rate, fos, fmt, **kw):
    from vdlm2dec_amd.demod import Receiver, plan_channels
    return Receiver(rate, plan_channels(S.FC, fos), fmt=fmt, **kw)


def _grid(f):
    return int(round(f / 25_000)) * 25_000


def _fos(rate, fmt):
    """a first and a last channel far apart in the band (real input: above the mixer centre, air.c)"""
    if rate == 100_000:
        return (0, 25_000)
    if fmt == "f32":
        return (_grid(0.12 * rate), _grid(0.4 * rate))
    return (_grid(-0.3 * rate), _grid(0.35 * rate))


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _oracle_dec(O, raw, fmt, rate, fo, sdrclk):
    ch = O.OracleChannel(rate, fo, S.FC + fo, tap_dec=True, sdrclk=sdrclk)
    ch.feed(raw, fmt)
    d = ch.dec()
    ch.close()
    return d


def _ragged(per, n, rng):
    """push sizes: whole runs of periods and periods +- a remainder, up to n samples in all"""
    out, pos = [], 0
    while pos < n:
        k = int(rng.choice([4, 5, 6, 9, 13, 64])) * per + int(rng.choice([0, 0, 1, -1, 17, -17, per // 2]))
        k = max(1, min(k, n - pos))
        out.append(k)
        pos += k
    return out


def _check_bursts(O, got, want, sdrclk, frames=None):
    """records equal to the oracle's: keys, trigger / end stamps, df bits, frames; the sample stamps from the decimated ones"""
    key = lambda b: (b.chn, b.end_dec)      # noqa: E731
    got, want = sorted(got, key=key), sorted(want, key=key)
    assert [(b.chn, b.nbrow, b.nlbyte, b.data) for b in got] == [b.key() for b in want]
    assert [(b.trig_dec, b.end_dec) for b in got] == [(b.trig_dec, b.end_dec) for b in want]
    assert [int(np.float32(b.df).view(np.uint32)) for b in got] == [int(np.float32(b.df).view(np.uint32)) for b in want]
    for b in got:
        assert b.trig_sample == ((b.trig_dec + 1) * sdrclk + 20) // 21 - 1, (b.trig_dec, b.trig_sample)
        assert b.end_sample == ((b.end_dec + 1) * sdrclk + 20) // 21 - 1, (b.end_dec, b.end_sample)
    if frames is not None:
        wf = [(0, b.chn, f) for b in sorted(want, key=lambda b: (b.end_dec, b.chn)) for f in O.frames_of_block(b.nbrow, b.nlbyte, b.data)]
        assert sorted(frames) == sorted(wf)


# rate, sdrclk (0 = rate / 4000), format, the K1 kernel that must take whole periods ("pp": k1_pp; "general": k1_channelise only)
MATRIX = [
    (100_000, 0, "cs16", "pp"),             # L = 4 < 32 samples of a chunk, maxwin = 2
    (100_000, 0, "cu8", "general"),         # a period of 100 cu8 samples is 200 bytes: no whole 16-byte pieces
    (1_000_000, 0, "cs16", "pp"),
    (2_025_000, 0, "cs16", "general"),      # SDRCLK 506.25 -> 506; 4 * 506 = 2024 is no whole number of L = 81
    (2_400_000, 0, "cu8", "pp"),
    (2_500_000, 0, "cu8", "general"),       # 2500 cu8 samples = 5000 bytes
    (2_500_000, 0, "cs16", "pp"),           # ... the same rate in cs16: 10000 bytes
    (3_000_000, 0, "f32", "pp"),            # real input
    (8_000_000, 0, "cs16", "pp"),
    (2_000_000, 400, "cs16", "pp"),         # custom SDRCLK: 1600 = 20 LO tables
    (2_000_000, 510, "cs16", "general"),    # 2040 is no whole number of 80
    (2_000_000, 22, "cs16", "general"),     # the smallest SDRCLK: maxwin = 2, 88 = 1.1 LO tables
    (25_700_000, 0, "cs16", "pp"),          # the LDS ceiling: k1_channelise at 163 712 bytes for the edges of a push
]


def _row_input(rate, sdrclk, fmt):
    fos = _fos(rate, fmt)
    infos = (3, 40) if rate > 10_000_000 else (3, 40, 120, 17)
    spec = S.regimes(rate=rate, fo=fos, seed=rate // 1000 + sdrclk, infos=infos, gap=0.001)
    return spec, synth.synth_stream(spec, fmt)


@pytest.mark.timeout(240)
@pytest.mark.parametrize("rate,sdrclk,fmt,path", MATRIX, ids=[f"{r // 1000}k-{c or 'def'}-{f}" for r, c, f, _ in MATRIX])
def test_rate_matrix(built, oracle, monkeypatch, rate, sdrclk, fmt, path):
    clk = sdrclk or rate // 4000
    per = 4 * clk
    spec, raw = _row_input(rate, sdrclk, fmt)
    n = raw.size // PER[fmt]
    fos = spec.fo
    assert n >= 16 * per
    want = oracle.run_oracle(raw, fmt, rate, fos, S.FC, sdrclk=sdrclk)
    if sdrclk == 0:
        assert len(want) >= 2            # the bursts decode at the default SDRCLK: the comparison below has something to compare
    decs = {c: _oracle_dec(oracle, raw, fmt, rate, fos[c], sdrclk) for c in (0, len(fos) - 1)}
    monkeypatch.setenv("VDL2GPU_STAGE_EVERY", "1")          # every push is timed: fast_pushes counts every fast launch
    monkeypatch.delenv("VDL2GPU_NO_K1_FAST", raising=False)

    # one whole push
    with _rx(rate, fos, fmt, sdrclk=sdrclk, max_push=n, keep_dec=True, frames=True) as rx:
        rx.push(raw)
        for c, d in decs.items():
            g = rx.debug_dec(0, c)
            assert len(g) == len(d) and np.array_equal(_bits(g), _bits(d)), ("whole", c)
        _check_bursts(oracle, rx.poll(), want, clk, rx.poll_frames())
        fast = rx.timing()["fast_pushes"]
    assert (fast > 0) == (path == "pp"), fast

    # ragged pushes: whole periods and periods +- remainders, so that carried windows meet whole pushes
    sizes = _ragged(per, n, np.random.default_rng(rate + sdrclk))
    with _rx(rate, fos, fmt, sdrclk=sdrclk, max_push=max(sizes), keep_dec=True) as rx:
        parts, got, pos = {c: [] for c in decs}, [], 0
        for k in sizes:
            rx.push(raw[PER[fmt] * pos:PER[fmt] * (pos + k)])
            for c in decs:
                parts[c].append(rx.debug_dec(0, c))
            got += rx.poll_ready()
            pos += k
        got += rx.poll()
        fast = rx.timing()["fast_pushes"]
    for c, d in decs.items():
        g = np.concatenate(parts[c])
        assert len(g) == len(d) and np.array_equal(_bits(g), _bits(d)), ("ragged", c)
    _check_bursts(oracle, got, want, clk)
    assert (fast > 0) == (path == "pp"), fast

    # the same planes with the period-parallel kernels switched off: the general kernel alone
    monkeypatch.setenv("VDL2GPU_NO_K1_FAST", "1")
    with _rx(rate, fos, fmt, sdrclk=sdrclk, max_push=n, keep_dec=True) as rx:
        rx.push(raw)
        for c, d in decs.items():
            g = rx.debug_dec(0, c)
            assert len(g) == len(d) and np.array_equal(_bits(g), _bits(d)), ("general", c)
        assert rx.timing()["fast_pushes"] == 0
        _check_bursts(oracle, rx.poll(), want, clk)


# ------------------------------------------------------------------------------------------------ device-resident layouts
# rate, format, the kernel that takes whole periods of a 16-byte-grid push
LAYOUTS = [
    (2_000_000, "cu8", "k1_fast"), (2_000_000, "cs16", "k1_fast"), (2_000_000, "cf32", "k1_fast"),
    (5_000_000, "f32", "k1_pp"), (10_000_000, "cs16", "k1_pp"), (2_025_000, "cs16", "general"),
]


def _poison(fmt, buf, lo, hi, front):
    v = np.dtype(NP[fmt])
    buf[lo:hi].view(v)[:] = POISON[fmt][0 if front else 1]


def _device_pushes(fmt, streams, sizes, off, stride_pad):
    """per push one allocation: [GUARD + off poison][stream 0][2 GUARD poison][stream 1] ... [stream 2][GUARD poison], the streams
    stride bytes apart (a multiple of 16 plus stride_pad); returns [(tensor, pointer of stream 0's first sample, stride)]"""
    import torch
    B = BYTES[fmt]
    out, pos = [], 0
    for k in sizes:
        nb = k * B
        stride = (nb + 2 * GUARD + 15) // 16 * 16 + stride_pad
        head = GUARD + off * B
        total = head + (len(streams) - 1) * stride + nb + GUARD
        host = np.zeros((total + 15) // 16 * 16, np.uint8)
        _poison(fmt, host, 0, head, True)
        for s, raw in enumerate(streams):
            a = head + s * stride
            host[a:a + nb] = np.ascontiguousarray(raw[PER[fmt] * pos:PER[fmt] * (pos + k)]).view(np.uint8)
            _poison(fmt, host, a + nb, a + stride if s + 1 < len(streams) else total, False)
            if s + 1 < len(streams):
                # the gap before the next stream's samples: GUARD bytes or more of back poison, then as much front poison
                mid = a + nb + (stride - nb) // 2 // B * B
                _poison(fmt, host, mid, a + stride, True)
        t = torch.from_numpy(host).to("cuda:0")
        out.append((t, t.data_ptr() + head, stride))
        pos += k
    torch.cuda.synchronize()
    return out


@pytest.mark.timeout(300)
@pytest.mark.parametrize("rate,fmt,path", LAYOUTS, ids=[f"{r // 1000}k-{f}-{p}" for r, f, p in LAYOUTS])
def test_device_input_at_every_offset_and_stride(built, oracle, monkeypatch, rate, fmt, path):
    """Three streams of device-resident samples, each push in its own allocation with poison around every stream: the push
    starts at every whole-sample offset from a 16-byte boundary and at a large odd one; the first push is a whole run of periods
    (superperiods at 2 MS/s), which a pointer off the grid sends through the re-basing branch of the k1_pp set-up, the rest are
    ragged.  Stream strides on the 16-byte grid keep the period-parallel kernels; strides off it must turn them off.  A kernel
    that reads a sample outside what was pushed reads poison, and the planes differ."""
    B = BYTES[fmt]
    clk = rate // 4000
    per = 4 * clk
    fos = _fos(rate, fmt)
    sizes = [per * 16, per * 13 + 7, per * 6 - 5, per * 9 + 1, per * 4]
    n = sum(sizes)
    rng = np.random.default_rng(rate // 1000 + B)
    if fmt == "cu8":
        streams = [rng.integers(0, 256, 2 * n, dtype=np.uint8) for _ in range(3)]
    elif fmt == "cs16":
        streams = [rng.integers(-3000, 3000, 2 * n, dtype=np.int16) for _ in range(3)]
    else:
        streams = [rng.normal(0, 20, PER[fmt] * n).astype(np.float32) for _ in range(3)]
    want = {(s, c): _oracle_dec(oracle, streams[s], fmt, rate, fos[c], 0) for s in range(3) for c in (0, 1)}
    monkeypatch.setenv("VDL2GPU_STAGE_EVERY", "1")
    offsets = list(range(16 // B)) + [4099]
    cases = [(off, 0) for off in offsets] + [(0, B), (offsets[-1], B), (1, B)]     # stride_pad = B: a stride off the grid
    from vdlm2dec_amd.demod import Receiver, plan_channels
    for off, pad in cases:
        bufs = _device_pushes(fmt, streams, sizes, off, pad)
        assert all((p - GUARD - off * B) % 16 == 0 for _, p, _ in bufs)
        with Receiver(rate, [plan_channels(S.FC, fos)] * 3, fmt=fmt, max_push=max(sizes), keep_dec=True) as rx:
            parts = {k: [] for k in want}
            for (t, p, stride), k in zip(bufs, sizes):
                rx.push_device(p, k, stride)
                for s, c in want:
                    parts[(s, c)].append(rx.debug_dec(s, c))
            rx.poll()
            fast = rx.timing()["fast_pushes"]
        for (s, c), d in want.items():
            g = np.concatenate(parts[(s, c)])
            assert len(g) == len(d) and np.array_equal(_bits(g), _bits(d)), (off, pad, s, c)
        assert (fast > 0) == (path != "general" and pad == 0), (off, pad, fast)
        del bufs


# ---------------------------------------------------------------------------------------------------- options at 2.4 MS/s
@pytest.mark.timeout(240)
def test_levels_soft_maps_and_frames_at_2400k(built, oracle):
    import test_gpu_levels as TL
    import soft_ref as R
    rate, fmt = 2_400_000, "cu8"
    spec = S.regimes(rate=rate, fo=(-600_000, 850_000), seed=241, infos=(2, 31, 66, 120, 250, 7))
    raw = synth.synth_stream(spec, fmt)
    want = oracle.run_oracle(raw, fmt, rate, spec.fo, S.FC)
    maps = {}
    for c, fo in enumerate(spec.fo):
        for b, hard, rel in R.channel_maps(raw, fmt, rate, fo, S.FC, c):
            assert hard.tobytes() == b.data
            maps[(c, b.trig_dec)] = rel
    assert len(want) >= 5
    with _rx(rate, spec.fo, fmt, max_push=spec.nsamples, keep_dec=True, levels=True, soft_rs=True, frames=True) as rx:
        rx.push(raw)                    # one push: the levels are checked on the planes debug_dec() returns, those of the last push
        got = rx.poll()
        frames = rx.poll_frames()
        _check_bursts(oracle, got, want, rate // 4000, frames)
        TL._check_exact(rx, got, spec, fmt)
        for b in got:
            assert b.soft is not None and np.array_equal(b.soft, maps[(b.chn, b.trig_dec)]), (b.chn, b.trig_dec)
