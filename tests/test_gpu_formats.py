"""VDL2GPU_FMT_CS8 (interleaved signed 8-bit I,Q) and VDL2GPU_FMT_S16R (real signed 16-bit) on the GPU.

An integer sample converts to float without rounding, so a handle fed one of the two formats must produce bit for bit what the
oracle -- the CPU restatement of the reference -- produces from the same values handed to it as cf32 / f32 (the "float twin"): the
84 kS/s planes, the bursts, their stamps, levels and soft maps.  tests/test_fmt_abi.py shows on the CPU that the oracle decodes
every burst of the streams used here, so every comparison below demands the full count."""
import ctypes as C
import math

import numpy as np
import pytest

import scenarios as S
from test_gpu_rates import GUARD, _bits, _check_bursts, _fos, _oracle_dec, _ragged
from vdlm2dec_amd import lib, synth

pytestmark = pytest.mark.gpu

TWIN = {"cs8": "cf32", "s16": "f32"}                 # the float format that carries the same values
NP = {"cs8": np.int8, "s16": np.int16}
PER = {"cs8": 2, "s16": 1}                           # array elements per sample
BYTES = 2                                            # bytes per sample, both
POISON = {"cs8": (-128, 127), "s16": (-32767, 32767)}
FS = {"cs8": 128.0, "s16": 32768.0}                  # include/vdl2gpu.h, "scale:"


def _rx(rate, fos, fmt, **kw):
    from vdlm2dec_amd.demod import Receiver, plan_channels
    return Receiver(rate, plan_channels(S.FC, fos), fmt=fmt, **kw)


def _twin(raw):
    return np.ascontiguousarray(raw).astype(np.float32)          # exact: |v| <= 32768


def _planes_equal(rx, decs, tag, stream=0):
    for c, d in decs.items():
        g = rx.debug_dec(stream, c)
        assert len(g) == len(d) and np.array_equal(_bits(g), _bits(d)), (tag, c)


def _check(oracle, got, want, clk, frames=None):
    """test_gpu_rates' record check (keys, stamps, df bits, frames) and the ppm bits"""
    _check_bursts(oracle, got, want, clk, frames)
    key = lambda b: (b.chn, b.end_dec)      # noqa: E731
    assert [int(np.float32(b.ppm).view(np.uint32)) for b in sorted(got, key=key)] == \
           [int(np.float32(b.ppm).view(np.uint32)) for b in sorted(want, key=key)]


# rate, format, the K1 kernel that must take the whole periods of a push.  With 2-byte samples a period of 4 * SDRCLK samples
# is whole 16-byte pieces at 2.4, 5 and 10 MS/s (as for cu8) and is not at 2.5 MS/s (5000 bytes); at 2.025 MS/s a period is no
# whole number of LO tables whatever the format.
ROWS = [
    (2_000_000, "cs8", "k1_fast"), (2_400_000, "cs8", "k1_pp"), (10_000_000, "cs8", "k1_pp"),
    (2_500_000, "cs8", "general"), (2_025_000, "cs8", "general"),
    (2_000_000, "s16", "k1_fast"), (5_000_000, "s16", "k1_pp"),
    (2_500_000, "s16", "general"), (2_025_000, "s16", "general"),
]


def _row_input(rate, fmt):
    fos = _fos(rate, TWIN[fmt])         # real input: channels above the mixer centre
    spec = S.regimes(rate=rate, fo=fos, seed=rate // 1000 + (7 if fmt == "s16" else 0), infos=(3, 40, 120, 17), gap=0.001)
    return spec, synth.synth_stream(spec, fmt)


@pytest.mark.timeout(240)
@pytest.mark.parametrize("rate,fmt,path", ROWS, ids=[f"{r // 1000}k-{f}-{p}" for r, f, p in ROWS])
def test_parity_at_every_kernel(built, oracle, monkeypatch, rate, fmt, path):
    clk = rate // 4000
    per = 4 * clk
    spec, raw = _row_input(rate, fmt)
    assert raw.dtype == NP[fmt]
    n = raw.size // PER[fmt]
    fos = spec.fo
    tw = _twin(raw)
    want = oracle.run_oracle(tw, TWIN[fmt], rate, fos, S.FC)
    assert len(want) == len(spec.bursts) == 4           # every burst sent
    decs = {c: _oracle_dec(oracle, tw, TWIN[fmt], rate, fos[c], 0) for c in (0, len(fos) - 1)}
    monkeypatch.setenv("VDL2GPU_STAGE_EVERY", "1")      # every push is timed: fast_pushes counts every k1_fast / k1_pp launch
    for k in ("VDL2GPU_NO_K1_FAST", "VDL2GPU_K1_PP"):
        monkeypatch.delenv(k, raising=False)

    # one whole push
    with _rx(rate, fos, fmt, max_push=n, keep_dec=True, frames=True) as rx:
        rx.push(raw)
        _planes_equal(rx, decs, "whole")
        _check(oracle, rx.poll(), want, clk, rx.poll_frames())
        fast = rx.timing()["fast_pushes"]
    assert (fast > 0) == (path != "general"), fast

    # ragged pushes: whole periods and periods +- remainders
    sizes = _ragged(per, n, np.random.default_rng(rate + BYTES))
    with _rx(rate, fos, fmt, max_push=max(sizes), keep_dec=True) as rx:
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
    _check(oracle, got, want, clk)
    assert (fast > 0) == (path != "general"), fast

    # the same stream on the other kernels that can take it: the general one alone, and at 2 MS/s k1_pp in k1_fast's place
    monkeypatch.setenv("VDL2GPU_NO_K1_FAST", "1")
    with _rx(rate, fos, fmt, max_push=n, keep_dec=True) as rx:
        rx.push(raw)
        _planes_equal(rx, decs, "general")
        assert rx.timing()["fast_pushes"] == 0
        _check(oracle, rx.poll(), want, clk)
    monkeypatch.delenv("VDL2GPU_NO_K1_FAST")
    if path == "k1_fast":
        monkeypatch.setenv("VDL2GPU_K1_PP", "1")
        with _rx(rate, fos, fmt, max_push=n, keep_dec=True) as rx:
            rx.push(raw)
            _planes_equal(rx, decs, "k1_pp at 2 MS/s")
            assert rx.timing()["fast_pushes"] > 0
            _check(oracle, rx.poll(), want, clk)


# --------------------------------------------------------------------------------------------------------------- twin handles
def _poll_all(rx, n=4096):
    buf, lv, sv = (lib.BurstT * n)(), (lib.LevelT * n)(), (lib.SoftT * n)()
    k = rx.poll_soft_raw(buf, lv, sv, n)
    assert k < n
    return buf, lv, sv, k


@pytest.mark.timeout(300)
@pytest.mark.parametrize("fmt,rate,fo,sent", [("cs8", 2_000_000, S.FO8, 16), ("s16", 5_000_000, S.FO8_AIR_5MS, 16)])
def test_twin_handles(built, fmt, rate, fo, sent):
    """The same values pushed as cs8 / s16 and, widened on the host, as cf32 / f32: identical planes, records byte for byte, level
    powers and soft maps; the dBFS figures differ by the full scale alone (cf32 / f32: FS = 1)."""
    spec = S.eight_channels(rate=rate, fo=fo)
    raw = synth.synth_stream(spec, fmt)
    res = []
    for f, r in ((fmt, raw), (TWIN[fmt], _twin(raw))):
        with _rx(rate, spec.fo, f, max_push=spec.nsamples, keep_dec=True, levels=True, soft_rs=True, frames=True) as rx:
            rx.push(r)
            buf, lv, sv, k = _poll_all(rx)
            res.append(dict(k=k, recs=bytes(C.string_at(C.addressof(buf), k * C.sizeof(lib.BurstT))),
                            soft=bytes(C.string_at(C.addressof(sv), k * C.sizeof(lib.SoftT))),
                            lv=[(v.sig_dbfs, v.noise_dbfs, v.sig_power, v.noise_power, v.sym_first_dec, v.nsym, v.subphase,
                                 v.noise_blocks) for v in lv[:k]],
                            planes=[_bits(rx.debug_dec(0, c)) for c in range(8)], frames=rx.poll_frames()))
    a, b = res
    assert a["k"] == b["k"] == sent == len(spec.bursts)
    for c in range(8):
        assert np.array_equal(a["planes"][c], b["planes"][c]), c
    assert a["recs"] == b["recs"] and a["soft"] == b["soft"] and a["frames"] == b["frames"]
    assert len(a["frames"]) > 0
    off = 20.0 * math.log10(FS[fmt])
    f32b = lambda v: int(np.float32(v).view(np.uint32))      # noqa: E731
    for x, y in zip(a["lv"], b["lv"]):
        assert x[4:] == y[4:] and x[5] > 0                  # sym_first_dec, nsym, subphase, noise_blocks
        assert f32b(x[2]) == f32b(y[2])                     # sig_power
        assert math.isclose(x[0], y[0] - off, abs_tol=1e-4), (x, y)
        if x[7]:
            assert f32b(x[3]) == f32b(y[3])
            assert math.isclose(x[1], y[1] - off, abs_tol=1e-4), (x, y)
        else:
            assert math.isnan(x[1]) and math.isnan(y[1]) and math.isnan(x[3]) and math.isnan(y[3])
    assert any(x[7] for x in a["lv"])


# ------------------------------------------------------------------------------------------------------------ input layouts
def _poison(fmt, buf, lo, hi, front):
    buf[lo:hi].view(NP[fmt])[:] = POISON[fmt][0 if front else 1]


def _device_pushes(fmt, streams, sizes, off, stride_pad):
    """test_gpu_rates._device_pushes for the 2-byte formats: per push one allocation, [GUARD + off poison][stream 0][poison]
    [stream 1][poison][stream 2][GUARD poison], the streams stride bytes apart (a multiple of 16 plus stride_pad)"""
    import torch
    out, pos = [], 0
    for k in sizes:
        nb = k * BYTES
        stride = (nb + 2 * GUARD + 15) // 16 * 16 + stride_pad
        head = GUARD + off * BYTES
        total = head + (len(streams) - 1) * stride + nb + GUARD
        host = np.zeros((total + 15) // 16 * 16, np.uint8)
        _poison(fmt, host, 0, head, True)
        for s, raw in enumerate(streams):
            a = head + s * stride
            host[a:a + nb] = np.ascontiguousarray(raw[PER[fmt] * pos:PER[fmt] * (pos + k)]).view(np.uint8)
            _poison(fmt, host, a + nb, a + stride if s + 1 < len(streams) else total, False)
            if s + 1 < len(streams):
                mid = a + nb + (stride - nb) // 2 // BYTES * BYTES
                _poison(fmt, host, mid, a + stride, True)
        t = torch.from_numpy(host).to("cuda:0")
        out.append((t, t.data_ptr() + head, stride))
        pos += k
    torch.cuda.synchronize()
    return out


@pytest.mark.timeout(300)
@pytest.mark.parametrize("fmt", ["cs8", "s16"])
def test_device_input_at_every_offset_and_stride(built, oracle, monkeypatch, fmt):
    """test_gpu_rates.test_device_input_at_every_offset_and_stride for the two formats at 2 MS/s (k1_fast): three device-resident
    streams, the push at every whole-sample offset from a 16-byte boundary and at a large odd one, strides on and off the 16-byte
    grid, poison in front of and behind every stream.  A kernel that reads outside what was pushed reads poison."""
    rate = 2_000_000
    per = 4 * (rate // 4000)
    fos = _fos(rate, TWIN[fmt])
    sizes = [per * 16, per * 13 + 7, per * 6 - 5, per * 9 + 1, per * 4]
    n = sum(sizes)
    rng = np.random.default_rng(rate // 1000 + (8 if fmt == "cs8" else 16))
    if fmt == "cs8":
        streams = [rng.integers(-128, 128, 2 * n, dtype=np.int8) for _ in range(3)]
    else:
        streams = [rng.integers(-32768, 32768, n, dtype=np.int16) for _ in range(3)]
    want = {(s, c): _oracle_dec(oracle, _twin(streams[s]), TWIN[fmt], rate, fos[c], 0) for s in range(3) for c in (0, 1)}
    monkeypatch.setenv("VDL2GPU_STAGE_EVERY", "1")
    offsets = list(range(16 // BYTES)) + [4099]
    cases = [(off, 0) for off in offsets] + [(0, BYTES), (offsets[-1], BYTES), (1, BYTES)]
    from vdlm2dec_amd.demod import Receiver, plan_channels
    for off, pad in cases:
        bufs = _device_pushes(fmt, streams, sizes, off, pad)
        assert all((p - GUARD - off * BYTES) % 16 == 0 for _, p, _ in bufs)
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
        assert (fast > 0) == (pad == 0), (off, pad, fast)
        del bufs


# ------------------------------------------------------------------------------------------------------------------ extremes
@pytest.mark.timeout(240)
@pytest.mark.parametrize("fmt", ["cs8", "s16"])
def test_rails(built, oracle, monkeypatch, fmt):
    """Thousands of samples at either rail (and, for cs8, I and Q at opposite rails) beside a burst, on all three kernels: a zero-
    where a sign-extension is meant, or I and Q swapped, changes the planes."""
    rate = 2_000_000
    fos = _fos(rate, TWIN[fmt])
    spec = S.regimes(rate=rate, fo=fos, seed=91, infos=(40, 17), gap=0.03)
    raw = synth.synth_stream(spec, fmt).copy()
    lo, hi = (-128, 127) if fmt == "cs8" else (-32768, 32767)
    p = PER[fmt]
    b0 = spec.bursts[0]
    a = int((b0.t0 + b0.duration() + 0.004) * rate)             # in the gap behind the first burst
    raw[p * a:p * (a + 6000)] = lo
    raw[p * (a + 9000):p * (a + 15001)] = hi
    if fmt == "cs8":
        raw[2 * (a + 20000):2 * (a + 24000):2] = lo             # I low, Q high
        raw[2 * (a + 20000) + 1:2 * (a + 24000):2] = hi
        raw[2 * (a + 26000):2 * (a + 30000):2] = hi
        raw[2 * (a + 26000) + 1:2 * (a + 30000):2] = lo
    assert p * (a + 30000) < raw.size and (a + 30000) / rate < spec.bursts[1].t0 - 0.002
    n = raw.size // p
    tw = _twin(raw)
    want = oracle.run_oracle(tw, TWIN[fmt], rate, fos, S.FC)
    assert len(want) == 2
    decs = {c: _oracle_dec(oracle, tw, TWIN[fmt], rate, fos[c], 0) for c in (0, 1)}
    assert max(float(np.abs(d).max()) for d in decs.values()) > (1.0 if fmt == "cs8" else 256.0)
    monkeypatch.setenv("VDL2GPU_STAGE_EVERY", "1")
    for env, fast_wanted in ((None, True), ("VDL2GPU_K1_PP", True), ("VDL2GPU_NO_K1_FAST", False)):
        for k in ("VDL2GPU_NO_K1_FAST", "VDL2GPU_K1_PP"):
            monkeypatch.delenv(k, raising=False)
        if env:
            monkeypatch.setenv(env, "1")
        # whole superperiods from the first sample (k1_fast / k1_pp take all of it) and a push with ragged ends
        for first in (n, n - 8000 * 3 - 77):
            with _rx(rate, fos, fmt, max_push=n, keep_dec=True) as rx:
                parts = {c: [] for c in decs}
                for s0, s1 in ((0, first), (first, n)):
                    if s1 > s0:
                        rx.push(raw[p * s0:p * s1])
                        for c in decs:
                            parts[c].append(rx.debug_dec(0, c))
                got = rx.poll()
                assert (rx.timing()["fast_pushes"] > 0) == fast_wanted, env
            for c, d in decs.items():
                g = np.concatenate(parts[c])
                assert len(g) == len(d) and np.array_equal(_bits(g), _bits(d)), (env, first, c)
            _check(oracle, got, want, rate // 4000)


# --------------------------------------------------------------------------------------------------------- windows of zeros
# rate, format, zero runs as (unit, offset in the unit, length): the unit is what the fast kernel of the rate takes whole, a
# superperiod of 8000 samples at 2 MS/s (k1_fast) and a period of 4 * SDRCLK samples elsewhere (k1_pp).  The short runs cover
# a whole window (23/24, 59/60, 119/120 samples) only at some offsets, the long ones several windows at any; one run straddles
# the end of its unit.  Then 8000 zeros from the start of a unit: at 2 MS/s every window of that superperiod.
ZERO_ROWS = [
    (2_000_000, "cs16", 8, [(1, 0, 30), (1, 1011, 200), (2, 2503, 30), (2, 5000, 200), (4, 7990, 30), (5, 3777, 200),
                            (6, 123, 30), (3, 0, 8000)]),
    (10_000_000, "cs16", 16, [(1, 0, 130), (2, 1011, 700), (4, 2503, 130), (5, 9990, 130), (7, 3777, 700), (9, 123, 130),
                              (12, 2222, 700), (10, 0, 8000)]),
    (5_000_000, "f32", 16, [(1, 0, 130), (2, 1011, 700), (4, 2503, 130), (5, 4990, 130), (7, 3777, 700), (9, 123, 130),
                            (13, 2222, 700), (10, 0, 8000)]),
]


@pytest.mark.timeout(120)
@pytest.mark.parametrize("rate,fmt,units,runs", ZERO_ROWS, ids=[f"{r[0] // 1000}k-{r[1]}" for r in ZERO_ROWS])
def test_zero_windows_beside_live_ones(built, oracle, monkeypatch, rate, fmt, units, runs):
    """Runs of exact zeros in the input: output windows whose sum is exactly zero beside windows of the same wavefront that
    are not, and one stretch in which a whole wavefront's are.  k1_fast and k1_pp then leave the reciprocal division for the
    plain one (k1_div_exact: some lane's |sum| < 1e-30) with live data in the other lanes; the planes must stay the oracle's
    bit for bit, signs of zero included.  One push of whole units from the first sample: the fast kernel takes all of it.
    The records are not compared: the runs cut through bursts."""
    from test_gpu_rates import PER as PER_R
    clk = rate // 4000
    unit = 8000 if rate == 2_000_000 else 4 * clk
    n = units * unit
    fos = _fos(rate, fmt)
    spec = S.regimes(rate=rate, fo=fos, seed=rate // 1000 + 3, infos=(3, 40, 120, 17), gap=0.001)
    p = PER_R[fmt]
    raw = synth.synth_stream(spec, fmt)[:p * n].copy()
    assert raw.size == p * n
    for u, off, ln in runs:
        a = u * unit + off
        assert unit <= a and a + ln <= n - unit         # clear of the push's first and last unit
        raw[p * a:p * (a + ln)] = 0
    decs = {c: _oracle_dec(oracle, raw, fmt, rate, fos[c], 0) for c in (0, len(fos) - 1)}
    for d in decs.values():
        z = (_bits(d).reshape(-1, 2) & 0x7FFFFFFF == 0).all(axis=1)
        # the 8000 zeros alone hold 8000 * 21 / SDRCLK windows less one, every long run a few more
        assert z.sum() >= 8000 * 21 // clk and not z[:84].any() and not z[-84:].any(), int(z.sum())
    monkeypatch.setenv("VDL2GPU_STAGE_EVERY", "1")
    envs = ((None, True), ("VDL2GPU_K1_PP", True), ("VDL2GPU_NO_K1_FAST", False)) if rate == 2_000_000 else ((None, True),)
    for env, fast_wanted in envs:
        for k in ("VDL2GPU_NO_K1_FAST", "VDL2GPU_K1_PP"):
            monkeypatch.delenv(k, raising=False)
        if env:
            monkeypatch.setenv(env, "1")
        with _rx(rate, fos, fmt, max_push=n, keep_dec=True) as rx:
            rx.push(raw)
            _planes_equal(rx, decs, env or "default")
            rx.poll()
            assert (rx.timing()["fast_pushes"] > 0) == fast_wanted, env


# ---------------------------------------------------------------------------------------------------------------------- ring
@pytest.mark.timeout(240)
def test_ingest_ring_cs8(built, oracle):
    """Slots of 32768 cs8 samples: 2 bytes a sample in the ring as for cu8, and the bursts are the push path's and the oracle's."""
    spec = S.eight_channels()
    raw = synth.synth_stream(spec, "cs8")
    want = oracle.run_oracle(_twin(raw), "cf32", spec.rate, spec.fo, S.FC)
    assert len(want) == len(spec.bursts) == 16
    blk = 32768
    with _rx(spec.rate, spec.fo, "cu8", max_push=blk) as rx:
        rx.ring_init(blk, nslots=3)
        cu8_stride = rx.ring_acquire().shape[1]
        rx.ring_commit(0)
    with _rx(spec.rate, spec.fo, "cs8", max_push=blk) as rx:
        pushed = rx.run(raw, block=blk)
    with _rx(spec.rate, spec.fo, "cs8", max_push=blk) as rx:
        rx.ring_init(blk, nslots=3)
        got = []
        rawb = raw.view(np.uint8)
        for i, s0 in enumerate(range(0, spec.nsamples, blk)):
            m = min(blk, spec.nsamples - s0)
            slot = rx.ring_acquire()
            assert slot.shape == (1, cu8_stride)                    # what a cu8 handle gets: 2 bytes a sample
            slot[0, :2 * m] = rawb[2 * s0:2 * (s0 + m)]
            rx.ring_commit(m)
            if i % 3 == 2:
                got += rx.poll_ready()
        got += rx.poll()
    assert cu8_stride == blk * 2                                    # no padding today: a slot is the samples
    key = lambda b: (b.chn, b.end_dec)      # noqa: E731
    assert sorted(got, key=key) == sorted(pushed, key=key)
    _check(oracle, got, want, spec.rate // 4000)


# ------------------------------------------------------------------------------------------------------------- many streams
@pytest.mark.timeout(300)
def test_eight_streams_of_cs8(built, oracle):
    """8 streams x 8 channels in one handle (the streams' addresses are multiples of the sample size): every stream's bursts
    against the push of that stream alone on the oracle, for the first and the last stream; planes for both."""
    specs = [S.eight_channels(seed=8 + s) for s in range(8)]
    n = min(sp.nsamples for sp in specs)
    raws = [synth.synth_stream(sp, "cs8")[:2 * n] for sp in specs]
    from vdlm2dec_amd.demod import Receiver, plan_channels
    with Receiver(2_000_000, [plan_channels(S.FC, sp.fo) for sp in specs], fmt="cs8", max_push=n, keep_dec=True) as rx:
        rx.push(np.stack(raws))
        got = rx.poll()
        planes = {(s, c): rx.debug_dec(s, c) for s in (0, 7) for c in (0, 7)}
    assert {b.stream for b in got} == set(range(8))
    for s in (0, 7):
        tw = _twin(raws[s])
        want = oracle.run_oracle(tw, "cf32", 2_000_000, specs[s].fo, S.FC)
        if s == 0:
            assert len(want) == len(specs[0].bursts) == 16
        assert len(want) >= 10
        _check(oracle, [b for b in got if b.stream == s], want, 500)
        for c in (0, 7):
            d = _oracle_dec(oracle, tw, "cf32", 2_000_000, specs[s].fo[c], 0)
            g = planes[(s, c)]
            assert len(g) == len(d) and np.array_equal(_bits(g), _bits(d)), (s, c)
