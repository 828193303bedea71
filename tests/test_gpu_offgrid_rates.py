"""The pipeline at sample rates off the 25 kHz grid (2.048, 2.56, 1.92, 7.68, 15.36, 30.72 MS/s), through the C ABI.

The oracle's LO table is SDRINRATE / 25000 entries long, no whole period of the oscillator off the grid, so it judges only the
centre channel there (test_centre_channel_equals_the_plain_oracle).  Everywhere else the yardsticks are those of
tests/offgrid_model.py, which tests/test_offgrid_rates.py pins to the oracle: the numpy channeliser model for the 84 kS/s planes
(P3) and the oracle's demodulator run over the model's planes for the burst records (P2) and frames (P1).

Which channeliser runs: whole periods of a 16-byte-aligned push go to k1_pp at every rate here (timing()["fast_pushes"]); the
edges, short pushes, unaligned pointers and VDL2GPU_NO_K1_FAST go to k1_channelise -- with the LO table in LDS where it fits
160 KiB beside the windows (2.048 MS/s: 131 KB of table), with the table in global memory where it does not (15.36 and 30.72 MS/s:
vdl2gpu_debug_k1 counts the launches of each, _check_kernels)."""
import numpy as np
import pytest

import offgrid_model as M
import scenarios as S
import test_gpu_rates as TR
from vdlm2dec_amd import synth

pytestmark = pytest.mark.gpu

PER = {"cu8": 2, "cs16": 2, "cf32": 2, "f32": 1, "cs8": 2, "s16": 1}
# rate, format, channels
SCENARIOS = [
    (2_048_000, "cu8", 8), (2_560_000, "cs8", 2), (1_920_000, "cf32", 3), (7_680_000, "f32", 2), (15_360_000, "cs16", 4),
    (30_720_000, "s16", 1), (2_048_000, "s16", 2), (15_360_000, "cu8", 1),
]


def _table_in_lds(rate, sdrclk=0):
    """vdl2gpu_create's rule: the general kernel's whole LDS (table, wrap-around, windows) within 160 KiB"""
    from vdlm2dec_amd import lib
    L, maxwin = lib.load().vdl2gpu_lo_len(rate), ((sdrclk or rate // 4000) + 20) // 21
    return ((L + maxwin) * 8 + 32 * maxwin) * 8 <= 160 * 1024


def _check_kernels(rx, rate, fast, sdrclk=0):
    """what the host launched (vdl2gpu_debug_k1): the general kernel with the table where the rate puts it and never the other
    one, k1_pp exactly when whole periods were expected on it, k1_fast never off the grid"""
    k = rx.debug_k1()
    lds = _table_in_lds(rate, sdrclk)
    assert k["general_global" if lds else "general_lds"] == 0 and k["k1_fast"] == 0, k
    assert (k["k1_pp"] > 0) == fast, k
    return k["general_lds" if lds else "general_global"]


def fos_of(rate, fmt, nch):
    """nch offsets on the 25 kHz grid, none at the centre, spread over the band (real input: above the mixer centre)"""
    lo, hi = (0.12, 0.4) if fmt in M.REAL else (-0.36, 0.38)
    f = [TR._grid((lo + (hi - lo) * (c + 0.5) / nch) * rate) for c in range(nch)]
    assert len(set(f)) == nch and 0 not in f and all(v % 25_000 == 0 for v in f)
    return tuple(f)


def scenario(rate, fmt, nch):
    """one short burst per channel (two on one or two channels); the seeds are ones with which the reference's demodulator
    decodes every channel (tests/test_offgrid_rates.py checks it on the CPU)"""
    infos = (3, 40, 9, 28, 12, 31, 60, 10)[:max(nch, 2)]
    spec = S.regimes(rate=rate, fo=fos_of(rate, fmt, nch), seed=8 if nch == 8 else rate // 1000 + nch, infos=infos, gap=0.001)
    return spec, synth.synth_stream(spec, fmt)


def expected(O, raw, fmt, rate, fos):
    planes = [M.channelise(raw, fmt, rate, fo) for fo in fos]
    return {"planes": planes, "blocks": [M.demod_blocks(O, p, S.FC + fo, chn=c) for c, (p, fo) in enumerate(zip(planes, fos))]}


def _rx(rate, fos, fmt, nstreams=1, **kw):
    from vdlm2dec_amd.demod import Receiver, plan_channels
    ch = plan_channels(S.FC, fos)
    return Receiver(rate, ch if nstreams == 1 else [ch] * nstreams, fmt=fmt, **kw)


_gfields = M.block_fields      # a vdl2gpu_burst_t has the fields of the oracle's block


def _check_bursts(got, blocks, sdrclk, stream=0):
    """records of one stream equal to the demodulator-only oracle's, and their sample stamps to the schedule's (vdl2gpu_plan:
    output j ends at input ceil((j + 1) * SDRCLK / 21) - 1)"""
    key = lambda f: (f[0], f[6])      # noqa: E731
    got = [b for b in got if b.stream == stream]
    assert sorted((_gfields(b) for b in got), key=key) == sorted((M.block_fields(b) for bl in blocks for b in bl), key=key)
    for b in got:
        assert b.trig_sample == ((b.trig_dec + 1) * sdrclk + 20) // 21 - 1, (b.trig_dec, b.trig_sample)
        assert b.end_sample == ((b.end_dec + 1) * sdrclk + 20) // 21 - 1, (b.end_dec, b.end_sample)


def _check_planes(rx, planes, what, stream=0):
    for c, d in enumerate(planes):
        g = rx.debug_dec(stream, c)
        assert len(g) == len(d) and np.array_equal(M.bits(g), M.bits(d)), (what, stream, c)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("rate,fmt,nch", SCENARIOS, ids=[f"{r // 1000}k-{f}-{n}ch" for r, f, n in SCENARIOS])
def test_planes_bursts_and_frames(built, oracle, monkeypatch, rate, fmt, nch):
    clk = rate // 4000
    spec, raw = scenario(rate, fmt, nch)
    n = raw.size // PER[fmt]
    want = expected(oracle, raw, fmt, rate, spec.fo)
    wf = []
    for c, bl in enumerate(want["blocks"]):
        fr = [(0, c, f) for b in sorted(bl, key=lambda b: b.end_dec) for f in oracle.frames_of_block(b.nbrow, b.nlbyte, b.data)]
        assert len(fr) >= 1, c          # every channel decodes a CRC-clean frame: nothing below passes empty
        wf += fr
    monkeypatch.setenv("VDL2GPU_STAGE_EVERY", "1")
    monkeypatch.delenv("VDL2GPU_NO_K1_FAST", raising=False)
    with _rx(rate, spec.fo, fmt, max_push=n, keep_dec=True, frames=True) as rx:
        rx.push(raw)
        _check_planes(rx, want["planes"], "whole")                          # P3
        _check_bursts(rx.poll(), want["blocks"], clk)                       # P2
        assert sorted(rx.poll_frames()) == sorted(wf)                       # P1
        assert rx.timing()["fast_pushes"] > 0                               # whole periods on k1_pp
        _check_kernels(rx, rate, True)
    # the same through the general kernel alone: the table in LDS at 2.048 / 2.56 / 1.92 / 7.68 MS/s, in global memory above
    assert _table_in_lds(rate) == (rate < 15_000_000)
    monkeypatch.setenv("VDL2GPU_NO_K1_FAST", "1")
    with _rx(rate, spec.fo, fmt, max_push=n, keep_dec=True) as rx:
        rx.push(raw)
        _check_planes(rx, want["planes"], "general")
        assert rx.timing()["fast_pushes"] == 0
        assert _check_kernels(rx, rate, False) == 1                         # one launch of the right general kernel took it all
        _check_bursts(rx.poll(), want["blocks"], clk)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("rate,fmt", [(2_048_000, "cu8"), (7_680_000, "cs16")])
def test_centre_channel_equals_the_plain_oracle(built, oracle, rate, fmt):
    """Fo = 0: every table entry is 1 - 0j whatever the table's length, so the oracle fed the raw recording is exact -- an
    end-to-end check with no model in between."""
    spec = S.regimes(rate=rate, fo=(0,), seed=rate // 1000, infos=(3, 40, 120, 17), gap=0.001)
    raw = synth.synth_stream(spec, fmt)
    want = oracle.run_oracle(raw, fmt, rate, (0,), S.FC)
    assert len(want) >= 3
    dec = TR._oracle_dec(oracle, raw, fmt, rate, 0, 0)
    with _rx(rate, (0,), fmt, max_push=spec.nsamples, keep_dec=True, frames=True) as rx:
        rx.push(raw)
        _check_planes(rx, [dec], "centre")
        TR._check_bursts(oracle, rx.poll(), want, rate // 4000, rx.poll_frames())


PATHS = [(2_048_000, "cu8"), (15_360_000, "cs16")]


def _small_sizes(per, n):
    """single samples and pushes shorter than four periods, then the rest in pushes of nine periods and a bit, n samples in all"""
    out = [1, 1, 2, 3, 7, per // 3, per - 1, per, per + 1, 2 * per + 5, 1, 3 * per + per // 2, 4 * per - 1, 1, 5 * per + 3, 2, 1]
    assert sum(out) < n
    while sum(out) < n:
        out.append(min(9 * per + 11, n - sum(out)))
    return out


@pytest.mark.timeout(900)
@pytest.mark.parametrize("rate,fmt", PATHS, ids=[f"{r // 1000}k-{f}" for r, f in PATHS])
def test_every_push_shape_gives_the_whole_push(built, oracle, monkeypatch, rate, fmt):
    """ragged pushes (periods +- remainders), pushes down to single samples and shorter than four periods, and 8 streams: the
    planes and bursts of the one whole push, which are the model's"""
    clk = rate // 4000
    per = 4 * clk
    spec, raw = scenario(rate, fmt, 2)
    n = raw.size // PER[fmt]
    want = expected(oracle, raw, fmt, rate, spec.fo)
    assert sum(len(b) for b in want["blocks"]) >= 2
    monkeypatch.setenv("VDL2GPU_STAGE_EVERY", "1")
    monkeypatch.delenv("VDL2GPU_NO_K1_FAST", raising=False)
    for what, sizes in (("ragged", TR._ragged(per, n, np.random.default_rng(rate))),
                        ("small", _small_sizes(per, n))):
        assert what != "small" or (min(sizes) == 1 and sum(k < 4 * per for k in sizes) >= 10)
        with _rx(rate, spec.fo, fmt, max_push=max(sizes), keep_dec=True) as rx:
            parts, got, pos = [[] for _ in spec.fo], [], 0
            for k in sizes:
                rx.push(raw[PER[fmt] * pos:PER[fmt] * (pos + k)])
                for c in range(len(spec.fo)):
                    parts[c].append(rx.debug_dec(0, c))
                got += rx.poll_ready()
                pos += k
            got += rx.poll()
            fast = rx.timing()["fast_pushes"]
            assert _check_kernels(rx, rate, True) >= (len(sizes) if what == "small" else min(len(sizes) - 1, 1))   # small: every push has an edge
        for c, d in enumerate(want["planes"]):
            g = np.concatenate(parts[c])
            assert len(g) == len(d) and np.array_equal(M.bits(g), M.bits(d)), (what, c)
        _check_bursts(got, want["blocks"], clk)
        assert fast > 0, what           # the long pushes among them take k1_pp between two general launches
    # 8 streams: the recording shifted circularly by a different number of samples in each
    shifts = [0, 1, 777, per, 5 * per + 3, n // 3, n // 2 + 1, n - 5]
    streams = [np.roll(raw, PER[fmt] * sh) for sh in shifts]
    wants = [want] + [expected(oracle, s, fmt, rate, spec.fo) for s in streams[1:]]
    with _rx(rate, spec.fo, fmt, nstreams=8, max_push=n, keep_dec=True) as rx:
        rx.push(np.stack(streams))
        for s in range(8):
            _check_planes(rx, wants[s]["planes"], "8 streams", s)
        got = rx.poll()
        for s in range(8):
            _check_bursts(got, wants[s]["blocks"], clk, s)
        assert rx.timing()["fast_pushes"] > 0


@pytest.mark.timeout(900)
@pytest.mark.parametrize("rate,fmt", PATHS, ids=[f"{r // 1000}k-{f}" for r, f in PATHS])
def test_device_input_at_every_offset(built, monkeypatch, rate, fmt):
    """Two streams of device-resident samples, every push in its own allocation with poison around each stream (the layout of
    test_gpu_rates.py), starting at every whole-sample offset from a 16-byte boundary and at a large odd one; a stream stride off
    the 16-byte grid turns k1_pp off.  A kernel that reads outside what was pushed reads poison, and the planes differ."""
    from vdlm2dec_amd.demod import Receiver, plan_channels
    B = TR.BYTES[fmt]
    per = 4 * (rate // 4000)
    fos = fos_of(rate, fmt, 2)
    sizes = [per * 16, per * 13 + 7, per * 6 - 5, per * 9 + 1, per * 4]
    n = sum(sizes)
    rng = np.random.default_rng(rate // 1000 + B)
    if fmt == "cu8":
        streams = [rng.integers(0, 256, 2 * n, dtype=np.uint8) for _ in range(2)]
    else:
        streams = [rng.integers(-3000, 3000, 2 * n, dtype=np.int16) for _ in range(2)]
    want = {(s, c): M.channelise(streams[s], fmt, rate, fos[c]) for s in range(2) for c in range(2)}
    monkeypatch.setenv("VDL2GPU_STAGE_EVERY", "1")
    monkeypatch.delenv("VDL2GPU_NO_K1_FAST", raising=False)
    offsets = list(range(16 // B)) + [4099]
    for off, pad in [(off, 0) for off in offsets] + [(0, B), (1, B)]:
        bufs = TR._device_pushes(fmt, streams, sizes, off, pad)
        assert all((p - TR.GUARD - off * B) % 16 == 0 for _, p, _ in bufs)
        with Receiver(rate, [plan_channels(S.FC, fos)] * 2, fmt=fmt, max_push=max(sizes), keep_dec=True) as rx:
            parts = {k: [] for k in want}
            for (t, p, stride), k in zip(bufs, sizes):
                rx.push_device(p, k, stride)
                for s, c in want:
                    parts[(s, c)].append(rx.debug_dec(s, c))
            rx.poll()
            fast = rx.timing()["fast_pushes"]
            assert _check_kernels(rx, rate, pad == 0) >= 1
        for (s, c), d in want.items():
            g = np.concatenate(parts[(s, c)])
            assert len(g) == len(d) and np.array_equal(M.bits(g), M.bits(d)), (off, pad, s, c)
        assert (fast > 0) == (pad == 0), (off, pad, fast)
        del bufs


@pytest.mark.timeout(300)
def test_ring_at_2048k(built, oracle):
    """the ingest ring (vdl2gpu_ring_*) at 2.048 MS/s cu8: the bursts of vdl2gpu_push"""
    rate, fmt = 2_048_000, "cu8"
    spec, raw = scenario(rate, fmt, 2)
    n = raw.size // 2
    want = expected(oracle, raw, fmt, rate, spec.fo)
    with _rx(rate, spec.fo, fmt, max_push=n) as rx:
        rx.push(raw)
        pushed = sorted(_gfields(b) for b in rx.poll())
    slot = 40_000           # no whole number of periods: every commit carries a window over
    with _rx(rate, spec.fo, fmt, max_push=slot) as rx:
        rx.ring_init(slot, 4)
        got = []
        for pos in range(0, n, slot):
            k = min(slot, n - pos)
            buf = rx.ring_acquire()
            buf[0, :2 * k] = raw[2 * pos:2 * (pos + k)]
            rx.ring_commit(k)
            got += rx.poll_ready()
        got += rx.poll()
    assert len(pushed) >= 2 and sorted(_gfields(b) for b in got) == pushed
    _check_bursts(got, want["blocks"], rate // 4000)


# rate, SDRCLK: a custom SDRCLK that makes a window (512 samples) many LO tables long (128 and 21 entries); the table would fit
# LDS, the windows beside it do not, so these handles run the global-table kernel with an index that wraps several times a tile
LONG_WINDOWS = [(128_000, 10752), (105_000, 10752)]


@pytest.mark.timeout(300)
@pytest.mark.parametrize("rate,sdrclk", LONG_WINDOWS, ids=[f"{r // 1000}k-{c}" for r, c in LONG_WINDOWS])
def test_windows_longer_than_the_table(built, monkeypatch, rate, sdrclk):
    from vdlm2dec_amd import lib
    L, per = lib.load().vdl2gpu_lo_len(rate), 4 * sdrclk
    assert per % L == 0 and (sdrclk + 20) // 21 == 512 > L and not _table_in_lds(rate, sdrclk)
    fos = (25_000, -50_000)
    n = 9 * per + 12345
    raw = np.random.default_rng(rate).integers(-3000, 3000, 2 * n, dtype=np.int16)
    want = [M.channelise(raw, "cs16", rate, fo, sdrclk) for fo in fos]
    monkeypatch.setenv("VDL2GPU_STAGE_EVERY", "1")
    monkeypatch.delenv("VDL2GPU_NO_K1_FAST", raising=False)
    for sizes in ([n], [per + 7, 1, 5 * per - 3, n - 6 * per - 5]):
        with _rx(rate, fos, "cs16", sdrclk=sdrclk, max_push=max(sizes), keep_dec=True) as rx:
            parts, pos = [[] for _ in fos], 0
            for k in sizes:
                rx.push(raw[2 * pos:2 * (pos + k)])
                for c in range(len(fos)):
                    parts[c].append(rx.debug_dec(0, c))
                pos += k
            rx.poll()
            k1 = rx.debug_k1()
        assert k1["general_global"] >= len(sizes) and k1["general_lds"] == 0, k1
        assert (k1["k1_pp"] > 0) == (L >= 32), k1       # k1_pp steps its table index by chunks of 32: not with a table of 21
        for c, d in enumerate(want):
            g = np.concatenate(parts[c])
            assert len(g) == len(d) and np.array_equal(M.bits(g), M.bits(d)), (sizes, c)
