"""VDL2GPU_F_LEVELS on the GPU: the levels change nothing else, agree with the definition (tests/levels_ref.py) on the planes
the demodulator held, are bit-identical across pushes, paths and repair rounds, scale exactly, and measure what physics says."""
import ctypes as C
import math

import numpy as np
import pytest

import levels_ref as R
import scenarios as S
from vdlm2dec_amd import lib, synth

pytestmark = pytest.mark.gpu

EINVAL = -1      # VDL2GPU_EINVAL
FMT_SYNTH = {"cu8": "cu8", "cs16": "cs16", "cf32": "cf32", "f32r": "f32"}     # Receiver / synth name of each format


def _rx(spec, fmt, nstreams=1, **kw):
    from vdlm2dec_amd.demod import Receiver, plan_channels
    plan = plan_channels(S.FC, spec.fo)
    return Receiver(spec.rate, [plan] * nstreams if nstreams > 1 else plan, fmt=fmt, **kw)


def _lv(b):
    L = b.level
    return (np.float32(L.sig_power).view(np.uint32).item(), np.float32(L.noise_power).view(np.uint32).item(),
            L.sym_first_dec, L.nsym, L.subphase, L.noise_blocks)


def _by_burst(bursts):
    out = {}
    for b in bursts:
        k = (b.stream, b.chn, b.trig_dec)
        assert k not in out
        out[k] = _lv(b)
    return out


def _raw_recs(rx, n=1 << 14, levels=False):
    """one poll into ctypes arrays (lv == NULL on a plain handle)"""
    buf = (lib.BurstT * n)()
    lv = (lib.LevelT * n)() if levels else None
    k = rx.poll_levels_raw(buf, lv, n)
    return buf, lv, k


@pytest.mark.timeout(300)
@pytest.mark.parametrize("fmt,rate,fo", [("cu8", 2_000_000, S.FO8), ("cs16", 10_000_000, S.FO8_10MS)])
def test_levels_change_nothing_else(built, fmt, rate, fo):
    spec = S.eight_channels(rate=rate, fo=fo)
    raw = synth.synth_stream(spec, fmt)
    res = []
    for levels in (False, True):
        with _rx(spec, fmt, max_push=1 << 19, frames=True, levels=levels) as rx:
            for s in range(0, raw.size // 2, 1 << 18):
                rx.push(raw[2 * s:2 * min(raw.size // 2, s + (1 << 18))])
            buf, lv, n = _raw_recs(rx, levels=levels)
            recs = bytes(C.string_at(C.addressof(buf), n * C.sizeof(lib.BurstT)))
            res.append((recs, n, rx.stats(), rx.poll_frames()))
            if levels:
                assert all(lv[i].nsym > 0 for i in range(n))
    assert res[0][1] >= 10
    assert res[0] == res[1]


def _check_exact(rx, bursts, spec, fmt, nstreams=1):
    mflt = R.mflt_taps()
    K = R.scale_k("f32" if fmt == "f32r" else fmt, spec.rate, mflt)
    planes = {}
    db = lambda p: 10 * math.log10(p / K) if p > 0 else -math.inf      # noqa: E731  (a window of exact zeros: the power is 0 to the bit)
    for b in bursts:
        L = b.level
        if (b.stream, b.chn) not in planes:
            planes[(b.stream, b.chn)] = rx.debug_dec(b.stream, b.chn)
        x = planes[(b.stream, b.chn)]
        # the pinned relation: the last evaluation is end_dec, the first lies 1..8 behind the trigger (burst_timing's j0)
        assert L.sym_first_dec + 8 * (L.nsym - 1) == b.end_dec
        assert 1 <= L.sym_first_dec - b.trig_dec <= 8 and 0 <= L.subphase <= 3
        # nsym from the burst geometry (burst_geom; nbrow / nlbyte of the header)
        nd_last = b.nlbyte if b.nlbyte else 249
        nd = (b.nbrow - 1) * 249 + nd_last
        if b.nlbyte <= 2:
            nf_rows, nf_last = b.nbrow - 1, 6
        else:
            nf_rows, nf_last = b.nbrow, (2 if b.nlbyte <= 30 else (4 if b.nlbyte <= 67 else 6))
        nf = (nf_rows - 1) * 6 + nf_last if nf_rows > 0 else 0
        assert L.nsym == (25 + 8 * (nd + nf) + 2) // 3
        sig, noise, nb = R.levels(x, mflt, L.sym_first_dec, L.nsym, L.subphase)
        assert L.noise_blocks == nb
        assert math.isclose(L.sig_power, sig, rel_tol=1e-5), (b.trig_dec, L, sig)
        assert math.isclose(L.sig_dbfs, db(sig), abs_tol=1e-4)
        if nb:
            assert math.isclose(L.noise_power, noise, rel_tol=1e-5), (b.trig_dec, L, noise)
            assert math.isclose(L.noise_dbfs, db(noise), abs_tol=1e-4)
        else:
            assert math.isnan(L.noise_power) and math.isnan(L.noise_dbfs)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("fmt,rate", [("cu8", 2_000_000), ("cs16", 2_000_000), ("cf32", 2_000_000), ("f32r", 2_000_000),
                                      ("cs16", 10_000_000), ("cu8", 10_000_000)])
def test_levels_exact_against_definition(built, fmt, rate):
    if fmt == "f32r":
        spec = S.eight_channels(rate=5_000_000, fo=S.FO8_AIR_5MS)
    else:
        spec = S.eight_channels(rate=rate, fo=S.FO8 if rate == 2_000_000 else S.FO8_10MS)
    raw = synth.synth_stream(spec, FMT_SYNTH[fmt])
    with _rx(spec, FMT_SYNTH[fmt], max_push=spec.nsamples, keep_dec=True, levels=True) as rx:
        rx.push(raw)
        bursts = rx.poll()
        assert len(bursts) >= 10
        _check_exact(rx, bursts, spec, fmt)


@pytest.mark.timeout(300)
def test_levels_exact_three_streams(built):
    specs = [S.eight_channels(seed=8 + s) for s in range(3)]
    n = min(sp.nsamples for sp in specs)
    raw = np.stack([synth.synth_stream(sp, "cs16")[:2 * n] for sp in specs])
    with _rx(specs[0], "cs16", nstreams=3, max_push=n, keep_dec=True, levels=True) as rx:
        rx.push(raw)
        bursts = rx.poll()
        assert len({b.stream for b in bursts}) == 3
        _check_exact(rx, bursts, specs[0], "cs16", 3)


@pytest.mark.timeout(300)
def test_levels_cut_invariance(built):
    spec = synth.random_scenario(2_000_000, S.FO8, 1 << 21, seed=71, bursts_per_s=20.0, info_max=400)
    raw = synth.synth_stream(spec, "cs16")
    n = raw.size // 2
    runs = []
    with _rx(spec, "cs16", max_push=n, levels=True) as rx:
        runs.append(_by_burst(rx.run(raw, block=n)))
    with _rx(spec, "cs16", max_push=32768, levels=True) as rx:
        runs.append(_by_burst(rx.run(raw, block=32768)))
    rng = np.random.default_rng(5)
    with _rx(spec, "cs16", max_push=1 << 18, levels=True) as rx:
        got, s = [], 0
        while s < n:
            e = min(n, s + int(rng.integers(1000, 1 << 18)))
            rx.push(raw[2 * s:2 * e])
            got += rx.poll_ready()
            s = e
        got += rx.poll()
        runs.append(_by_burst(got))
    with _rx(spec, "cs16", max_push=32768, levels=True) as rx:
        rx.ring_init(32768, 4)
        got = []
        for s in range(0, n, 32768):
            m = min(32768, n - s)
            slot = rx.ring_acquire()
            slot[0, :4 * m] = raw[2 * s:2 * (s + m)].view(np.uint8)
            rx.ring_commit(m)
            got += rx.poll_ready()
        got += rx.poll()
        runs.append(_by_burst(got))
    assert len(runs[0]) >= 20
    for r in runs[1:]:
        assert r == runs[0]


@pytest.mark.timeout(600)
def test_levels_path_invariance(built):
    spec = synth.random_scenario(2_000_000, S.FO8[:4], 1 << 20, seed=93, bursts_per_s=25.0, info_max=200)
    raw = synth.synth_stream(spec, "cs16")
    runs = []
    for kw in ({}, {"serial": True}, {"full_scan": True}, {"flags": lib.F_TEST_NOREGION}):
        with _rx(spec, "cs16", max_push=1 << 18, levels=True, **kw) as rx:
            runs.append(_by_burst(rx.run(raw)))
            st = rx.stats()
        if kw.get("flags"):
            assert st["repairs"] + st["serial_redos"] > 0, st
    assert len(runs[0]) >= 10
    for r in runs[1:]:
        assert r == runs[0]


@pytest.mark.timeout(300)
def test_levels_through_repair_rounds(built):
    """A repair round voids and re-decodes bursts (the recording test_gpu_parity uses for it): the same levels as the serial machine."""
    import bench
    spec, raw = bench.make_tile(1077, "cs16", 2_000_000, S.FO8, 4.0)
    big = np.concatenate([raw, bench.make_tile(2077, "cs16", 2_000_000, S.FO8, 4.0)[1]])
    with _rx(spec, "cs16", max_push=big.size // 2, levels=True) as rx:
        rx.push(big)
        a = _by_burst(rx.poll())
        st = rx.stats()
    with _rx(spec, "cs16", max_push=big.size // 2, levels=True, serial=True) as rx:
        rx.push(big)
        b = _by_burst(rx.poll())
    assert st["repairs"] >= 1, st
    assert a == b and len(a) >= 60


@pytest.mark.timeout(300)
def test_levels_scale_exactly(built):
    spec = S.eight_channels()
    raw = synth.synth_stream(spec, "cf32")
    res = []
    for g in (1.0, 2.0):
        with _rx(spec, "cf32", max_push=spec.nsamples, levels=True) as rx:
            res.append(rx.run(raw * np.float32(g), block=1 << 16))
    assert [b.key() for b in res[0]] == [b.key() for b in res[1]] and len(res[0]) >= 10
    for a, b in zip(res[0], res[1]):
        assert np.float32(b.level.sig_power) == np.float32(4.0) * np.float32(a.level.sig_power)
        if a.level.noise_blocks:
            assert np.float32(b.level.noise_power) == np.float32(4.0) * np.float32(a.level.noise_power)


def _one_channel(amp, noise, seed, nb=12):
    rng = np.random.default_rng(seed)
    bursts, t = [], 0.04
    for _ in range(nb):
        b = synth.Burst(chan=0, t0=t, info=bytes(rng.integers(0, 256, 40, dtype=np.uint8).tolist()), amp=amp, cfo=0.0)
        bursts.append(b)
        t += b.duration() + 0.04
    return synth.StreamSpec(rate=2_000_000, fo=(100_000,), nsamples=S._pad(int((t + 0.01) * 2_000_000)), bursts=bursts,
                            noise=noise, seed=seed)


@pytest.mark.timeout(300)
def test_levels_physics(built):
    mflt = R.mflt_taps().astype(np.float64)
    K = R.scale_k("cf32", 2_000_000, mflt)
    sigma = 1.6
    spec = _one_channel(40.0, sigma, 3)
    with _rx(spec, "cf32", max_push=spec.nsamples, levels=True) as rx:
        got = rx.run(synth.synth_stream(spec, "cf32"))
    nd = [b.level.noise_dbfs for b in got if b.level.noise_blocks == 8]
    assert len(nd) >= 8
    # the channeliser averages M = sdrinrate / 84000 input samples per output: noise power 2 sigma^2 / M per output sample
    want = 10 * math.log10(2 * sigma ** 2 / (2_000_000 / 84000) * float(np.sum(mflt[0::4] ** 2)) / K)
    assert abs(float(np.mean(nd)) - want) < 0.3, (np.mean(nd), want)
    # sigma = 0: amplitude A and 2A on otherwise equal bursts read 6.02 dB apart
    means = []
    for amp in (20.0, 40.0):
        spec = _one_channel(amp, 0.0, 4)
        with _rx(spec, "cf32", max_push=spec.nsamples, levels=True) as rx:
            got = rx.run(synth.synth_stream(spec, "cf32"))
        assert len(got) == 12
        means.append(float(np.mean([b.level.sig_dbfs for b in got])))
    assert abs(means[1] - means[0] - 6.02) < 0.2, means


@pytest.mark.timeout(300)
def test_levels_api_edges(built):
    spec = S.eight_channels()
    raw = synth.synth_stream(spec, "cu8")
    with _rx(spec, "cu8", max_push=spec.nsamples) as rx:        # no F_LEVELS
        rx.push(raw)
        buf = (lib.BurstT * 4096)()
        lv = (lib.LevelT * 4096)()
        assert rx.L.vdl2gpu_poll_levels(rx.h, buf, lv, 4096) == EINVAL
        assert rx.L.vdl2gpu_poll_levels_ready(rx.h, buf, lv, 4096) == EINVAL
        n = rx.poll_levels_raw(buf, None, 4096)                 # lv == NULL: the plain poll; nothing was consumed above
        plain = [bytes(C.string_at(C.addressof(buf[i]), C.sizeof(lib.BurstT))) for i in range(n)]
    with _rx(spec, "cu8", max_push=spec.nsamples) as rx:
        rx.push(raw)
        m = rx.poll_raw(buf, 4096)
        assert plain == [bytes(C.string_at(C.addressof(buf[i]), C.sizeof(lib.BurstT))) for i in range(m)] and n >= 10
    with _rx(spec, "cu8", max_push=spec.nsamples, levels=True) as rx:
        rx.push(raw)
        want = {(b.stream, b.chn, b.trig_dec): _lv(b) for b in rx.poll()}
    with _rx(spec, "cu8", max_push=spec.nsamples, levels=True) as rx:
        rx.push(raw)
        got, plain_keys = {}, []
        for turn in range(10000):
            if turn % 2:
                k = rx.poll_levels_raw(buf, lv, 3)
                for i in range(k):
                    key = (buf[i].stream, buf[i].chn, buf[i].trig_dec)
                    got[key] = (np.float32(lv[i].sig_power).view(np.uint32).item(), np.float32(lv[i].noise_power).view(np.uint32).item(),
                                lv[i].sym_first_dec, lv[i].nsym, lv[i].subphase, lv[i].noise_blocks)
            else:
                k = rx.poll_raw(buf, 2)
                plain_keys += [(buf[i].stream, buf[i].chn, buf[i].trig_dec) for i in range(k)]
            if k == 0 and turn > 2:
                break
    assert not set(got) & set(plain_keys)
    assert set(got) | set(plain_keys) == set(want) and len(got) + len(plain_keys) == len(want)
    assert all(got[k] == want[k] for k in got)
    # the stream's start clips the noise window of the first bursts: none of it (NaN) for the stream's first, part of it later
    with _rx(spec, "cu8", max_push=spec.nsamples, levels=True) as rx:
        bursts = sorted(rx.run(raw), key=lambda b: b.trig_dec)
    assert bursts[0].level.noise_blocks < 8
    assert bursts[0].level.noise_blocks == 0 and math.isnan(bursts[0].level.noise_power) and math.isnan(bursts[0].level.noise_dbfs)
    assert any(0 < b.level.noise_blocks < 8 for b in bursts)
    for b in bursts:
        assert (b.level.noise_blocks == 0) == math.isnan(b.level.noise_power)
        assert b.level.noise_blocks == min(8, max(0, (b.level.sym_first_dec - 776) // 256 + 1))
