"""VDL2GPU_F_SYMCLK on the GPU: the records agree with the definition (tests/symclk_ref.py) on the planes the demodulator held, at
every segment edge; the flag changes nothing else; the records are bit-identical across cuts and paths; every stream is measured on
its own plane; the collectors' edges; and the numbers mean what the header says (a transmitter's arrival time and clock offset, within
twice the model's own error: symclk_ref.B_*)."""
import ctypes as C
import math

import numpy as np
import pytest

import levels_ref as LR
import scenarios as S
import symclk_ref as R
from vdlm2dec_amd import demod, lib, synth

pytestmark = pytest.mark.gpu

EINVAL = -1      # VDL2GPU_EINVAL


def _rx(spec, fmt, nstreams=1, **kw):
    from vdlm2dec_amd.demod import Receiver, plan_channels
    plan = plan_channels(S.FC, spec.fo)
    return Receiver(spec.rate, [plan] * nstreams if nstreams > 1 else plan, fmt=fmt, **kw)


def _sig(k):
    """a symbol-clock record to the bit (NaN included)"""
    return (k.sym_first_dec, k.nsym, k.nseg, np.float64(k.toa_sample).tobytes(),
            np.array([k.tau0, k.clock_ppm, k.tau_rms], np.float32).tobytes(), k.e.tobytes())


def _by_burst(bursts):
    out = {}
    for b in bursts:
        key = (b.stream, b.chn, b.trig_dec)
        assert key not in out
        out[key] = _sig(b.clock)
    return out


def _check_exact(rx, bursts, rate):
    """every record against the float64 definition on its own channel's plane"""
    mflt = LR.mflt_taps()
    planes = {}
    for b in bursts:
        k = b.clock
        if (b.stream, b.chn) not in planes:
            planes[(b.stream, b.chn)] = rx.debug_dec(b.stream, b.chn)
        x = planes[(b.stream, b.chn)]
        nsym = R.nsym_of(b.nbrow, b.nlbyte)
        assert (k.nsym, k.nseg, k.sym_first_dec) == (nsym, (nsym + 255) // 256, b.end_dec - 8 * (nsym - 1))
        assert 1 <= k.sym_first_dec - b.trig_dec <= 8
        want = R.sums(x, mflt, k.sym_first_dec, nsym)
        assert not k.e[k.nseg:].any()                                   # segments >= nseg: all zero
        for s in range(k.nseg):
            for d in range(8):
                assert math.isclose(k.e[s, d], want[s, d], rel_tol=1e-5), (b.trig_dec, s, d, k.e[s, d], want[s, d])
        # the derived fields: the public function on the record's own sums, to the bit, and the definition in numpy
        assert _sig(demod.symclk_from_sums(k.sym_first_dec, k.nsym, k.e, rate)) == _sig(k)
        tau0, ppm, rms, toa, tau = R.derived(k.sym_first_dec, k.nsym, k.e, rate, mflt)
        assert math.isclose(k.toa_sample, toa, rel_tol=1e-12) and math.isclose(k.tau0, tau0, rel_tol=1e-6, abs_tol=1e-7)
        assert np.allclose(k.tau_s, tau, rtol=0, atol=1e-12)
        if k.nseg == 1:
            assert math.isnan(k.clock_ppm) and math.isnan(k.tau_rms)
        else:
            assert math.isclose(k.clock_ppm, ppm, rel_tol=1e-6, abs_tol=1e-6) and math.isclose(k.tau_rms, rms, rel_tol=1e-6, abs_tol=1e-9)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("rate,fo", [(2_000_000, S.FO8), (10_000_000, S.FO8_10MS)])
def test_symclk_exact_against_definition(built, rate, fo):
    spec = S.eight_channels(rate=rate, fo=fo)
    raw = synth.synth_stream(spec, "cs16")
    with _rx(spec, "cs16", max_push=spec.nsamples, keep_dec=True, symclk=True) as rx:
        rx.push(raw)
        bursts = rx.poll()
        assert len(bursts) >= 10
        _check_exact(rx, bursts, rate)


# transmitted bytes B -> symbols (25 + 8 B + 2) / 3: 92 -> 254 and 93 -> 257 (256 itself is not reachable), 188 -> 510 and 189 -> 513;
# one row with more than 67 data bytes sends 6 parity bytes, so B - 6 payload bytes.  The longest burst the receiver accepts has 8 rows
# with 248 bytes in the last: 1991 payload and 48 parity bytes, 5446 symbols (the 5449 of VDL2GPU_MAXROWS x VDL2GPU_ROWLEN is the
# bound, which no header reaches: 8 x 249 bytes are 9 rows to the receiver); ceil(5446 / 256) = 22 segments all the same.
EDGE_PAYLOADS = (40, 86, 87, 182, 183)
EDGE_NSYM = (126, 254, 257, 510, 513)
LONGEST_PAYLOAD, LONGEST_NSYM = 1991, 5446


@pytest.mark.timeout(300)
def test_symclk_segment_edges(built):
    rng = np.random.default_rng(24)
    bursts, t = [], 0.003
    for n in EDGE_PAYLOADS:
        b = synth.Burst(chan=0, t0=t, info=b"", amp=35.0, cfo=float(rng.uniform(-200, 200)),
                        raw_payload=bytes(rng.integers(0, 256, n, dtype=np.uint8).tolist()))
        bursts.append(b)
        t += b.duration() + 0.003
    bursts.append(synth.Burst(chan=1, t0=0.004, info=b"", amp=30.0, cfo=120.0,
                              raw_payload=bytes(rng.integers(0, 256, LONGEST_PAYLOAD, dtype=np.uint8).tolist())))
    end = max(t, 0.004 + bursts[-1].duration())
    spec = synth.StreamSpec(rate=2_000_000, fo=(100_000, -250_000), nsamples=S._pad(int((end + 0.006) * 2_000_000)), bursts=bursts,
                            noise=1.5, seed=24)
    raw = synth.synth_stream(spec, "cs16")
    with _rx(spec, "cs16", max_push=spec.nsamples, keep_dec=True, symclk=True) as rx:
        rx.push(raw)
        got = sorted(rx.poll(), key=lambda b: (b.chn, b.trig_dec))
        assert [b.clock.nsym for b in got] == list(EDGE_NSYM) + [LONGEST_NSYM]
        assert [b.clock.nseg for b in got] == [1, 1, 2, 2, 3, 22] and lib.SYMCLK_SEGS == 22
        _check_exact(rx, got, spec.rate)
    k = got[2].clock       # 257 symbols: the second segment holds one symbol, its weight in the fit is 1
    assert k.e[1].all() and max(k.e[1]) < max(k.e[0]) / 50


def _cols(b):
    return (b.level, b.soft.tobytes(), b.carrier, b.report, b.fb.tobytes())


@pytest.mark.timeout(300)
def test_symclk_changes_nothing_else(built):
    spec = S.eight_channels()
    raw = synth.synth_stream(spec, "cs16")
    n = raw.size // 2
    buf = (lib.BurstT * 4096)()
    res = []
    for on in (False, True):
        with _rx(spec, "cs16", max_push=1 << 19, frames=True, symclk=on) as rx:
            for s in range(0, n, 1 << 18):
                rx.push(raw[2 * s:2 * min(n, s + (1 << 18))])
            m = rx.poll_raw(buf, 4096)
            res.append((bytes(C.string_at(C.addressof(buf), m * C.sizeof(lib.BurstT))), m, rx.stats(), rx.poll_frames()))
    assert res[0][1] >= 10 and res[0] == res[1]
    # every other column on: each is what it is without symclk
    full = []
    for on in (False, True):
        with _rx(spec, "cs16", max_push=n, frames=True, levels=True, soft_rs=True, carrier=True, block_report=True, feedback=True,
                 symclk=on) as rx:
            rx.push(raw)
            bursts = rx.poll()
            full.append(([(b.key(), b.trig_dec, b.end_dec, b.df) + _cols(b) for b in bursts], rx.poll_frames(), rx.stats()))
            assert all((b.clock is not None) == on for b in bursts)
    assert len(full[0][0]) >= 10 and full[0][1]
    # (NaN levels compare unequal to themselves: through repr)
    assert repr(full[0]) == repr(full[1])


@pytest.mark.timeout(600)
def test_symclk_cut_and_path_invariance(built):
    """whole; in pieces that cut inside bursts (deferred bursts); pushes shorter than VDL2_SERIAL_BELOW (the serial machine);
    VDL2GPU_F_SERIAL; VDL2GPU_F_FULLSCAN: the same records to the bit"""
    spec = synth.random_scenario(2_000_000, S.FO8[:4], 1 << 20, seed=124, bursts_per_s=20.0, info_max=500)
    raw = synth.synth_stream(spec, "cs16")
    n = raw.size // 2
    runs = []
    with _rx(spec, "cs16", max_push=n, symclk=True) as rx:
        runs.append(_by_burst(rx.run(raw, block=n)))
    rng = np.random.default_rng(6)
    with _rx(spec, "cs16", max_push=1 << 18, symclk=True) as rx:
        got, s = [], 0
        while s < n:
            e = min(n, s + int(rng.integers(100_000, 1 << 18)))       # >= VDL2_SERIAL_BELOW frames each: the parallel path, cut anywhere
            rx.push(raw[2 * s:2 * e])
            got += rx.poll_ready()
            s = e
        got += rx.poll()
        deferred = rx.stats()["deferrals"]
        runs.append(_by_burst(got))
    assert deferred >= 1
    with _rx(spec, "cs16", max_push=32768, symclk=True) as rx:       # 1376 frames a push, below VDL2_SERIAL_BELOW = 4096
        runs.append(_by_burst(rx.run(raw, block=32768)))
    for kw in ({"serial": True}, {"full_scan": True}):
        with _rx(spec, "cs16", max_push=1 << 18, symclk=True, **kw) as rx:
            runs.append(_by_burst(rx.run(raw)))
    assert len(runs[0]) >= 10 and any(sig[2] >= 2 for sig in runs[0].values())
    for r in runs[1:]:
        assert r == runs[0]


@pytest.mark.timeout(300)
def test_symclk_three_streams(built):
    specs = [S.eight_channels(seed=8 + s) for s in range(3)]
    n = min(sp.nsamples for sp in specs)
    raw = np.stack([synth.synth_stream(sp, "cs16")[:2 * n] for sp in specs])
    with _rx(specs[0], "cs16", nstreams=3, max_push=n, keep_dec=True, symclk=True) as rx:
        rx.push(raw)
        bursts = rx.poll()
        assert len({b.stream for b in bursts}) == 3
        _check_exact(rx, bursts, specs[0].rate)


@pytest.mark.timeout(300)
def test_symclk_api_edges(built):
    spec = S.eight_channels()
    raw = synth.synth_stream(spec, "cu8")
    buf = (lib.BurstT * 4096)()
    kv = (lib.SymClkT * 4096)()
    with _rx(spec, "cu8", max_push=spec.nsamples) as rx:        # no F_SYMCLK
        rx.push(raw)
        assert rx.L.vdl2gpu_poll_symclk(rx.h, buf, None, None, None, None, None, kv, 4096) == EINVAL
        assert rx.L.vdl2gpu_poll_symclk_ready(rx.h, buf, None, None, None, None, None, kv, 4096) == EINVAL
        assert b"clk needs VDL2GPU_F_SYMCLK" in rx.L.vdl2gpu_last_error(rx.h)
        n = rx.poll_symclk_raw(buf, None, None, None, None, None, None, 4096)       # clk == NULL: the plain poll; nothing was consumed above
        plain = [bytes(C.string_at(C.addressof(buf[i]), C.sizeof(lib.BurstT))) for i in range(n)]
    with _rx(spec, "cu8", max_push=spec.nsamples) as rx:
        rx.push(raw)
        m = rx.poll_raw(buf, 4096)
        assert plain == [bytes(C.string_at(C.addressof(buf[i]), C.sizeof(lib.BurstT))) for i in range(m)] and n >= 10
    with _rx(spec, "cu8", max_push=spec.nsamples, symclk=True) as rx:
        rx.push(raw)
        want = _by_burst(rx.poll())
    with _rx(spec, "cu8", max_push=spec.nsamples, symclk=True) as rx:
        rx.push(raw)
        lv = (lib.LevelT * 4)()
        assert rx.L.vdl2gpu_poll_symclk(rx.h, buf, lv, None, None, None, None, kv, 4) == EINVAL     # another column the handle lacks
        got, plain_keys = {}, []
        for turn in range(10000):
            if turn % 2:
                k = rx.poll_symclk_raw(buf, None, None, None, None, None, kv, 3)
                for i in range(k):
                    got[(buf[i].stream, buf[i].chn, buf[i].trig_dec)] = _sig(demod.SymClock.from_c(kv[i], spec.rate))
            else:
                k = rx.poll_raw(buf, 2)
                plain_keys += [(buf[i].stream, buf[i].chn, buf[i].trig_dec) for i in range(k)]
            if k == 0 and turn > 2:
                break
    assert not set(got) & set(plain_keys)
    assert set(got) | set(plain_keys) == set(want) and len(got) + len(plain_keys) == len(want)
    assert all(got[k] == want[k] for k in got) and len(got) >= 4


@pytest.mark.timeout(300)
def test_symclk_physics(built):
    """Bursts at a random fraction of a symbol with the transmitter's symbol clock 0, +50 and -30 ppm off: toa_sample against the true
    centre of the first symbol behind the unique word, clock_ppm against sym_ppm, within twice the worst error of the model's table
    (symclk_ref.B_*: profiles/r24_symclk_accuracy.txt)."""
    rng = np.random.default_rng(2024)
    fo = (100_000, -150_000, 300_000)
    bursts = []
    for c, ppm in enumerate(R.PPMS):
        t = 0.003 + float(rng.uniform(0, 1 / 10500))
        for n in (900, 300):       # about 2540 symbols (10 segments) and 870 (4 segments)
            b = synth.Burst(chan=c, t0=t, info=bytes(rng.integers(0, 256, n, dtype=np.uint8).tolist()), amp=30.0,
                            cfo=float(rng.uniform(-300, 300)), sym_ppm=ppm)
            bursts.append(b)
            t += b.duration() + 0.003 + float(rng.uniform(0, 1 / 10500))
    end = max(b.t0 + b.duration() for b in bursts)
    spec = synth.StreamSpec(rate=2_000_000, fo=fo, nsamples=S._pad(int((end + 0.006) * 2_000_000)), bursts=bursts, noise=1.7, seed=2024)
    with _rx(spec, "cs16", max_push=spec.nsamples, symclk=True) as rx:
        got = sorted(rx.run(synth.synth_stream(spec, "cs16")), key=lambda b: (b.chn, b.trig_dec))
    assert len(got) == len(bursts)
    for b, tx in zip(got, bursts):
        k = b.clock
        truth = (tx.t0 + R.UW_SYMBOLS / (10500.0 * (1 + tx.sym_ppm * 1e-6))) * spec.rate
        err_us = (k.toa_sample - truth) / spec.rate * 1e6
        print(f"chn {b.chn} nsym {k.nsym} nseg {k.nseg} sym_ppm {tx.sym_ppm:+.0f}: toa error {err_us:+.4f} us, clock_ppm {k.clock_ppm:+.3f}, tau_rms {k.tau_rms:.4f}")
        assert abs(err_us) <= R.B_TOA_US, (b.chn, k.nsym, err_us)
        assert k.nseg >= 3
        assert abs(k.clock_ppm - tx.sym_ppm) <= (R.B_PPM_LONG if k.nseg >= 10 else R.B_PPM_MID), (b.chn, k.nsym, k.clock_ppm, tx.sym_ppm)
    assert {k.clock.nseg >= 10 for k in got} == {True, False}
