"""VDL2GPU_F_CARRIER on the GPU: the flag changes nothing else; the sums are the definition's (tests/carrier_ref.py, on the oracle's
tap and pinned by the oracle's bytes) for every burst on every decode path, push cut, geometry and stream epoch; the record stays
beside its burst through a full record ring and a compacted host queue; and the frequency the host derives is the transmitted one.

2 MS/s cs16 unless said otherwise; a model is computed once per process and shared by the tests that use it."""
import ctypes as C

import numpy as np
import pytest

import carrier_ref as CR
import epoch_rule as E
import geom_craft as G
import scenarios as S
import test_gpu_epoch as TE
import test_gpu_full as TF
from test_carrier_abi import B_HZ, physics_model
from test_gpu_chain import PART, _env, _push_parts
from test_gpu_planes import _rx as _rx_identity
from vdlm2dec_amd import lib, synth

pytestmark = pytest.mark.gpu

RATE = 2_000_000
_cache = {}


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _rx(fo, rate=RATE, fmt="cs16", plans=None, **kw):
    from vdlm2dec_amd.demod import Receiver, plan_channels
    return Receiver(rate, plans or plan_channels(S.FC, fo), fmt=fmt, **kw)


def _paths_scenario():
    """the scenario of test_gpu_soft.test_maps_equal_the_model: 4 channels, seed 93, noise 6 -- (spec, raw, model)"""
    def make():
        spec = synth.random_scenario(RATE, S.FO8[:4], 1 << 20, seed=93, bursts_per_s=25.0, info_max=300, noise=6.0)
        raw = synth.synth_stream(spec, "cs16")
        return spec, raw, CR.stream_sums(raw, "cs16", RATE, spec.fo, S.FC)
    return _cached("paths", make)


def _fields(c):
    return (c.nsym, c.sum_e, c.sum_e2, c.dphi, c.freq_hz, c.ppm, c.rms_rad)


def _record(b):
    """what a burst's carrier record holds, comparable"""
    return _fields(b.carrier)


def _check(bursts, want, least=5, shift=0):
    """every burst has the model's sums and the helper's floats; want: {(stream, chn, trig_dec): (oracle Block, sums)}; shift: the
    frames the records' stamps are moved by (a stream epoch)"""
    from vdlm2dec_amd.demod import carrier_from_sums
    assert len(bursts) == len(want) >= least, (len(bursts), len(want))
    assert len({(b.stream, b.chn, b.trig_dec) for b in bursts}) == len(bursts)
    for b in bursts:
        blk, sums = want[(b.stream, b.chn, b.trig_dec - shift)]
        assert b.data == blk.data, (b.stream, b.chn, b.trig_dec)
        assert b.carrier is not None and _record(b)[:3] == sums, (b.stream, b.chn, b.trig_dec, b.carrier, sums)
        assert sums[0] == (25 + 8 * sum(G.takes(b.nbrow, b.nlbyte)) - 1) // 3 - 7
        assert _record(b) == _fields(carrier_from_sums(b.df, b.Fr, *sums))
        assert abs(b.carrier.sum_e) <= 16 * sums[0] and sums[2] <= 256 * sums[0]


# ================================================================================================ 1. nothing else changes
@pytest.mark.timeout(300)
@pytest.mark.parametrize("fmt,rate,fo", [("cu8", 2_000_000, S.FO8), ("cs16", 10_000_000, S.FO8_10MS)])
def test_carrier_changes_nothing_else(built, fmt, rate, fo):
    """bursts, levels, maps, stats and frames are byte-identical with the flag off and on"""
    spec = S.eight_channels(rate=rate, fo=fo)
    raw = synth.synth_stream(spec, fmt)
    res = []
    for car in (False, True):
        with _rx(fo, rate, fmt, max_push=1 << 18, frames=True, levels=True, soft_rs=True, carrier=car) as rx:
            rng = np.random.default_rng(3)
            s, n = 0, raw.size // 2
            while s < n:
                e = min(n, s + int(rng.integers(5000, 1 << 18)))
                rx.push(raw[2 * s:2 * e])
                s = e
            k = 1 << 12
            buf, lv, sv = (lib.BurstT * k)(), (lib.LevelT * k)(), (lib.SoftT * k)()
            cv = (lib.CarrierT * k)() if car else None
            m = rx.poll_carrier_raw(buf, lv, sv, cv, k) if car else rx.poll_soft_raw(buf, lv, sv, k)
            res.append((bytes(C.string_at(C.addressof(buf), m * C.sizeof(lib.BurstT))),
                        bytes(C.string_at(C.addressof(lv), m * C.sizeof(lib.LevelT))),
                        bytes(C.string_at(C.addressof(sv), m * C.sizeof(lib.SoftT))), m, rx.stats(), rx.poll_frames()))
            if car:
                assert all(cv[i].nsym > 0 and cv[i].reserved == 0 for i in range(m))
    assert res[0][3] >= 10
    assert res[0] == res[1]


# ================================================================================================ 2. exact against the model
@pytest.mark.timeout(600)
@pytest.mark.parametrize("kw", [{}, {"serial": True}, {"full_scan": True}, {"flags": lib.F_TEST_NOREGION}],
                         ids=["default", "serial", "fullscan", "repairs"])
def test_sums_equal_the_model(built, oracle, kw):
    spec, raw, want = _paths_scenario()
    with _rx(spec.fo, max_push=1 << 18, carrier=True, **kw) as rx:
        got = rx.run(raw)
        st = rx.stats()
    if kw.get("flags"):
        assert st["repairs"] + st["serial_redos"] > 0, st
    _check(got, want)


# ================================================================================================ 3. several streams
@pytest.mark.timeout(600)
def test_three_streams_with_distinct_plans(built, oracle):
    from vdlm2dec_amd.demod import plan_channels
    ins = S.distinct_streams(3, nsamples=1 << 19)
    want = {}
    for s, (r, fo, fc) in enumerate(ins):
        want.update(CR.stream_sums(r, "cs16", RATE, fo, fc, stream=s))
    raw = np.stack([r for r, _, _ in ins])
    with _rx(None, plans=[plan_channels(fc, fo) for _, fo, fc in ins], max_push=1 << 18, carrier=True) as rx:
        got = rx.run(raw)
    _check(got, want)
    assert {b.stream for b in got} == {0, 1, 2}
    assert len({b.Fr for b in got}) > 8        # every stream its own channel frequencies: its own ppm for the same offset


# ================================================================================================ 4. push cuts
@pytest.mark.timeout(600)
def test_records_do_not_depend_on_the_push_cut(built, oracle):
    spec, raw, want = _paths_scenario()
    n = raw.size // 2
    runs = []
    for block in (n, 32768):
        with _rx(spec.fo, max_push=block, carrier=True) as rx:
            runs.append({(b.chn, b.trig_dec): _record(b) for b in rx.run(raw, block=block)})
    with _rx(spec.fo, max_push=1 << 18, carrier=True) as rx:
        rng = np.random.default_rng(5)
        s, got = 0, []
        while s < n:
            e = min(n, s + int(rng.integers(1000, 1 << 18)))
            rx.push(raw[2 * s:2 * e])
            got += rx.poll_ready()
            s = e
        got += rx.poll()
        runs.append({(b.chn, b.trig_dec): _record(b) for b in got})
        _check(got, want)
    assert len(runs[0]) == len(want) >= 5
    assert runs[1] == runs[0] and runs[2] == runs[0]


# ================================================================================================ 5. geometry edges
def _plane_model(name):
    def make():
        j = G.judge(name)
        return {(0, 0, b.trig_dec): (b, sums) for b, sums in CR.tap_sums(j.dec, j.triggers, j.blocks)}
    return _cached(("plane", name), make)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("path", ("default", "noregion-r0"))
def test_every_geometry(built, oracle, monkeypatch, path):
    """tests/geom_craft.py's sweep: nbrow 1 .. 8 x the last row's byte counts either side of every parity threshold (nlbyte 0, <= 2,
    <= 30, <= 67, above), every timing class -- through K2d's kernel, and with the region
    scan dropped and no repair round through the serial machine's payload path (K2f redoes the channel)"""
    kw = _env(monkeypatch, path)
    j = G.judge("geom")
    raw = j.plane.raw()
    with _rx_identity(PART, kw, carrier=True) as rx:
        for _ in _push_parts(rx, raw):
            pass
        got = rx.poll()
        st = rx.stats()
    assert st["bursts"] == len(j.blocks) and st["overflowed"] == 0
    if path != "default":
        assert st["serial_redos"] > 0, st
    _check(got, _plane_model("geom"), least=100)
    seen = {(b.nbrow, b.nlbyte) for b in got}
    assert seen >= set(G.geometries())
    for lo, hi in ((0, 0), (1, 2), (3, 30), (31, 67), (68, 248)):
        assert any(lo <= n <= hi for _, n in seen), (lo, hi)
    assert {1, 8} <= {r for r, _ in seen}


@pytest.mark.timeout(300)
def test_a_burst_decoded_in_the_push_after_its_trigger(built, oracle, monkeypatch):
    """geom_craft's edge_cut plane: a burst's last symbol, header and trigger walked across the end of a push frame by frame"""
    F = 5000
    kw = _env(monkeypatch, "default")
    j = G.judge(f"edge_cut:{F}")
    with _rx_identity(2 * F, kw, carrier=True) as rx:
        got = rx.run(j.plane.raw(), block=2 * F)
        st = rx.stats()
    assert st["bursts"] == len(j.blocks) and st["deferrals"] > 0
    _check(got, _plane_model(f"edge_cut:{F}"), least=50)
    assert min(G.sent_bytes(b.nbrow, b.nlbyte) for b in got) == G.SHORTEST      # the shortest burst a header may announce


# ================================================================================================ 6. a stream epoch
@pytest.mark.timeout(300)
def test_sums_past_two_to_the_32_samples(built, oracle, monkeypatch):
    """VDL2GPU_TEST_EPOCH: the stream crosses 2^32 input samples with a burst in flight; the sums are the unshifted run's (and the model's)"""
    ref = TE._two(oracle)
    blk, t0 = TE._epoch(ref, "in32")
    sizes = TE._ragged(ref, blk)
    want = {}
    for c in ref.dec:
        for b, sums in CR.tap_sums(ref.dec[c], ref.trig[c], [b for b in ref.blocks if b.chn == c]):
            want[(0, c, b.trig_dec)] = (b, sums)
    runs = []
    for epoch in (0, t0):
        TE._env(monkeypatch, epoch)
        if not epoch:
            monkeypatch.delenv("VDL2GPU_TEST_EPOCH")
        with TE._rx(ref, max(sizes), carrier=True) as rx:
            _, got = TE._pushed(rx, ref, sizes, every=False)
            assert rx.stats()["samples_in"] == epoch + ref.n
        d0 = E.d0(epoch, ref.clk)
        _check(got, want, least=3, shift=d0)
        runs.append({(b.chn, b.trig_dec - d0): _record(b) for b in got})
    assert t0 < 1 << 32 < t0 + ref.n and runs[0] == runs[1]


# ================================================================================================ 7. API edges
@pytest.mark.timeout(300)
def test_car_needs_the_flag_and_null_columns_are_a_plain_poll(built, oracle):
    spec, raw, want = _paths_scenario()
    k = 4096
    size = C.sizeof(lib.BurstT)
    with _rx(spec.fo, max_push=1 << 18, levels=True) as rx:          # no VDL2GPU_F_CARRIER
        for s in range(0, raw.size // 2, 1 << 18):
            rx.push(raw[2 * s:2 * (s + (1 << 18))])
        rx.sync()
        buf, cv = (lib.BurstT * k)(), (lib.CarrierT * k)()
        for fn in (rx.L.vdl2gpu_poll_carrier, rx.L.vdl2gpu_poll_carrier_ready):
            assert fn(rx.h, buf, None, None, cv, k) == -1             # VDL2GPU_EINVAL ...
            assert b"VDL2GPU_F_CARRIER" in rx.L.vdl2gpu_last_error(rx.h)
        with pytest.raises(lib.Vdl2GpuError):
            rx.poll_carrier_raw(buf, None, None, cv, k)
        m = rx.poll_raw(buf, k)                                       # ... and nothing was consumed
        assert m == len(want)
        plain = bytes(C.string_at(C.addressof(buf), m * size))
    with _rx(spec.fo, max_push=1 << 18, carrier=True) as rx:
        for s in range(0, raw.size // 2, 1 << 18):
            rx.push(raw[2 * s:2 * (s + (1 << 18))])
        buf = (lib.BurstT * k)()
        lv = (lib.LevelT * k)()
        assert rx.L.vdl2gpu_poll_carrier(rx.h, buf, lv, None, None, k) == -1      # lv on a handle without VDL2GPU_F_LEVELS, as ever
        m = rx.poll_carrier_raw(buf, None, None, None, k)             # all three NULL: vdl2gpu_poll
        assert m == len(want) and bytes(C.string_at(C.addressof(buf), m * size)) == plain
        assert rx.poll_carrier_raw(buf, None, None, None, k) == 0


@pytest.mark.timeout(300)
def test_record_ring_full_keeps_car_with_its_burst(built, oracle):
    """tests/test_gpu_full.py's ring scenario with max_bursts = 5: the busy push overfills the ring; what is delivered has its own sums"""
    scn = TF._scn("ring", oracle)
    got, _, stats = TF._run_ring(scn, max_bursts=5, carrier=True)
    TF._check_ring(scn, got, stats, 5)
    assert stats[-1]["overflowed"] > 0
    want = _cached("ring", lambda: CR.stream_sums(scn.raw, "cs16", RATE, scn.fo, S.FC))
    delivered = [b for g in got for b in g]
    _check(delivered, {(0, b.chn, b.trig_dec): want[(0, b.chn, b.trig_dec)] for b in delivered})


def _bite(rx, k):
    """ONE vdl2gpu_poll_carrier of at most k records"""
    from vdlm2dec_amd.demod import Burst, Carrier
    buf, cv = (lib.BurstT * k)(), (lib.CarrierT * k)()
    n = rx.poll_carrier_raw(buf, None, None, cv, k)
    return [Burst(b.stream, b.chn, b.Fr, b.nbrow, b.nlbyte, b.df, b.ppm, b.trig_dec, b.end_dec, b.trig_sample, b.end_sample, bytes(b.data),
                  carrier=Carrier.from_c(cv[i])) for i, b in ((i, buf[i]) for i in range(n))]


NSTREAMS = 12


@pytest.mark.timeout(600)
def test_burst_queue_compaction_carries_the_carrier_records(built, oracle, monkeypatch):
    """test_gpu_full.test_burst_queue_compaction_carries_levels_and_maps' method: a consumer of small bites, more than 1024 records handed
    out and others waiting when a push is collected, five records a push in a slab and the others through the bounce buffer
    (VDL2GPU_SLAB_CAP = 5): every waiting record moves with its carrier record.  One recording of 3 << 17 samples goes to 12 streams,
    turned by another number of samples for each, so that neighbours in the hand-out order are different bursts."""
    rng = np.random.default_rng(4242)
    nsamp, bursts = 3 << 17, []
    for c in range(8):
        t = 0.002 + 0.0013 * c
        while True:
            b = synth.Burst(chan=c, t0=t, info=bytes(rng.integers(0, 256, int(rng.integers(1, 9)), dtype=np.uint8).tolist()),
                            amp=float(rng.uniform(15, 50)), cfo=float(rng.uniform(-300, 300)))
            if t + b.duration() + 0.002 > nsamp / RATE:
                break
            bursts.append(b)
            t += b.duration() + 0.002
    spec = synth.StreamSpec(rate=RATE, fo=S.FO8, nsamples=nsamp, bursts=bursts, seed=4242)
    base = synth.synth_stream(spec, "cs16")
    sizes = [nsamp // 16] * 16
    scns = [TF._Scn(oracle, spec, sizes, margin=0, raw=np.roll(base, 2 * 24571 * s)) for s in range(NSTREAMS)]
    order = sorted(((b.end_dec, s, b.chn), TF._key(b, s)) for s, scn in enumerate(scns) for b in scn.want)
    counts = [sum(len(scn.per_push[k]) for scn in scns) for k in range(16)]
    bite = 85
    assert len(order) > 1024 + 2 * bite and TF._compactions(counts, bite) >= 1, (len(order), counts)
    monkeypatch.setenv("VDL2GPU_SLAB_CAP", "5")
    raw = np.stack([scn.raw for scn in scns])
    with TF._rx(scns[0], nstreams=NSTREAMS, carrier=True, testhooks=True) as rx:
        got = []
        for chunk in scns[0].pushes(raw):
            rx.push(chunk)
            got += _bite(rx, bite)
        handed = len(got)
        got += rx.poll()
        st = rx.stats()
    print(f"burst compaction: oracle {len(order)} ({counts} a push), {handed} handed out in bites of {bite}, then {len(got) - handed}")
    assert st["overflowed"] == 0
    assert [TF._key(b) for b in got] == [k for _, k in order]
    want = {}
    for s, scn in enumerate(scns):
        want.update(CR.stream_sums(scn.raw, "cs16", RATE, scn.fo, S.FC, stream=s))
    _check(got, want)


# ================================================================================================ 8. physics
@pytest.mark.timeout(300)
def test_freq_hz_is_the_transmitted_offset(built, oracle):
    """Bursts with known cfo in +-400 Hz at noise 1.7 (carrier_ref.physics_spec).  The model alone, on the CPU
    (tests/test_carrier_abi.py::test_physics_on_the_cpu): 22 bursts, 21 with rms_rad < 0.1, the worst of those 2.026 Hz off;
    B = 4.052 Hz is twice that.  Every burst with rms_rad < 0.1 must be within B, and the rms error at most a fifth of the
    one-shot estimate's (10500 df / 2 pi + 656.25): the model gives 0.76 Hz against 9.0 Hz."""
    spec, raw, rows = physics_model()
    model = {(c, t): (cfo, f, r) for c, t, cfo, f, r, _ in rows}
    with _rx(spec.fo, max_push=1 << 18, carrier=True) as rx:
        got = rx.run(raw)
    assert len(got) == len(rows) >= 15
    err, one = [], []
    for b in got:
        cfo, f, r = model[(b.chn, b.trig_dec)]
        print(f"chn {b.chn} trig {b.trig_dec}: cfo {cfo:+8.2f} freq_hz {b.carrier.freq_hz:+8.2f} rms_rad {b.carrier.rms_rad:.4f} "
              f"one-shot {10500.0 * b.df / (2 * np.pi) + 656.25:+8.2f}")
        assert np.float32(f) == np.float32(b.carrier.freq_hz) and np.float32(r) == np.float32(b.carrier.rms_rad)
        if b.carrier.rms_rad < 0.1:
            assert abs(b.carrier.freq_hz - cfo) <= B_HZ, (b.chn, b.trig_dec, b.carrier, cfo)
        err.append(b.carrier.freq_hz - cfo)
        one.append(10500.0 * b.df / (2 * np.pi) + 656.25 - cfo)
    assert sum(b.carrier.rms_rad >= 0.1 for b in got) <= 0.1 * len(got)
    e, o = np.sqrt(np.mean(np.square(err))), np.sqrt(np.mean(np.square(one)))
    print(f"rms error {e:.3f} Hz, one-shot {o:.3f} Hz, ratio {o / e:.1f}")
    assert e <= o / 5


# ================================================================================================ 9. closing the loop
@pytest.mark.timeout(300)
def test_feeding_freq_hz_back_into_fo(built, oracle):
    """Every burst transmitted 300 Hz high.  A plain handle reports it; an exact-Fo handle whose offsets are moved by the rounded
    median reads a median |freq_hz| within B (4.052 Hz, see test_freq_hz_is_the_transmitted_offset)."""
    from vdlm2dec_amd.demod import ThreadParam, plan_channels
    spec, raw, rows = physics_model(300.0)
    with _rx(spec.fo, max_push=1 << 18, carrier=True) as rx:
        first = rx.run(raw)
    assert len(first) == len(rows) >= 15
    med = float(np.median([b.carrier.freq_hz for b in first]))
    assert abs(med - 300.0) <= B_HZ
    plan = [ThreadParam(p.chn, p.Fr, p.Fo + round(med)) for p in plan_channels(S.FC, spec.fo)]
    with _rx(None, plans=plan, max_push=1 << 18, carrier=True, exact_fo=True) as rx:
        second = rx.run(raw)
    assert len(second) >= 15
    left = float(np.median([abs(b.carrier.freq_hz) for b in second]))
    print(f"median freq_hz {med:+.2f} Hz; with Fo + {round(med)}: median |freq_hz| {left:.2f} Hz")
    assert left <= B_HZ
