"""The output path when it is full (include/vdl2gpu.h): the device record ring (max_bursts), the host queues'
bound of 4 x max_bursts and the compaction of the storage behind them, the frame arena.  What is dropped is counted, never silent,
and what is handed out is exact: every expectation is the oracle's over the same IQ (oracle.run_oracle, oracle.frames_of_block,
and the level / reliability models tests/levels_ref.py and tests/soft_ref.py).

2 MS/s cs16, at most 1 << 21 samples of IQ per scenario, cut into a few pushes.  Every scenario builder asserts on the CPU what the
oracle makes of its recording -- bursts and frames per push, which frames exceed a slot --, so a change in synth cannot turn a test
into one that checks nothing.  A scenario is made once and shared by the tests that use it."""
import bisect
import collections
import ctypes as C
import math

import numpy as np
import pytest

import blocks_craft as K
import levels_ref as LR
import scenarios as S
import soft_ref as SR
from vdlm2dec_amd import lib, synth

pytestmark = pytest.mark.gpu

RATE = 2_000_000
SDRCLK = RATE // 4000       # the default (rtl.c:37)
MARGIN = 4000               # input samples (2 ms) no burst of a scenario with per-push expectations ends within of a cut
HDR = 56                    # offsetof(vdl2gpu_frame_t, data)
SLOT = 256                  # K4_SLOT: a record's own frame slot


def _end_sample(end_dec: int) -> int:
    """the input sample that completes the 84 kS/s output end_dec (dec_to_sample of vdl2gpu.hip; d8psk.c:374-381)"""
    return ((end_dec + 1) * SDRCLK + 20) // 21 - 1


def _entry(n: int) -> int:
    """bytes a frame of n bytes takes in the arena"""
    return (HDR + n + 7) & ~7


def _dfbits(df) -> int:
    return int(np.float32(df).view(np.uint32))


def _key(b, stream=None):
    """full key of a burst record, the oracle's or the library's"""
    return (b.stream if stream is None else stream, b.chn, b.nbrow, b.nlbyte, b.data, _dfbits(b.df))


def _exact_subset(got, want):
    """the delivered items, as a multiset, are contained in the oracle's: nothing twice, nothing invented"""
    extra = collections.Counter(got) - collections.Counter(want)
    assert not extra, f"{sum(extra.values())} delivered items the oracle does not have (or has fewer times); lengths " \
                      f"{sorted(len(k[-1]) if isinstance(k[-1], bytes) else len(k[-2]) for k in extra)[:20]}"


def _in_time_order(bursts):
    last = {}
    for b in bursts:
        assert last.get((b.stream, b.chn), -1) < b.end_dec, (b.stream, b.chn, b.end_dec)
        last[(b.stream, b.chn)] = b.end_dec


class _Scn:
    """a recording, its cut into pushes and what the oracle makes of it: want = the bursts in hand-out order (end_dec, chn),
    per_push[k] = those the k-th push completes.  margin: no burst may end that close to a cut (0: not checked -- the scenario does
    not depend on which push a burst near a cut comes out of)"""

    def __init__(self, oracle, spec, sizes, margin=MARGIN, raw=None):
        self.fo, self.sizes = tuple(spec.fo), list(sizes)
        self.cuts = np.cumsum(sizes).tolist()
        assert self.cuts[-1] == spec.nsamples <= 1 << 21
        self.raw = synth.synth_stream(spec, "cs16") if raw is None else raw
        self.want = sorted(oracle.run_oracle(self.raw, "cs16", RATE, self.fo, S.FC), key=lambda b: (b.end_dec, b.chn))
        self.per_push = [[] for _ in sizes]
        for b in self.want:
            s = _end_sample(b.end_dec)
            assert all(abs(s - c) > margin for c in self.cuts[:-1]) or not margin, f"a burst ends {s}, too close to a cut"
            self.per_push[bisect.bisect_right(self.cuts, s)].append(b)
        self.frames = {id(b): oracle.frames_of_block(b.nbrow, b.nlbyte, b.data, cap=1 << 16) for b in self.want}

    def pushes(self, raw=None):
        raw, s = self.raw if raw is None else raw, 0
        for n in self.sizes:
            yield raw[..., 2 * s:2 * (s + n)]
            s += n

    def want_frames(self, bursts=None):
        """(stream 0, chn, hdata) in hand-out order (end_dec, chn, seq)"""
        return [(0, b.chn, f) for b in (self.want if bursts is None else bursts) for f in self.frames[id(b)]]


_scenarios = {}


def _scn(name, oracle):
    if name not in _scenarios:
        _scenarios[name] = {"ring": _ring_scenario, "bound": _bound_scenario, "arena": _arena_scenario,
                            "many_frames": _many_frames_scenario}[name](oracle)
    return _scenarios[name]


def _rx(scn, nstreams=1, **kw):
    from vdlm2dec_amd.demod import Receiver, plan_channels
    plan = plan_channels(S.FC, scn.fo)
    return Receiver(RATE, [plan] * nstreams if nstreams > 1 else plan, fmt="cs16", max_push=max(scn.sizes), **kw)


# ------------------------------------------------------------------------------------------------ the level and soft models
def _models(oracle, raw, fo, stream=0):
    """{(stream, chn, trig_dec): (oracle Block, reliability map, (sym_first_dec, nsym, subphase, sig, noise, noise_blocks))}"""
    mflt, pn, out = LR.mflt_taps(), SR.pn_bits(), {}
    for c, f in enumerate(fo):
        ch = oracle.OracleChannel(RATE, f, S.FC + f, chn=c, tap_dec=True)
        ch.feed(raw, "cs16")
        x, trigs, blocks = ch.dec(), ch.triggers(), ch.blocks()
        ch.close()
        clk = {t["dec_index"]: t["clk"] for t in trigs if t["accepted"] == 1}
        for b in blocks:
            hard, rel = SR.soft_block(x, b.nbrow, b.nlbyte, b.df, b.trig_dec, clk[b.trig_dec], pn)
            assert hard.tobytes() == b.data
            j0, rb = SR.timing(clk[b.trig_dec])
            nsym = SR.geom(b.nbrow, b.nlbyte)[6]
            out[(stream, c, b.trig_dec)] = (b, rel, (b.trig_dec + j0, nsym, rb) + LR.levels(x, mflt, b.trig_dec + j0, nsym, rb))
    return out


def _check_level_and_map(b, model, k_scale):
    """the burst's level record and reliability map are its own (compared as tests/test_gpu_levels.py and test_gpu_soft.py do)"""
    blk, rel, (first, nsym, sub, sig, noise, nb) = model[(b.stream, b.chn, b.trig_dec)]
    assert b.data == blk.data and b.end_dec == blk.end_dec
    assert b.soft is not None and np.array_equal(b.soft, rel), (b.stream, b.chn, b.trig_dec)
    L = b.level
    assert (L.sym_first_dec, L.nsym, L.subphase, L.noise_blocks) == (first, nsym, sub, nb), (b.stream, b.chn, b.trig_dec, L)
    assert L.sym_first_dec + 8 * (L.nsym - 1) == b.end_dec
    assert math.isclose(L.sig_power, sig, rel_tol=1e-5), (b.trig_dec, L, sig)
    assert math.isclose(L.sig_dbfs, 10 * math.log10(sig / k_scale), abs_tol=1e-4)
    if nb:
        assert math.isclose(L.noise_power, noise, rel_tol=1e-5), (b.trig_dec, L, noise)
        assert math.isclose(L.noise_dbfs, 10 * math.log10(noise / k_scale), abs_tol=1e-4)
    else:
        assert math.isnan(L.noise_power) and math.isnan(L.noise_dbfs)


def _bite(rx, k):
    """ONE vdl2gpu_poll_soft of at most k records (Receiver.poll keeps calling until the queue is empty)"""
    from vdlm2dec_amd.demod import Burst, Level
    buf = (lib.BurstT * k)()
    lv = (lib.LevelT * k)() if rx.levels else None
    sv = (lib.SoftT * k)() if rx.soft_rs else None
    n = rx.poll_soft_raw(buf, lv, sv, k)
    return [Burst(b.stream, b.chn, b.Fr, b.nbrow, b.nlbyte, b.df, b.ppm, b.trig_dec, b.end_dec, b.trig_sample, b.end_sample,
                  bytes(b.data), Level.from_c(lv[i]) if lv is not None else None,
                  np.frombuffer(bytes(sv[i].rel), np.uint8).reshape(8, 255).copy() if sv is not None else None)
            for i, b in ((i, buf[i]) for i in range(n))]


def _bite_frames(rx, k):
    buf = (lib.FrameT * k)()
    n = rx._check(rx.L.vdl2gpu_poll_frames(rx.h, buf, k))
    return [(buf[i].stream, buf[i].chn, bytes(buf[i].data[:buf[i].len])) for i in range(n)]


# ================================================================================================ a. the record ring (max_bursts)
def _ring_scenario(oracle):
    """3 channels, 3 pushes: a busy second push (N2 >= 12 bursts) between two that complete at most 5 each -- what is left of a
    random scenario once the first and third push have been thinned to one burst a channel (a burst that begins in one push and
    ends in the next belongs to the next, and stays)"""
    step = 3 << 17
    spec = synth.random_scenario(RATE, S.FO8[:3], 3 * step, seed=2611, bursts_per_s=45.0, info_max=60)
    keep, seen = [], collections.Counter()
    for b in spec.bursts:
        end = (b.t0 + b.duration()) * RATE
        if any(abs(end - c) < 3 * MARGIN for c in (step, 2 * step)):
            continue
        k = min(2, int(end // step))
        seen[(k, b.chan)] += 1
        if k == 1 or seen[(k, b.chan)] == 1:
            keep.append(b)
    spec.bursts = keep
    scn = _Scn(oracle, spec, [step] * 3)
    n = [len(p) for p in scn.per_push]
    assert 2 <= n[0] <= 5 and n[1] >= 12 and 2 <= n[2] <= 5, n
    assert len(scn.want) == len(keep) and len({_key(b, 0) for b in scn.want}) == len(scn.want)
    assert all(len(scn.frames[id(b)]) == 1 for b in scn.want)
    assert len({f for fs in scn.frames.values() for f in fs}) == len(scn.want)       # a frame names its burst
    return scn


def _run_ring(scn, **kw):
    """push by push, polling after each: per push the bursts, the frames (frames=True) and the counters behind it"""
    frames_on = kw.get("frames", False)
    with _rx(scn, **kw) as rx:
        got, frames, stats = [], [], []
        for chunk in scn.pushes():
            rx.push(chunk)
            if frames_on:
                frames.append(rx.poll_frames())
            got.append(rx.poll())
            stats.append(rx.stats())
    return got, frames, stats


def _check_ring(scn, got, stats, cap, exact=True):
    """exact: the run has no repair and no serial redo -- no void record takes a slot, so the accounting is an equality and a push
    within the ring's capacity comes out whole"""
    st = stats[-1]
    n = [len(p) for p in scn.per_push]
    print(f"max_bursts {cap}: oracle {n}, delivered {[len(g) for g in got]}, overflowed {[s['overflowed'] for s in stats]}, "
          f"repairs {st['repairs']}, serial_redos {st['serial_redos']}")
    delivered = [b for g in got for b in g]
    assert all(len(g) <= cap for g in got)
    _exact_subset([_key(b) for b in delivered], [_key(b, 0) for b in scn.want])
    _in_time_order(delivered)
    assert len(delivered) + st["overflowed"] >= len(scn.want)
    if not exact:
        return
    assert st["repairs"] == 0 and st["serial_redos"] == 0
    assert len(delivered) + st["overflowed"] == len(scn.want)
    ovf = 0
    for k, g in enumerate(got):
        # a ring of `cap` slots and nothing void in it: the push hands out min(cap, its bursts), and counts the rest, push by push
        assert len(g) == min(cap, n[k]) and stats[k]["overflowed"] - ovf == n[k] - len(g), k
        ovf = stats[k]["overflowed"]
        _exact_subset([_key(b) for b in g], [_key(b, 0) for b in scn.per_push[k]])
        if n[k] <= cap:     # the first and the third push in every run with room for them: the full ring before left their state alone
            assert [_key(b) for b in g] == [_key(b, 0) for b in scn.per_push[k]], k
    if cap >= max(n):
        assert st["overflowed"] == 0 and [_key(b) for b in delivered] == [_key(b, 0) for b in scn.want]


@pytest.mark.parametrize("which", ["1", "5", "N2-1", "N2", "N2+1"])
def test_record_ring_full(built, oracle, which):
    """The reserved-slot path of the payload decode (k2d_run with sel_reserved): max_bursts below, at and above what
    the busy push yields.  The default build decodes the scenario without a repair, which the check asserts."""
    scn = _scn("ring", oracle)
    n2 = len(scn.per_push[1])
    cap = {"1": 1, "5": 5, "N2-1": n2 - 1, "N2": n2, "N2+1": n2 + 1}[which]
    got, _, stats = _run_ring(scn, max_bursts=cap)
    _check_ring(scn, got, stats, cap)


@pytest.mark.parametrize("path", ["serial", "full_scan", "repairs"])
def test_record_ring_full_on_the_other_paths(built, oracle, monkeypatch, path):
    """max_bursts = 5 down the other three ways a record reaches the ring: the serial machine's own overflow count, the atomic
    slots of a complete scan, and the second payload pass with the tagging loop behind a repair round (void first-pass records take
    slots there: subset, order and >= only)."""
    scn = _scn("ring", oracle)
    if path == "repairs":
        monkeypatch.setenv("VDL2GPU_REPAIR_ROUNDS", "3")
        kw = {"flags": lib.F_TEST_NOREGION}
    else:
        kw = {path: True}
    got, _, stats = _run_ring(scn, max_bursts=5, **kw)
    _check_ring(scn, got, stats, 5, exact=path != "repairs" and stats[-1]["repairs"] == 0 and stats[-1]["serial_redos"] == 0)
    if path == "repairs":
        assert stats[-1]["repairs"] > 0, stats[-1]


def test_record_ring_full_with_frames(built, oracle):
    """The block kernel works on the clamped record count: the frames are those of the bursts that were delivered, no other."""
    scn = _scn("ring", oracle)
    got, frames, stats = _run_ring(scn, max_bursts=5, frames=True)
    _check_ring(scn, got, stats, 5)
    assert stats[-1]["frames_dropped"] == 0
    by_key = {_key(b, 0): b for b in scn.want}
    for g, fr in zip(got, frames):
        _exact_subset(fr, scn.want_frames())
        assert sorted(fr) == sorted(scn.want_frames([by_key[_key(b)] for b in g]))


def test_record_ring_full_with_levels_and_maps(built, oracle):
    """Levels and reliability maps lie beside the records, slot for slot: each delivered burst has its own."""
    scn = _scn("ring", oracle)
    got, _, stats = _run_ring(scn, max_bursts=5, levels=True, soft_rs=True)
    _check_ring(scn, got, stats, 5)
    model = _models(oracle, scn.raw, scn.fo)
    k_scale = LR.scale_k("cs16", RATE, LR.mflt_taps())
    for b in (b for g in got for b in g):
        _check_level_and_map(b, model, k_scale)


# ================================================================================================ b. the host queues
MAXB = 8


def _bound_scenario(oracle):
    """8 pushes, 3 channels, two bursts a channel and push: no push fills the ring of 8, all of them overfill the queue of 32"""
    rng = np.random.default_rng(90)
    step, bursts = 1 << 17, []
    for k in range(8):
        for c in range(3):
            t = k * step / RATE + 0.004 + 0.001 * c
            for _ in range(2):
                b = synth.Burst(chan=c, t0=t, info=bytes(rng.integers(0, 256, int(rng.integers(3, 30)), dtype=np.uint8).tolist()),
                                amp=float(rng.uniform(15, 50)), cfo=float(rng.uniform(-300, 300)))
                bursts.append(b)
                t += b.duration() + 0.003
            assert t < (k + 1) * step / RATE - 0.004
    fo = (S.FO8[0], S.FO8[3], S.FO8[6])     # (apart: a strong burst 100 kHz away can trigger the sync detector of its neighbour)
    scn = _Scn(oracle, synth.StreamSpec(rate=RATE, fo=fo, nsamples=8 * step, bursts=bursts, seed=90), [step] * 8)
    n = [len(p) for p in scn.per_push]
    assert all(1 <= v <= MAXB for v in n) and sum(n) > 4 * MAXB + max(n) and sum(n[:-1]) > 4 * MAXB, n
    assert len({_key(b, 0) for b in scn.want}) == len(scn.want)
    fr = scn.want_frames()
    assert len(fr) == len(scn.want) == len(set(fr))       # one frame a burst: the frames queue meets the same bound
    return scn


def test_host_burst_queue_sheds_its_oldest(built, oracle):
    """A consumer of frames only: the burst queue keeps the newest records -- 4 x max_bursts when a push's records join, so at most
    that plus one push -- and counts the others."""
    scn = _scn("bound", oracle)
    with _rx(scn, max_bursts=MAXB, frames=True) as rx:
        frames = []
        for chunk in scn.pushes():
            rx.push(chunk)
            frames += rx.poll_frames()
        got = rx.poll()
        st = rx.stats()
    print(f"bursts: oracle {len(scn.want)}, delivered {len(got)}, overflowed {st['overflowed']}")
    want = [_key(b, 0) for b in scn.want]
    _exact_subset([_key(b) for b in got], want)
    assert [_key(b) for b in got] == want[len(want) - len(got):]
    assert len(got) + st["overflowed"] == len(want) and st["overflowed"] > 0
    assert 4 * MAXB <= len(got) <= 4 * MAXB + len(scn.per_push[-1])
    assert frames == scn.want_frames() and st["frames_dropped"] == 0


def test_host_frames_queue_sheds_its_oldest(built, oracle):
    """The mirror image: a consumer of bursts only."""
    scn = _scn("bound", oracle)
    with _rx(scn, max_bursts=MAXB, frames=True) as rx:
        got = []
        for chunk in scn.pushes():
            rx.push(chunk)
            got += rx.poll()
        frames = rx.poll_frames()
        st = rx.stats()
    print(f"frames: oracle {len(scn.want)}, delivered {len(frames)}, frames_dropped {st['frames_dropped']}")
    want = scn.want_frames()
    _exact_subset(frames, want)
    assert frames == want[len(want) - len(frames):]
    assert len(frames) + st["frames_dropped"] == len(want) and st["frames_dropped"] > 0
    assert 4 * MAXB <= len(frames) <= 4 * MAXB + len(scn.per_push[-1])
    assert [_key(b) for b in got] == [_key(b, 0) for b in scn.want] and st["overflowed"] == 0


def _compactions(counts, bite):
    """how often the storage behind a queue is compacted when push k brings counts[k] entries and the consumer takes one bite
    after every push: at a harvest with unread entries behind a handed-out prefix of more than 1024 that is the larger part"""
    pos = size = hits = 0
    for n in counts:
        if pos == size:
            pos = size = 0
        elif pos > 1024 and pos > size // 2:
            hits, size, pos = hits + 1, size - pos, 0
        size += n
        pos += min(bite, size - pos)
    return hits


NSTREAMS = 12


def test_burst_queue_compaction_carries_levels_and_maps(built, oracle, monkeypatch):
    """A consumer that takes small bites: more than 1024 records have been handed out and others wait when a push is collected,
    so the storage is compacted and every waiting record moves with its level record and its map -- from a slab or from the pageable
    queue (VDL2GPU_SLAB_CAP = 5: five records a push lie in a slab, the others come through the bounce buffer).

    One stream cannot get there within the sample limit: the shortest burst takes 10 ms with its gap, 8 channels give about 700
    bursts in 1 << 21 samples.  So ONE recording of 3 << 17 samples goes to 12 streams of one handle, each with the recording turned by
    its own number of samples (neighbours in the hand-out order are then different bursts: a slip of one place shows); the oracle
    decodes each turned recording."""
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
    scns = [_Scn(oracle, spec, sizes, margin=0, raw=np.roll(base, 2 * 24571 * s)) for s in range(NSTREAMS)]
    want = sorted(((b.end_dec, s, b.chn), _key(b, s), b.trig_dec) for s, scn in enumerate(scns) for b in scn.want)
    counts = [sum(len(scn.per_push[k]) for scn in scns) for k in range(16)]
    bite = 85
    assert len(want) > 1024 + 2 * bite and _compactions(counts, bite) >= 1, (len(want), counts)
    assert len({(k[0], k[1], t) for _, k, t in want}) == len(want)
    monkeypatch.setenv("VDL2GPU_SLAB_CAP", "5")
    raw = np.stack([scn.raw for scn in scns])
    with _rx(scns[0], nstreams=NSTREAMS, levels=True, soft_rs=True, testhooks=True) as rx:
        got = []
        for chunk in scns[0].pushes(raw):
            rx.push(chunk)
            got += _bite(rx, bite)
        handed = len(got)
        got += rx.poll()
        st = rx.stats()
    print(f"burst compaction: oracle {len(want)} ({counts} a push), {handed} handed out in bites of {bite}, then {len(got) - handed}")
    assert st["overflowed"] == 0
    assert [_key(b) for b in got] == [k for _, k, _ in want]
    assert len({(b.stream, b.chn, b.trig_dec) for b in got}) == len(got)
    model = {}
    for s, scn in enumerate(scns):
        model.update(_models(oracle, scn.raw, scn.fo, stream=s))
    k_scale = LR.scale_k("cs16", RATE, LR.mflt_taps())
    for b in got:
        _check_level_and_map(b, model, k_scale)


def _many_frames_scenario(oracle):
    """8 channels of bursts with twelve nested frames each (the most a burst may carry): four figures of frames in 1 << 20 samples"""
    rng = np.random.default_rng(1212)
    nsamp, bursts = 1 << 20, []
    for c in range(8):
        t = 0.002 + 0.0017 * c
        while True:
            b = synth.Burst(chan=c, t0=t, info=b"", amp=float(rng.uniform(20, 50)), cfo=float(rng.uniform(-300, 300)),
                            raw_payload=K.nested(12, rng))
            if t + b.duration() + 0.003 > nsamp / RATE:
                break
            bursts.append(b)
            t += b.duration() + 0.003
    scn = _Scn(oracle, synth.StreamSpec(rate=RATE, fo=S.FO8, nsamples=nsamp, bursts=bursts, seed=1212), [nsamp // 8] * 8, margin=0)
    assert sum(len(scn.frames[id(b)]) == 12 for b in scn.want) >= 0.9 * len(bursts) and len(bursts) >= 120
    return scn


def test_frames_queue_compaction(built, oracle):
    """The same consumer on the frames queue, whose entries are self-delimiting: compacted behind more than 1024 handed-out frames,
    every frame still comes out once and in order."""
    scn = _scn("many_frames", oracle)
    want = scn.want_frames()
    counts = [len(scn.want_frames(p)) for p in scn.per_push]
    bite = 150
    assert len(want) > 1024 + 2 * bite and _compactions(counts, bite) >= 1, (len(want), counts)
    with _rx(scn, frames=True) as rx:
        frames = []
        for chunk in scn.pushes():
            rx.push(chunk)
            frames += _bite_frames(rx, bite)
        handed = len(frames)
        frames += rx.poll_frames()
        got = rx.poll()
        st = rx.stats()
    print(f"frame compaction: oracle {len(want)} ({counts} a push), {handed} handed out in bites of {bite}, then {len(frames) - handed}")
    assert st["frames_dropped"] == 0 and st["overflowed"] == 0
    assert frames == want
    assert [_key(b) for b in got] == [_key(b, 0) for b in scn.want]


# ================================================================================================ c. the frame arena
L1, L2 = 208, 472                       # arena frames of the push that fits and of the one that does not: entries of 264 and 528 bytes
ARENA = 5 * _entry(L1)                  # 1320 bytes


def _arena_scenario(oracle):
    """Five pushes on 3 channels; an output ring serves every third push, so two quiet pushes lie between the push that fits (A) and
    the one that overflows (B): B meets A's entries in its arena.
      A      five frames of 208 bytes: five entries of 264 bytes, the whole arena
      -, -   noise
      B      three frames of 472 bytes (entries of 528: two fit, the third allocation fails at byte 1056, the boundary of A's fifth
             entry, which is still there) and six first frames of at most 200 bytes, which lie in their records' slots
      C      one frame of 208 bytes and two slot frames"""
    rng = np.random.default_rng(1320)

    def body(n):
        return bytes(v if v != 0x7e else 0x7d for v in rng.integers(0, 256, n).tolist())

    sizes = [5 << 16, 1 << 15, 1 << 15, 7 << 16, 3 << 16]
    plan = [[[L1, L1], [L1, L1], [L1]], None, None,
            [[L2, 40, 199], [L2, 200, 75], [L2, 120, 13]],
            [[L1], [90], [150]]]
    bursts, s0 = [], 0
    for size, chans in zip(sizes, plan):
        for c, lens in enumerate(chans or []):
            t = s0 / RATE + 0.004 + 0.0011 * c
            for n in lens:
                b = synth.Burst(chan=c, t0=t, info=b"", amp=float(rng.uniform(25, 50)), cfo=float(rng.uniform(-200, 200)),
                                raw_payload=K.frame(body(n - 4)))
                bursts.append(b)
                t += b.duration() + 0.003
            assert t < (s0 + size) / RATE - 0.004, (size, c, t)
        s0 += size
    scn = _Scn(oracle, synth.StreamSpec(rate=RATE, fo=S.FO8[:3], nsamples=sum(sizes), bursts=bursts, seed=1320), sizes)
    lens = [sorted(len(f) for b in p for f in scn.frames[id(b)]) for p in scn.per_push]
    assert all(len(scn.frames[id(b)]) == 1 for b in scn.want)
    assert lens == [[L1] * 5, [], [], [13, 40, 75, 120, 199, 200, L2, L2, L2], [90, 150, L1]], lens
    assert HDR + 200 <= SLOT < HDR + L1 and 5 * _entry(L1) == ARENA and _entry(L2) == 2 * _entry(L1)
    assert 2 * _entry(L2) + _entry(L1) == ARENA < 3 * _entry(L2)       # the failed allocation starts at A's fifth entry
    fr = scn.want_frames()
    assert len(set(fr)) == len(fr)
    return scn


def _run_arena(scn, arena, monkeypatch):
    monkeypatch.setenv("VDL2GPU_FRAME_ARENA", str(arena))
    with _rx(scn, frames=True, testhooks=True) as rx:
        frames, got, dropped = [], [], []
        for chunk in scn.pushes():
            rx.push(chunk)
            frames.append(rx.poll_frames())
            got.append(rx.poll())
            dropped.append(rx.stats()["frames_dropped"])
    assert [_key(b) for g in got for b in g] == [_key(b, 0) for b in scn.want]      # the records never notice
    return frames, dropped


def _report(tag, frames, want, dropped):
    extra = collections.Counter(frames) - collections.Counter(want)
    print(f"{tag}: oracle {len(want)} frames, delivered {len(frames)}, counted as dropped {dropped}; "
          f"not of this push: {sum(extra.values())}, of lengths {sorted(len(f[2]) for f in extra.elements())}")


def test_frame_arena_overflow(built, oracle, monkeypatch):
    """An arena of 1320 bytes.  Which of B's three long frames find room is up to the wavefronts; what must hold is that B's frames
    are B's: no entry the push did not write (A's fifth entry lies behind B's two), none twice, none of length 0, the loss counted."""
    scn = _scn("arena", oracle)
    frames, dropped = _run_arena(scn, ARENA, monkeypatch)
    want = [scn.want_frames(p) for p in scn.per_push]
    for k in range(5):
        _report(f"arena {ARENA}, push {k}", frames[k], want[k], dropped[k] - (dropped[k - 1] if k else 0))
    assert frames[0] == want[0] and dropped[0] == 0
    assert frames[1] == [] and frames[2] == [] and dropped[2] == 0
    b = frames[3]
    _exact_subset(b, want[3])
    assert not set(b) & set(want[0])
    assert all(len(f[2]) > 0 for f in b) and len(set(b)) == len(b)
    assert len(b) + (dropped[3] - dropped[2]) == len(want[3])
    assert {f for f in want[3] if len(f[2]) <= 200} <= set(b)
    long_ones = [f for f in b if len(f[2]) == L2]
    assert 1 <= len(long_ones) < 3
    assert len(long_ones) == 2          # 2 x 528 <= 1320 < 3 x 528: the counter is monotonic, the first two allocations succeed
    assert frames[4] == want[4] and dropped[4] == dropped[3]


def test_frame_arena_smaller_than_any_entry(built, oracle, monkeypatch):
    """An arena of 64 bytes: every frame that needs it is dropped and counted, the slot frames arrive, nothing else appears."""
    scn = _scn("arena", oracle)
    frames, dropped = _run_arena(scn, 64, monkeypatch)
    before = 0
    for k, p in enumerate(scn.per_push):
        want = scn.want_frames(p)
        _report(f"arena 64, push {k}", frames[k], want, dropped[k] - before)
        slot = [f for f in want if len(f[2]) <= 200]
        assert frames[k] == slot
        assert dropped[k] - before == len(want) - len(slot)
        before = dropped[k]
    assert before == 9
