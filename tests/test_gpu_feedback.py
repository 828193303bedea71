"""VDL2GPU_F_FEEDBACK on the GPU: every burst's decision-feedback rows equal the definition's (tests/feedback_ref.py, on the oracle's tap
and pinned by the oracle's bytes) byte for byte, on every decode path, push cut and burst geometry; the flag changes nothing else; with
VDL2GPU_F_FRAMES the block path's frames and reports are the model's row rule; vdl2gpu_decode_blocks_feedback on crafted rows; and the
rows stay beside their burst through a full record ring, the ingest ring and two streams.

2 MS/s cs16 unless said otherwise; a model is computed once per process and shared by the tests that use it."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import carrier_ref as CR
import feedback_ref as F
import geom_craft as G
import rs_cases
import scenarios as S
import test_gpu_full as TF
from test_gpu_chain import PART, _env, _push_parts
from test_gpu_planes import PATHS
from test_gpu_planes import _rx as _rx_identity
from vdlm2dec_amd import lib, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATE = 2_000_000
_cache = {}


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _rx(fo, fc=S.FC, plans=None, **kw):
    from vdlm2dec_amd.demod import Receiver, plan_channels
    return Receiver(RATE, plans or plan_channels(fc, fo), fmt="cs16", **kw)


def _rest(b):
    """everything of a burst but its feedback rows, comparable bit for bit"""
    return (b.stream, b.chn, b.Fr, b.nbrow, b.nlbyte, np.float32(b.df).view(np.uint32).item(), np.float32(b.ppm).view(np.uint32).item(),
            b.trig_dec, b.end_dec, b.trig_sample, b.end_sample, b.data, repr(b.level), None if b.soft is None else b.soft.tobytes(),
            repr(b.carrier), repr(b.report))


def _check(bursts, want, least=5):
    """every burst carries the model's rows; want: {(stream, chn, trig_dec): (oracle Block, fb rows)}"""
    assert len(bursts) == len(want) >= least, (len(bursts), len(want))
    assert len({(b.stream, b.chn, b.trig_dec) for b in bursts}) == len(bursts)
    for b in bursts:
        blk, fb = want[(b.stream, b.chn, b.trig_dec)]
        assert b.data == blk.data, (b.stream, b.chn, b.trig_dec)
        assert b.fb is not None and b.fb.shape == (8, 255) and b.fb.dtype == np.uint8
        assert np.array_equal(b.fb, fb), (b.stream, b.chn, b.trig_dec, np.argwhere(b.fb != fb)[:5])


# ================================================================================================ 1. parity on the five paths
def _physics():
    def make():
        spec = CR.physics_spec()
        raw = synth.synth_stream(spec, "cs16")
        return spec, raw, F.stream_rows(raw, "cs16", RATE, spec.fo, S.FC)
    return _cached("physics", make)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("path", list(PATHS))
def test_rows_equal_the_model_and_nothing_else_changes(built, oracle, monkeypatch, path):
    """carrier_ref.physics_spec() (4 channels, 2^20 samples, about 25 bursts) with every other column on: one push, and odd pushes with
    cuts inside bursts; the rows are the model's, the rest is a handle's without the flag"""
    kw = _env(monkeypatch, path)
    spec, raw, want = _physics()
    n = raw.size // 2
    cols = dict(levels=True, soft_rs=True, carrier=True)
    with _rx(spec.fo, max_push=n, **cols, **kw) as rx:
        plain = rx.run(raw, block=n)
    with _rx(spec.fo, max_push=n, feedback=True, **cols, **kw) as rx:
        one = rx.run(raw, block=n)
        st = rx.stats()
    if path.startswith("noregion"):
        assert st["repairs"] + st["serial_redos"] > 0, st
    _check(one, want, least=15)
    assert [_rest(b) for b in one] == [_rest(b) for b in plain]
    # cuts in the middle of three bursts, the rest odd
    mids = sorted((b.trig_sample + b.end_sample) // 2 for b in plain[2::7])[:3]
    cuts = sorted(set([0, n] + mids + [123_457, 500_001, 777_777]))
    with _rx(spec.fo, max_push=n, feedback=True, **cols, **kw) as rx:
        got = []
        for a, e in zip(cuts, cuts[1:]):
            rx.push(raw[2 * a:2 * e])
            got += rx.poll()        # (waits: what a call hands out does not depend on timing)
        st = rx.stats()
    assert st["deferrals"] > 0, st
    _check(got, want, least=15)
    with _rx(spec.fo, max_push=n, **cols, **kw) as rx:          # the same cuts and polls without the flag: the same records in the same order
        cut_plain = []
        for a, e in zip(cuts, cuts[1:]):
            rx.push(raw[2 * a:2 * e])
            cut_plain += rx.poll()
    assert [_rest(b) for b in got] == [_rest(b) for b in cut_plain]
    assert sorted(_rest(b) for b in got) == sorted(_rest(b) for b in plain)
    assert {(b.chn, b.trig_dec): b.fb.tobytes() for b in got} == {(b.chn, b.trig_dec): b.fb.tobytes() for b in one}


# ================================================================================================ 2. geometry
def _plane_model(name):
    def make():
        j = G.judge(name)
        return {(0, 0, b.trig_dec): (b, fb) for b, fb in F.tap_rows(j.dec, j.triggers, j.blocks)}
    return _cached(("plane", name), make)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("path", ("default", "serial"))
def test_every_geometry(built, oracle, monkeypatch, path):
    """tests/geom_craft.py's sweep: nbrow 1 .. 8 x the last row's byte counts either side of every parity threshold, byte counts around
    the strides of K2D_NT, every timing class -- through K2d (one chunk of indices where the phases were) and through the serial
    machine (chunks of 2043 / 2040 symbols: up to three for eight rows).  The plane is noiseless: the second slice is the first"""
    kw = _env(monkeypatch, path)
    j = G.judge("geom")
    raw = j.plane.raw()
    with _rx_identity(PART, kw, feedback=True) as rx:
        for _ in _push_parts(rx, raw):
            pass
        got = rx.poll()
        st = rx.stats()
    assert st["bursts"] == len(j.blocks) and st["overflowed"] == 0
    _check(got, _plane_model("geom"), least=100)
    seen = {(b.nbrow, b.nlbyte) for b in got}
    assert seen >= set(G.geometries()) and {1, 8} <= {r for r, _ in seen}
    for b in got:
        assert b.fb.tobytes() == b.data, (b.nbrow, b.nlbyte, b.trig_dec)


# ================================================================================================ 3. frames
def _scenario40():
    def make():
        sys.path.insert(0, os.path.join(ROOT, "scripts"))
        import ber_curve as B
        spec, _ = B.scenario(40, 18.0, seed=9300)
        raw = synth.synth_stream(spec, "cs16")
        out = {}
        for soft in (False, True):
            sent, hard, feed, taken, recs = F.scenario_frames(spec, raw, B.FO, B.FC, soft=soft)
            out[soft] = (sent, hard, feed, taken, recs)
        return spec, raw, B.FO, B.FC, out
    return _cached("s40", make)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("soft,rep", [(False, False), (True, False), (False, True), (True, True)], ids=["hard", "soft", "hard-rep", "soft-rep"])
def test_frames_of_the_pipeline_equal_the_model(built, oracle, soft, rep):
    """ber_curve.scenario(40, 18.0, seed=9300) with frames=True, feedback=True: the frames are the model's, as a set and in order, a
    strict superset of a handle's without the flag, none never sent; the reports' rows are the model's"""
    spec, raw, fo, fc, models = _scenario40()
    sent, hard, feed, taken, recs = models[soft]
    n = raw.size // 2
    with _rx(fo, fc, max_push=n, frames=True, soft_rs=soft) as rx:
        rx.push(raw)
        rx.poll()
        base = [(c, f) for _, c, f in rx.poll_frames()]
    with _rx(fo, fc, max_push=n, frames=True, soft_rs=soft, feedback=True, block_report=rep) as rx:
        rx.push(raw)
        bursts = rx.poll()
        got = [(c, f) for _, c, f in rx.poll_frames()]
    assert len(bursts) == len(recs) == 40
    model = {(b.chn, b.trig_dec): (b, fb, rel) for b, fb, rel in recs}
    want = []            # frames come out ordered by (end_dec, stream, chn, seq)
    for b in sorted(bursts, key=lambda b: (b.end_dec, b.stream, b.chn)):
        blk, fb, rel = model[(b.chn, b.trig_dec)]
        assert b.data == blk.data and np.array_equal(b.fb, fb)
        want += [(b.chn, f) for f in F.fb_frames(blk.data, fb, rel, blk.nbrow, blk.nlbyte)]
        if rep:
            m = F.report(blk.data, fb, rel, blk.nbrow, blk.nlbyte)
            r = b.report
            assert (r.row_roots, r.row_how, r.row_changed, r.bytes_changed, r.rows_failed, r.rows_rescued) == \
                (m["row_roots"], m["row_how"], m["row_changed"], m["bytes_changed"], m["rows_failed"], m["rows_rescued"]), (b.chn, b.trig_dec)
    assert got == want
    assert set(got) == feed
    assert set(got) > set(base) and len(set(got) - sent) == 0
    if rep:
        assert sum(b.report.row_how.count(lib.ROW_FEEDBACK) for b in bursts) == taken > 0
    if not soft:
        assert set(base) == hard and len(hard & sent) == 12 and len(feed & sent) >= 19


# ================================================================================================ 4. the batch call
@pytest.fixture(scope="module")
def anyrx(built):
    from vdlm2dec_amd.demod import Receiver, plan_channels
    with Receiver(RATE, plan_channels(S.FC, [-50000]), fmt="cu8", max_push=4096) as r:       # any handle serves the batch call
        yield r


def _hit(row, pos, mag=0x5a):
    """errors at `pos`, every one of another magnitude (mag, mag + 1, .. mod 255, never 0)"""
    row = row.copy()
    row[list(pos)] ^= np.array([(mag + 37 * i) % 255 + 1 for i in range(len(pos))], np.uint8)
    return row


def _last_row(nlbyte, seed):
    """a last row of nlbyte data bytes as it is received: zero fill, the parity that is sent, zeros where it is not"""
    nbrow, nl, data = synth.received_rows(bytes(np.random.default_rng(seed).integers(0, 256, nlbyte, dtype=np.uint8).tolist()))
    assert (nbrow, nl) == (1, nlbyte)
    return np.frombuffer(data, np.uint8).reshape(8, 255)[0].copy()


def _crafted():
    """[(name, nbrow, nlbyte, data rows, fb rows, rel or None)]"""
    cw = rs_cases.codewords()
    rng = np.random.default_rng(21)
    out = []

    def blk(name, nbrow, nlbyte, rows, fbrows, rel=None):
        data, fb = np.zeros((8, 255), np.uint8), np.zeros((8, 255), np.uint8)
        data[:len(rows)], fb[:len(fbrows)] = rows, fbrows
        out.append((name, nbrow, nlbyte, data, fb, rel))
    four = (3, 50, 99, 200)
    blk("ref fails, fb clean", 1, 249, [_hit(cw[0], four)], [cw[0]])
    blk("ref fails, fb with three errors decodes", 1, 249, [_hit(cw[1], four)], [_hit(cw[1], (7, 8, 240), 0x11)])
    blk("ref decodes, fb differs: ignored", 1, 249, [_hit(cw[2], (5, 6))], [_hit(cw[2], four)])
    blk("ref clean, fb garbage: ignored", 1, 249, [cw[3]], [rng.integers(0, 256, 255, dtype=np.uint8)])
    blk("both fail, hard mode: what the reference left", 1, 249, [_hit(cw[4], four)], [_hit(cw[4], (1, 2, 3, 4, 5), 0x33)])
    rel = np.full((8, 255), 200, np.uint8)
    rel[0, list(four)] = (1, 2, 3, 4)
    blk("both fail, soft mode: the trials run on the received row", 1, 249, [_hit(cw[5], four)], [_hit(cw[5], (1, 2, 3, 4, 5), 0x33)], rel)
    for nl, nfix, pos, mag in ((60, 2, (0, 5, 59), 0x5a), (25, 4, (1, 9), 0x11)):
        # 2 fixed erasures leave room for two errors, 4 for one; with 4 the two syndromes left nearly always name a position, and rs()
        # then "corrects" it: these two errors are among the few it gives up on
        row = _last_row(nl, 100 + nl)
        blk(f"last row with {nfix} fixed erasures", 1, nl, [_hit(row, pos, mag)], [_hit(row, (2,))])
        blk(f"last row with {nfix} fixed erasures, fb fails too", 1, nl, [_hit(row, pos, mag)], [_hit(row, pos, mag)])
    row = _last_row(25, 125)
    blk("4 fixed erasures in soft mode, both fail: no trial has room", 1, 25, [_hit(row, (1, 9), 0x11)], [_hit(row, (1, 9), 0x11)],
        np.full((8, 255), 7, np.uint8))
    rows = [cw[i].copy() for i in range(8)]
    bad = [_hit(r, four) if i % 2 else r for i, r in enumerate(rows)]
    fbr = [rows[i] if i in (1, 5) else _hit(rows[i], (9, 19, 29, 39), 0x77) for i in range(8)]
    blk("8 rows: 1 and 5 from fb, 3 and 7 fail, the even ones clean", 8, 249, bad, fbr)
    return out


def _batch(rx, cases, with_fb, report=True):
    blocks = [(nbrow, nlbyte, d.tobytes()) for _, nbrow, nlbyte, d, _, _ in cases]
    return rx.decode_blocks(blocks, fb=[f for *_, f, _ in cases] if with_fb else None, report=report)


def test_decode_blocks_with_feedback_rows(anyrx, oracle):
    cases = _crafted()
    hard = [c for c in cases if c[5] is None]
    soft = [c for c in cases if c[5] is not None]
    seen = set()
    for group, rels in ((hard, None), (soft, [c[5] for c in soft])):
        blocks = [(nbrow, nlbyte, d.tobytes()) for _, nbrow, nlbyte, d, _, _ in group]
        frames, reps = anyrx.decode_blocks(blocks, soft=rels, fb=[c[4] for c in group], report=True)
        plain = anyrx.decode_blocks(blocks, soft=rels, fb=[c[4] for c in group])
        assert plain == frames                        # the kernel without the report decodes the same
        want_frames = []
        for i, (name, nbrow, nlbyte, d, fb, rel) in enumerate(group):
            m = F.report(d, fb, rel, nbrow, nlbyte)
            r = reps[i]
            assert (r.row_roots, r.row_how, r.row_changed, r.bytes_changed, r.rows_failed, r.rows_rescued, r.status) == \
                (m["row_roots"], m["row_how"], m["row_changed"], m["bytes_changed"], m["rows_failed"], m["rows_rescued"], 0), name
            want_frames += [(i, f) for f in F.fb_frames(d, fb, rel, nbrow, nlbyte)]
            seen.update(m["row_how"])
        assert frames == want_frames
    assert seen >= {lib.ROW_NONE, lib.ROW_CLEAN, lib.ROW_REF, lib.ROW_SOFT2, lib.ROW_FAIL, lib.ROW_FEEDBACK}, seen
    by = {name: F.report(d, fb, rel, nbrow, nlbyte)["row_how"] for name, nbrow, nlbyte, d, fb, rel in cases}
    assert by["ref fails, fb clean"][0] == by["ref fails, fb with three errors decodes"][0] == lib.ROW_FEEDBACK
    assert by["ref decodes, fb differs: ignored"][0] == lib.ROW_REF and by["ref clean, fb garbage: ignored"][0] == lib.ROW_CLEAN
    assert by["both fail, hard mode: what the reference left"][0] == lib.ROW_FAIL
    assert by["both fail, soft mode: the trials run on the received row"][0] in (lib.ROW_SOFT2, lib.ROW_SOFT4)
    assert by["4 fixed erasures in soft mode, both fail: no trial has room"][0] == lib.ROW_FAIL
    assert by["last row with 2 fixed erasures"][0] == by["last row with 4 fixed erasures"][0] == lib.ROW_FEEDBACK
    assert by["last row with 2 fixed erasures, fb fails too"][0] == by["last row with 4 fixed erasures, fb fails too"][0] == lib.ROW_FAIL
    assert by["8 rows: 1 and 5 from fb, 3 and 7 fail, the even ones clean"] == (1, 6, 1, 5, 1, 6, 1, 5)


def test_decode_blocks_without_fb_is_the_old_call(anyrx, oracle):
    """fb == NULL: what the call decodes is held to references that do not pass through it -- the frames of crafted bursts
    (tests/blocks_craft.py) to the oracle's block path, the rows' reports to the model without feedback rows (soft_ref's row rule),
    hard and soft -- and the two entry points agree bit for bit (frames, dropped, reports)"""
    import blocks_craft as K
    every = K.everything()
    crafted = [(nbrow, nlbyte, np.frombuffer(bytes(data), np.uint8).reshape(8, 255), None) for _, (nbrow, nlbyte, data), _ in every[::25]]
    cases = crafted + [(nbrow, nlbyte, d, rel) for _, nbrow, nlbyte, d, _, rel in _crafted()]
    assert len(crafted) >= 40
    n = len(cases)
    arr, sarr = (lib.BurstT * n)(), (lib.SoftT * n)()
    for i, (nbrow, nlbyte, d, rel) in enumerate(cases):
        arr[i].nbrow, arr[i].nlbyte = nbrow, nlbyte
        C.memmove(C.addressof(arr[i].data), d.tobytes(), 2040)
        C.memmove(C.addressof(sarr[i].rel), (rel if rel is not None else np.full((8, 255), 255, np.uint8)).tobytes(), 2040)
    cap = 1024
    nframes = 0
    for s in (None, sarr):
        res = []
        for new in (False, True):
            out, rep, dropped = (lib.FrameT * cap)(), (lib.BlockRepT * n)(), C.c_int(-1)
            if new:
                nf = anyrx.L.vdl2gpu_decode_blocks_feedback(anyrx.h, arr, s, None, n, out, cap, C.byref(dropped), rep)
            else:
                nf = anyrx.L.vdl2gpu_decode_blocks_report(anyrx.h, arr, s, n, out, cap, C.byref(dropped), rep)
            assert nf >= 0
            res.append((nf, dropped.value, [(out[i].block, out[i].seq, bytes(out[i].data[:out[i].len])) for i in range(nf)],
                        bytes(C.string_at(C.addressof(rep), C.sizeof(rep)))))
            if not new:
                continue
            want = []
            for i, (nbrow, nlbyte, d, rel) in enumerate(cases):
                m = F.report(d, None, (rel if rel is not None else np.full((8, 255), 255, np.uint8)) if s is not None else None, nbrow, nlbyte)
                r = rep[i]
                assert (tuple(r.row_roots), tuple(r.row_how), tuple(r.row_changed), r.rows_failed, r.rows_rescued) == \
                    (m["row_roots"], m["row_how"], m["row_changed"], m["rows_failed"], m["rows_rescued"]), i
                assert lib.ROW_FEEDBACK not in tuple(r.row_how)
                if rel is None and all(h in (lib.ROW_CLEAN, lib.ROW_REF, lib.ROW_NONE) for h in m["row_how"]):
                    fr = oracle.frames_of_block(nbrow, nlbyte, d.tobytes())[:12]          # (more than 12 in a burst are dropped)
                    want += [(i, k, f) for k, f in enumerate(fr)]
                    assert [x for x in res[-1][2] if x[0] == i] == [(i, k, f) for k, f in enumerate(fr)], i
            nframes += len(want)
        assert res[0] == res[1]
    assert nframes >= 40
    assert anyrx.L.vdl2gpu_decode_blocks_feedback(None, None, None, None, 0, None, 0, None, None) == -1


# ================================================================================================ 5. the output path
@pytest.mark.timeout(300)
def test_record_ring_full_keeps_the_rows_with_their_burst(built, oracle):
    """tests/test_gpu_full.py's ring scenario with max_bursts = 5: the busy push overfills the ring; every burst handed out carries its
    own rows, and `overflowed` accounts for the rest"""
    scn = TF._scn("ring", oracle)
    got, _, stats = TF._run_ring(scn, max_bursts=5, feedback=True)
    TF._check_ring(scn, got, stats, 5)
    assert stats[-1]["overflowed"] > 0
    want = _cached("ring", lambda: F.stream_rows(scn.raw, "cs16", RATE, scn.fo, S.FC))
    delivered = [b for g in got for b in g]
    _check(delivered, {(0, b.chn, b.trig_dec): want[(0, b.chn, b.trig_dec)] for b in delivered})


@pytest.mark.timeout(300)
def test_ingest_ring(built, oracle):
    spec, raw, want = _physics()
    n = raw.size // 2
    with _rx(spec.fo, max_push=32768, feedback=True) as rx:
        rx.ring_init(32768, 4)
        got = []
        for s in range(0, n, 32768):
            m = min(32768, n - s)
            slot = rx.ring_acquire()
            slot[0, :4 * m] = raw[2 * s:2 * (s + m)].view(np.uint8)
            rx.ring_commit(m)
            got += rx.poll_ready()
        got += rx.poll()
    _check(got, want, least=15)


@pytest.mark.timeout(300)
def test_two_streams(built, oracle):
    from vdlm2dec_amd.demod import plan_channels
    ins = S.distinct_streams(2, nsamples=1 << 19)
    want = {}
    for s, (r, fo, fc) in enumerate(ins):
        want.update(F.stream_rows(r, "cs16", RATE, fo, fc, stream=s))
    raw = np.stack([r for r, _, _ in ins])
    with _rx(None, plans=[plan_channels(fc, fo) for _, fo, fc in ins], max_push=1 << 18, feedback=True) as rx:
        got = rx.run(raw)
    _check(got, want)
    assert {b.stream for b in got} == {0, 1}


@pytest.mark.timeout(300)
def test_fb_needs_the_flag_and_a_null_column_is_the_old_poll(built, oracle):
    spec, raw, want = _physics()
    n = raw.size // 2
    k = 4096
    size = C.sizeof(lib.BurstT)
    with _rx(spec.fo, max_push=n, carrier=True) as rx:              # no VDL2GPU_F_FEEDBACK
        rx.push(raw)
        rx.sync()
        buf, fv = (lib.BurstT * k)(), (lib.FbT * k)()
        for fn in (rx.L.vdl2gpu_poll_feedback, rx.L.vdl2gpu_poll_feedback_ready):
            assert fn(rx.h, buf, None, None, None, None, fv, k) == -1     # VDL2GPU_EINVAL ...
            assert b"VDL2GPU_F_FEEDBACK" in rx.L.vdl2gpu_last_error(rx.h)
        with pytest.raises(lib.Vdl2GpuError):
            rx.poll_feedback_raw(buf, None, None, None, None, fv, k)
        cv = (lib.CarrierT * k)()
        m = rx.poll_feedback_raw(buf, None, None, cv, None, None, k)  # ... and nothing was consumed; fb NULL: vdl2gpu_poll_report
        assert m == len(want)
        plain = bytes(C.string_at(C.addressof(buf), m * size))
    with _rx(spec.fo, max_push=n, feedback=True) as rx:
        rx.push(raw)
        buf = (lib.BurstT * k)()
        assert rx.L.vdl2gpu_poll_feedback(rx.h, buf, None, None, None, (lib.BlockRepT * k)(), None, k) == -1   # rep without its flag, as ever
        m = rx.poll_feedback_raw(buf, None, None, None, None, None, k)
        assert m == len(want) and bytes(C.string_at(C.addressof(buf), m * size)) == plain
        assert rx.poll_feedback_raw(buf, None, None, None, None, None, k) == 0
