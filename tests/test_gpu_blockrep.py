"""VDL2GPU_F_BLOCK_REPORT on the GPU: every report the kernel writes equals the CPU model's (tests/blockrep_ref.py, pinned to the oracle
by tests/test_blockrep_model.py) -- integers, so equality -- in the batch call (hard and soft mode, stale slots) and in the pipeline
(all side columns on; one push, many pushes, the bounce path, every burst through a repair round), and nothing else changes with the
flag."""
import ctypes as C

import numpy as np
import pytest

import blockrep_ref as M
import blocks_craft as K
import scenarios as S
import soft_cases
import soft_ref as R

pytestmark = pytest.mark.gpu

RATE = 2_000_000
FO = [-50_000, 250_000]


@pytest.fixture(scope="module")
def rx(built):
    from vdlm2dec_amd.demod import Receiver, plan_channels
    with Receiver(RATE, plan_channels(S.FC, [-50000]), fmt="cu8", max_push=4096) as r:       # any handle serves the batch call
        yield r


def _direct(rx, blocks, rels=None, report=True, cap=8192):
    """vdl2gpu_decode_blocks_report / _soft / vdl2gpu_decode_blocks themselves (Receiver.decode_blocks refuses a result with frames
    dropped, and a burst with more than 12 frames drops some): ([(block, seq, hdata)], dropped, [BlockReport] or None)"""
    from vdlm2dec_amd import demod, lib
    n = len(blocks)
    arr = (lib.BurstT * n)()
    for i, (nbrow, nlbyte, data) in enumerate(blocks):
        arr[i].nbrow, arr[i].nlbyte = nbrow, nlbyte
        C.memmove(C.addressof(arr[i].data), bytes(data), 8 * 255)
    sarr = None
    if rels is not None:
        sarr = (lib.SoftT * n)()
        for i, m in enumerate(rels):
            m = np.ascontiguousarray(m, np.uint8).reshape(8, 255)
            C.memmove(C.addressof(sarr[i].rel), m.ctypes.data, 8 * 255)
    out = (lib.FrameT * cap)()
    dropped = C.c_int(-1)
    rarr = (lib.BlockRepT * n)()
    C.memset(rarr, 0xa5, C.sizeof(rarr))                 # nothing of this may survive
    if report:
        nf = rx.L.vdl2gpu_decode_blocks_report(rx.h, arr, sarr, n, out, cap, C.byref(dropped), rarr)
    elif rels is not None:
        nf = rx.L.vdl2gpu_decode_blocks_soft(rx.h, arr, sarr, n, out, cap, C.byref(dropped))
    else:
        nf = rx.L.vdl2gpu_decode_blocks(rx.h, arr, n, out, cap, C.byref(dropped))
    assert nf >= 0, rx.L.vdl2gpu_last_error(rx.h)
    frames = [(out[i].block, out[i].seq, bytes(out[i].data[:out[i].len])) for i in range(nf)]
    return frames, dropped.value, [demod.BlockReport.from_c(r) for r in rarr] if report else None


def _equal(got, want, names):
    assert len(got) == len(want) == len(names)
    bad = [(n, g, w) for n, g, w in zip(names, got, want) if g != w]
    assert not bad, (len(bad), bad[:3])


BADHEAD = [("nbrow0", (0, 20, bytes(2040))), ("nbrow9", (9, 20, b"\x7e" * 2040)), ("nlbyte250", (1, 250, b"\x7e" * 2040))]


def _hard_set():
    e = [(n, b) for n, b, _ in K.everything()] + [(n, b) for n, b, _, _ in M.variants() + M.soft_fail_cases()] + M.many_flags() + BADHEAD
    return [n for n, _ in e], [b for _, b in e]


def test_batch_hard_mode(rx):
    """all crafted blocks and their corrupted variants in one call: reports equal the model's; the frames are those of
    vdl2gpu_decode_blocks on the same input, more than 12 in a burst dropped alike and still counted in `frames`; a header out of
    range gives status 1 and zeros"""
    names, blocks = _hard_set()
    assert len(blocks) > 1600
    frames, dropped, reps = _direct(rx, blocks)
    want = [M.model(*b) for b in blocks]
    _equal(reps, want, names)
    plain, pdropped, _ = _direct(rx, blocks, report=False)
    assert frames == plain and dropped == pdropped
    assert len(frames) + dropped == sum(r.frames for r in reps)
    assert dropped == sum(max(0, r.frames - 12) for r in reps) > 0
    for r in reps[-3:]:
        assert r == M._zero(1)
    assert {h for r in reps for h in r.row_how} == {M.NONE, M.CLEAN, M.REF, M.FAIL}
    assert any(r.too_short for r in reps) and any(r.bad_fcs for r in reps) and any(r.flag_at == -1 and r.status == 0 for r in reps)
    assert max(r.bad_fcs for r in reps) == 1978 and max(r.cand for r in reps) == 1988        # bursts of idle flags: the counters' far end


def test_batch_without_room_for_frames(rx):
    """max_frames == 0 (and frames == NULL): the reports are filled all the same, every frame is counted as dropped"""
    from vdlm2dec_amd import demod, lib
    entries = K.thresholds() + K.nested_blocks() + [(n, b, 0) for n, b in M.many_flags()]
    blocks = [b for _, b, _ in entries]
    n = len(blocks)
    arr = (lib.BurstT * n)()
    for i, (nbrow, nlbyte, data) in enumerate(blocks):
        arr[i].nbrow, arr[i].nlbyte = nbrow, nlbyte
        C.memmove(C.addressof(arr[i].data), bytes(data), 8 * 255)
    rarr = (lib.BlockRepT * n)()
    C.memset(rarr, 0xa5, C.sizeof(rarr))
    dropped = C.c_int(-1)
    assert rx.L.vdl2gpu_decode_blocks_report(rx.h, arr, None, n, None, 0, C.byref(dropped), rarr) == 0
    reps = [demod.BlockReport.from_c(r) for r in rarr]
    _equal(reps, [M.model(*b) for b in blocks], [e[0] for e in entries])
    assert dropped.value == sum(r.frames for r in reps) == sum(i for _, _, i in K.thresholds() + K.nested_blocks()) + 1     # (+ the frame in front of the flags)
    assert rx.L.vdl2gpu_decode_blocks_report(rx.h, arr, None, n, None, 0, C.byref(dropped), None) == 0 and dropped.value == 0   # rep == NULL: nothing to do


def test_batch_python_surface(rx):
    """Receiver.decode_blocks(report=True): the pair; without it the list, unchanged"""
    entries = K.thresholds() + K.flag_hunt()
    blocks = [b for _, b, _ in entries]
    frames, reps = rx.decode_blocks(blocks, report=True)
    assert frames == rx.decode_blocks(blocks) == rx.decode_blocks(blocks, report=False)
    _equal(reps, [M.model(*b) for b in blocks], [n for n, _, _ in entries])
    assert [r.frames for r in reps] == [i for _, _, i in entries]


def _soft_set():
    e = [(n, b, rel) for n, b, rel, _ in M.variants() + M.soft_fail_cases()]
    e += [(f"soft_cases{i}", (nbrow, nlbyte, data.tobytes()), rel) for i, (nbrow, nlbyte, data, rel, *_) in enumerate(soft_cases.cases())]
    return e


def test_batch_soft_mode(rx, oracle):
    """the same with reliability maps: reports equal the model's in soft mode, frames equal soft_ref.soft_frames"""
    e = _soft_set()
    names, blocks, rels = [n for n, _, _ in e], [b for _, b, _ in e], [r for _, _, r in e]
    frames, dropped, reps = _direct(rx, blocks, rels)
    _equal(reps, [M.model(*b, rel=r) for b, r in zip(blocks, rels)], names)
    want = [R.soft_frames(np.frombuffer(b[2], np.uint8), r, b[0], b[1]) for b, r in zip(blocks, rels)]
    assert [r.frames for r in reps] == [len(w) for w in want] and sum(len(w) for w in want) > 300
    assert dropped == sum(max(0, len(w) - 12) for w in want)           # (the table of 12: which twelve it keeps is not defined)
    few = {i for i, w in enumerate(want) if len(w) <= 12}
    assert [(i, f) for i, _, f in frames if i in few] == [(i, f) for i in sorted(few) for f in want[i]]
    assert len(frames) + dropped == sum(len(w) for w in want)
    soft, sdropped, _ = _direct(rx, blocks, rels, report=False)
    assert soft == frames and sdropped == dropped
    assert {h for r in reps for h in r.row_how} == {M.NONE, M.CLEAN, M.REF, M.SOFT2, M.SOFT4, M.FAIL}
    assert sum(r.rows_failed for r in reps[len(M.variants()):len(M.variants()) + len(M.soft_fail_cases())]) == len(M.soft_fail_cases())


def test_stale_slots(rx):
    """two calls on one handle: long multi-frame blocks, then as many short, flagless or out-of-range ones -- nothing of the first
    call shows through in the second"""
    long_ = [b for n, b, _ in K.nested_blocks() if n in ("nested12", "nested12-7e", "nested3-long")] + [K.one_runs()[-1][1]]
    short = [b for n, b, _ in K.flag_hunt() if n.startswith("stray")] + [b for _, b, _ in K.thresholds()] + [b for _, b in BADHEAD]
    n = 64
    first = [long_[i % len(long_)] for i in range(n)]
    second = [short[i % len(short)] for i in range(n)]
    _, _, reps1 = _direct(rx, first)
    assert reps1 == [M.model(*b) for b in first] and all(r.frames >= 1 and r.cand >= 1 for r in reps1)
    _, _, reps2 = _direct(rx, second)
    assert reps2 == [M.model(*b) for b in second]
    assert min(r.nbytes for r in reps1) > max(r.nbytes for r in reps2) and min(r.stuffed for r in reps1) >= max(r.stuffed for r in reps2)
    assert any(r.status == 1 for r in reps2) and any(r.flag_at == -1 and r.status == 0 for r in reps2) and any(r.too_short for r in reps2)


# ----------------------------------------------------------------------------------------------------------------------- pipeline
def _body(seed, n):
    rng = np.random.default_rng(seed)
    return bytes(v if v != 0x7e else 0x7d for v in rng.integers(0, 256, n).tolist())


def _payloads():
    """(name, payload, corrupt): what the block path can meet in a burst"""
    rng = np.random.default_rng(2048)
    tworow = K.frame(_body(5, 262))                  # two rows, a short last one
    assert 249 + 3 <= len(tworow) <= 249 + 30
    return [
        ("plain", K.frame(_body(1, 40)), None),
        ("nested3", K.nested(3, rng), None),
        ("len12", K.frame(_body(2, 8)), None),                                   # a 12-byte candidate: too short
        ("stray", K.frame(_body(3, 40), bytes([0, 0x01, 0])), None),             # a stray bit in front: no flag
        ("tworow", tworow, None),
        ("plain-e2", K.frame(_body(4, 60)), {(0, 3): 0x11, (0, 30): 0x80}),
        ("plain-e4", K.frame(_body(6, 60)), {(0, c): 0x21 for c in (1, 9, 17, 40)}),
        ("plain-e8", K.frame(_body(7, 60)), {(0, c): 0x42 for c in (2, 5, 11, 19, 23, 31, 44, 58)}),
        ("tworow-e2", tworow, {(0, 100): 0x01, (0, 200): 0xff}),
        ("tworow-e4", tworow, {(0, c): 0x18 for c in (7, 77, 177, 247)}),
        # 20 body bytes below 0x10 (no run of five ones: nothing is stuffed), two bytes that are not their FCS, a flag: "error crc"
        ("bad-fcs", K.bytes_of(K.FLAG + K.bits_of(bytes(rng.integers(1, 16, 20).tolist()) + b"\x01\x02") + K.FLAG), None),
        ("flags-only", b"\x7e" * 20, None),
    ]


_stream = {}


def _pipeline_input():
    """two streams of two channels, a dozen bursts each (stream 1: the same payloads in another order, on the other channels)"""
    if not _stream:
        from vdlm2dec_amd import synth
        raws = []
        for s in range(2):
            pl = _payloads()
            pl = pl if s == 0 else pl[::-1]
            t = [0.002, 0.003]
            bursts = []
            for i, (_, payload, corrupt) in enumerate(pl):
                c = (i + s) % 2
                b = synth.Burst(chan=c, t0=t[c], info=b"", amp=30.0 + 3 * i, cfo=40.0 * (i - 5), corrupt=corrupt, raw_payload=payload)
                bursts.append(b)
                t[c] += b.duration() + 0.002
            raws.append((bursts, max(t)))
        ns = (int((max(e for _, e in raws) + 0.004) * RATE) + 32767) // 32768 * 32768
        _stream["raw"] = np.stack([synth.synth_stream(synth.StreamSpec(rate=RATE, fo=FO, nsamples=ns, bursts=b, seed=31 + s), "cu8")
                                   for s, (b, _) in enumerate(raws)])
        _stream["n"] = sum(len(b) for b, _ in raws)
    return _stream["raw"], _stream["n"]


def _run(push=None, **kw):
    """the stream through a handle: (bursts sorted by (stream, chn, trig_dec), frames)"""
    from vdlm2dec_amd.demod import Receiver, plan_channels
    raw, _ = _pipeline_input()
    ns = raw.shape[1] // 2
    push = push or ns
    with Receiver(RATE, [plan_channels(S.FC, FO)] * 2, fmt="cu8", max_push=push, **kw) as r:
        for s in range(0, ns, push):
            r.push(raw[:, 2 * s:2 * (s + push)])
        got = r.poll()
        frames = r.poll_frames() if kw.get("frames") else None
        st = r.stats()
    assert st["frames_dropped"] == 0       # nothing is dropped: the reports' frames are the frames handed out
    return sorted(got, key=lambda b: (b.stream, b.chn, b.trig_dec)), frames


ALL = dict(frames=True, block_report=True, levels=True, soft_rs=True, carrier=True)
_runs = {}


def _all_on():
    if "all" not in _runs:
        _runs["all"] = _run(**ALL)
    return _runs["all"]


def test_pipeline_reports_equal_the_model():
    """every column on (a mixed-up column would show): each burst's report is the model of its own data and map; the reports' frames
    add up to what poll_frames returns; without soft_rs the reports are the hard-mode model's"""
    _, nb = _pipeline_input()
    got, frames = _all_on()
    assert len(got) == nb == 24
    for b in got:
        assert b.level is not None and b.carrier is not None and b.soft is not None
        assert b.report == M.model(b.nbrow, b.nlbyte, b.data, rel=b.soft), (b.stream, b.chn, b.trig_dec)
    assert sum(b.report.frames for b in got) == len(frames) > 0
    seen = {h for b in got for h in b.report.row_how}
    assert {M.CLEAN, M.REF} <= seen and any(b.report.rows_failed or b.report.rows_rescued for b in got)
    assert any(b.report.too_short for b in got) and any(b.report.bad_fcs for b in got) and any(b.report.flag_at == -1 for b in got)
    assert any(b.report.frames == 3 for b in got) and any(b.nbrow == 2 for b in got)
    hard, hframes = _run(frames=True, block_report=True)
    assert [b.key() for b in hard] == [b.key() for b in got]
    for b in hard:
        assert b.report == M.model(b.nbrow, b.nlbyte, b.data), (b.stream, b.chn, b.trig_dec)
    assert sum(b.report.frames for b in hard) == len(hframes)


def _pairs(got):
    return [(b.key(), b.report) for b in got]


@pytest.mark.parametrize("path", ("pushes", "bounce", "noregion"))
def test_report_does_not_depend_on_the_path(monkeypatch, path):
    """32768-sample pushes (rings and slabs reused several times); the test library with one record a slab (the side columns take the
    bounce path); the region scan dropped (every burst goes through a repair round, void records between the live ones): the same
    (key, report) list as one push gives"""
    from vdlm2dec_amd import lib
    want = _pairs(_all_on()[0])
    if path == "pushes":
        got, _ = _run(push=32768, **ALL)
    elif path == "bounce":
        monkeypatch.setenv("VDL2GPU_SLAB_CAP", "1")
        got, _ = _run(testhooks=True, **ALL)
    else:
        got, _ = _run(flags=lib.F_TEST_NOREGION, **ALL)
    assert _pairs(got) == want


def test_nothing_changes_without_the_flag():
    """bursts and frames are byte-equal with and without the flag; a report buffer on a handle without it is VDL2GPU_EINVAL and
    consumes nothing"""
    from vdlm2dec_amd import lib
    from vdlm2dec_amd.demod import Receiver, plan_channels
    with_, fwith = _run(frames=True, block_report=True)
    raw, nb = _pipeline_input()
    ns = raw.shape[1] // 2
    with Receiver(RATE, [plan_channels(S.FC, FO)] * 2, fmt="cu8", max_push=ns, frames=True) as r:
        r.push(raw)
        buf, rv = (lib.BurstT * 64)(), (lib.BlockRepT * 64)()
        with pytest.raises(lib.Vdl2GpuError, match="VDL2GPU_F_BLOCK_REPORT"):
            r.poll_report_raw(buf, None, None, None, rv, 64)
        assert r.poll_report_raw(buf, None, None, None, None, 0) == 0          # rep == NULL: a plain collector
        plain = sorted(r.poll(), key=lambda b: (b.stream, b.chn, b.trig_dec))
        fplain = r.poll_frames()
    assert len(plain) == nb and all(b.report is None for b in plain)

    def whole(b):
        return (b.stream, b.chn, b.Fr, b.nbrow, b.nlbyte, np.float32(b.df).tobytes(), np.float32(b.ppm).tobytes(), b.trig_dec, b.end_dec,
                b.trig_sample, b.end_sample, b.data)
    assert [whole(b) for b in plain] == [whole(b) for b in with_]
    assert fplain == fwith and len(fplain) > 0
