"""VDL2GPU_F_TRACKED on the GPU: the column is the model's (tests/tracked_ref.py) byte for byte on the planes the demodulator held, at
every segment edge and FEC regime; a burst whose symbol clock drifts gives no frame without the flag and the sent frame with it; the
flag changes nothing else; the column does not depend on where the stream was cut or on the path; vdl2gpu_decode_blocks_tracked on
polled records reproduces the pipeline's frames and reports."""
import ctypes as C

import numpy as np
import pytest

import allframes_ref as AF
import rawflags_ref as RF
import scenarios as S
import soft_ref as R
import tracked_ref as T
from test_tracked_model import table_case
from vdlm2dec_amd import lib, synth

pytestmark = pytest.mark.gpu

EINVAL = -1      # VDL2GPU_EINVAL


def _rx(spec, fmt, nstreams=1, **kw):
    from vdlm2dec_amd.demod import Receiver, plan_channels
    plan = plan_channels(S.FC, spec.fo)
    return Receiver(spec.rate, [plan] * nstreams if nstreams > 1 else plan, fmt=fmt, **kw)


def _check_exact(rx, bursts, pn):
    """every burst's column against the model on its own channel's plane, all 2048 bytes"""
    planes = {}
    for b in bursts:
        if (b.stream, b.chn) not in planes:
            planes[(b.stream, b.chn)] = rx.debug_dec(b.stream, b.chn)
        want = T.burst_column(planes[(b.stream, b.chn)], b.nbrow, b.nlbyte, b.df, b.end_dec, pn)
        assert b.trk.raw == T.column_bytes(want), (b.stream, b.chn, b.trig_dec, (b.trk.d_first, b.trk.d_last), want["d"])


def _by_burst(bursts):
    out = {}
    for b in bursts:
        key = (b.stream, b.chn, b.trig_dec)
        assert key not in out
        out[key] = b.trk.raw
    return out


# transmitted bytes B -> payload symbols n = (25 + 8 B - 1) / 3 - 7: 95 -> 254 and 96 -> 257 (a byte is 8 / 3 symbols: 255 and 256 are not
# reachable, these are the two lengths next to the edge), 191 -> 510 and 192 -> 513; a row with more than 67 data bytes sends 6 parity
# bytes, so B - 6 payload bytes.  The FEC regimes of the last row: nlbyte <= 2 (no parity), <= 30 (2), <= 67 (4), a full row (6); and
# the longest accepted burst (8 rows, 248 bytes in the last: 22 segments).
EDGE_PAYLOADS = (40, 89, 90, 185, 186)
EDGE_N = (118, 254, 257, 510, 513)
REGIME_PAYLOADS = (249 + 2, 249 + 30, 249 + 67, 248)
LONGEST_PAYLOAD = 1991


@pytest.mark.timeout(300)
def test_tracked_segment_edges_and_fec_regimes(built):
    rng = np.random.default_rng(25)
    bursts, t = [], 0.003
    for n in EDGE_PAYLOADS + REGIME_PAYLOADS:
        b = synth.Burst(chan=0, t0=t, info=b"", amp=35.0, cfo=float(rng.uniform(-200, 200)),
                        raw_payload=bytes(rng.integers(0, 256, n, dtype=np.uint8).tolist()))
        bursts.append(b)
        t += b.duration() + 0.003
    bursts.append(synth.Burst(chan=1, t0=0.004, info=b"", amp=30.0, cfo=120.0, sym_ppm=40.0,
                              raw_payload=bytes(rng.integers(0, 256, LONGEST_PAYLOAD, dtype=np.uint8).tolist())))
    end = max(t, 0.004 + bursts[-1].duration())
    spec = synth.StreamSpec(rate=2_000_000, fo=(100_000, -250_000), nsamples=S._pad(int((end + 0.006) * 2_000_000)), bursts=bursts,
                            noise=1.5, seed=25)
    raw = synth.synth_stream(spec, "cs16")
    pn = R.pn_bits()
    with _rx(spec, "cs16", max_push=spec.nsamples, keep_dec=True, tracked=True) as rx:
        rx.push(raw)
        got = sorted(rx.poll(), key=lambda b: (b.chn, b.trig_dec))
        assert len(got) == len(bursts)
        n_of = [(25 + 8 * sum(R.geom(b.nbrow, b.nlbyte)[4:6]) - 1) // 3 - 7 for b in got]
        assert n_of[:5] == list(EDGE_N) and n_of[-1] == 5446 - 8
        assert [b.trk.nseg for b in got[:5]] == [1, 1, 2, 2, 3] and got[-1].trk.nseg == 22 == lib.TRK_SEGS
        assert [b.nlbyte for b in got[5:8]] == [2, 30, 67] and {b.nbrow for b in got[5:8]} == {2}
        _check_exact(rx, got, pn)
    assert got[-1].trk.d_last < got[-1].trk.d_first       # +40 ppm over 22 segments walks towards earlier samples


DRIFT = ((50, 1), (-50, 3), (100, 0))     # (sym_ppm, seed) of the model's table: the reference delivers no frame of these


@pytest.mark.timeout(300)
@pytest.mark.parametrize("ppm,seed", DRIFT)
def test_drifting_burst_is_rescued(built, oracle, ppm, seed):
    """THE test that fails without the feature: a 7-row burst whose symbol clock is off gives no frame; with the flag the sent frame,
    row_how holds VDL2GPU_ROW_TRACKED, and the burst records are identical"""
    raw, tx = table_case(seed, ppm)
    nbrow, nlbyte, rows = synth.received_rows(tx.payload())
    sent = oracle.frames_of_block(nbrow, nlbyte, rows)
    spec = synth.StreamSpec(rate=2_000_000, fo=(100_000,), nsamples=raw.size // 2, bursts=[tx])
    pn = R.pn_bits()
    res = {}
    for on in (False, True):
        with _rx(spec, "cs16", max_push=spec.nsamples, keep_dec=True, frames=True, block_report=True, tracked=on) as rx:
            rx.push(raw)
            bursts = rx.poll()
            frames = rx.poll_frames()
            assert len(bursts) == 1
            res[on] = (bursts[0], frames)
            if on:
                _check_exact(rx, bursts, pn)
                again, reps = rx.decode_blocks(bursts, report=True, trk=[bursts[0].trk.data])
                assert [f for _, f in again] == [f for _, _, f in frames] and reps[0] == bursts[0].report
                plain = rx.decode_blocks(bursts, report=True)
                assert plain[0] == [] and plain[1][0] == res[False][0].report       # trk=None: the block path it was
    b0, b1 = res[False][0], res[True][0]
    assert res[False][1] == [] and b0.report.frames == 0
    assert [f for _, _, f in res[True][1]] == sent
    assert b0.key() == b1.key() and (b0.trig_dec, b0.end_dec, b0.df) == (b1.trig_dec, b1.end_dec, b1.df)
    rep = b1.report
    assert lib.ROW_TRACKED in rep.row_how and rep.frames == 1
    _, want, taken = T.second_attempt(b1.data, b1.trk.data, None, None, b1.nbrow, b1.nlbyte)
    assert taken and (rep.row_roots, rep.row_how, rep.row_changed, rep.bytes_changed, rep.rows_failed, rep.rows_rescued) == \
        tuple(want[k] for k in ("row_roots", "row_how", "row_changed", "bytes_changed", "rows_failed", "rows_rescued"))
    assert rep.row_roots == b0.report.row_roots


# the second attempt in the other instantiations of the block kernel: with and without a report, the soft and the feedback row rule
# in attempt A, every frame of a burst, a flag as six adjacent ones
COMBOS = (dict(), dict(soft_rs=True, block_report=True), dict(feedback=True, block_report=True), dict(feedback=True),
          dict(all_frames=True, block_report=True), dict(all_frames=True, raw_flags=True, block_report=True), dict(all_frames=True, raw_flags=True),
          dict(soft_rs=True, feedback=True, all_frames=True, raw_flags=True, block_report=True), dict(soft_rs=True, feedback=True, all_frames=True))


def no_7e_case(seed: int, ppm: float):
    """table_case with every info byte 0x7e made 0x7d: a frame that all-frames mode delivers without raw_flags too"""
    rng = np.random.default_rng(100 + seed)
    t0 = 0.004 + rng.uniform(0, 1 / 10500)
    info = rng.integers(0, 256, 1625, dtype=np.uint8)
    info[info == 0x7e] = 0x7d
    cfo = rng.uniform(-300, 300)
    b = synth.Burst(chan=0, t0=float(t0), info=bytes(info.tolist()), amp=30.0, cfo=float(cfo), sym_ppm=float(ppm))
    ns = S._pad(int((t0 + b.duration() + 0.006) * 2_000_000))
    return synth.synth_stream(synth.StreamSpec(rate=2_000_000, fo=(100_000,), nsamples=ns, bursts=[b], noise=1.7, seed=seed), "cs16"), b


# (sym_ppm, seed, generator, frames in all-frames mode without raw_flags): every burst of the table holds a data byte 0x7e, which cuts its
# frame in that mode -- attempt B takes rows, passes nothing, and the result is attempt A's; the third burst holds none and is delivered
SECOND = ((100, 0, table_case, 0), (-50, 3, table_case, 0), (100, 0, no_7e_case, 1))


@pytest.mark.timeout(300)
@pytest.mark.parametrize("ppm,seed,gen,all_only", SECOND)
def test_second_attempt_with_every_row_rule_and_mode(built, oracle, ppm, seed, gen, all_only):
    """a drifting burst of the table through handles with each of the other flags: the frames and the report are the model's rule
    (tracked_ref.second_attempt with that handle's feedback rows and reliability map, and that mode's frames), attempt B ran, and
    vdl2gpu_decode_blocks_tracked on the polled record gives the same"""
    raw, tx = gen(seed, ppm)
    spec = synth.StreamSpec(rate=2_000_000, fo=(100_000,), nsamples=raw.size // 2, bursts=[tx])
    for kw in COMBOS:
        with _rx(spec, "cs16", max_push=spec.nsamples, frames=True, tracked=True, **kw) as rx:
            rx.push(raw)
            (b,) = rx.poll()
            frames = [f for _, _, f in rx.poll_frames()]
            nbrow, nlbyte = b.nbrow, b.nlbyte
            if kw.get("raw_flags"):
                frames_of = lambda blk: RF.model(nbrow, nlbyte, blk.tobytes())[0]      # noqa: E731
            elif kw.get("all_frames"):
                frames_of = lambda blk: AF.model(nbrow, nlbyte, blk.tobytes())[0]      # noqa: E731
            else:
                frames_of = None
            want, rep, taken = T.second_attempt(b.data, b.trk.data, b.fb, b.soft, nbrow, nlbyte, frames_of)
            assert frames == want, kw
            if kw.get("all_frames") and not kw.get("raw_flags"):
                # without raw_flags a data byte 0x7e cuts the frame in all-frames mode: attempt B takes rows and passes nothing
                # either, and the result is attempt A's -- no frames, A's report (the model's `taken` is then empty)
                assert len(frames) == all_only and bool(taken) == bool(all_only), kw
                if kw.get("block_report") and not all_only:
                    assert lib.ROW_TRACKED not in b.report.row_how and b.report.frames == 0
            else:
                assert taken and len(frames) == 1, kw                # attempt A passed nothing, B took rows and delivered
            again = rx.decode_blocks([b], soft=None if b.soft is None else [b.soft], fb=None if b.fb is None else [b.fb],
                                     report=bool(kw.get("block_report")), all_frames=bool(kw.get("all_frames")),
                                     raw_flags=bool(kw.get("raw_flags")), trk=[b.trk.data])
            if kw.get("block_report"):
                r = b.report
                assert (r.row_roots, r.row_how, r.row_changed, r.bytes_changed, r.rows_failed, r.rows_rescued) == \
                    tuple(rep[k] for k in ("row_roots", "row_how", "row_changed", "bytes_changed", "rows_failed", "rows_rescued")), kw
                assert r.frames == len(want) and r.cand == r.too_short + r.bad_fcs + r.frames
                assert [f for _, f in again[0]] == frames and again[1][0] == r
            else:
                assert [f for _, f in again] == frames


@pytest.mark.timeout(300)
def test_tracked_changes_nothing_else_and_combines(built):
    spec = S.eight_channels()
    raw = synth.synth_stream(spec, "cs16")
    n = raw.size // 2
    pn = R.pn_bits()
    full = []
    for on in (False, True):
        with _rx(spec, "cs16", max_push=n, keep_dec=True, frames=True, levels=True, soft_rs=True, carrier=True, block_report=True,
                 feedback=True, symclk=True, all_frames=True, raw_flags=True, tracked=on) as rx:
            rx.push(raw)
            bursts = rx.poll()
            full.append(([(b.key(), b.trig_dec, b.end_dec, b.df, b.level, b.soft.tobytes(), b.carrier, b.fb.tobytes(), repr(b.clock))
                          for b in bursts], rx.stats()))
            frames = rx.poll_frames()
            assert all((b.trk is not None) == on for b in bursts)
            if on:
                _check_exact(rx, bursts, pn)
                # frames and reports by the model's rule: attempt A as the handle's flags define it (the library's own block path
                # without trk), attempt B only for a burst of which A passed nothing
                fa, ra = rx.decode_blocks(bursts, soft=[b.soft for b in bursts], fb=[b.fb for b in bursts], report=True, all_frames=True,
                                          raw_flags=True)
                ft, rt = rx.decode_blocks(bursts, soft=[b.soft for b in bursts], fb=[b.fb for b in bursts], report=True, all_frames=True,
                                          raw_flags=True, trk=[b.trk.data for b in bursts])
                assert rt == [b.report for b in bursts] and sorted(f for _, f in ft) == sorted(f for _, _, f in frames)
                for i, b in enumerate(bursts):
                    if ra[i].frames:          # no frame delivered without the rows is ever lost, and its report is A's
                        assert rt[i] == ra[i] and [f for j, f in ft if j == i] == [f for j, f in fa if j == i]
    assert len(full[0][0]) >= 10 and repr(full[0]) == repr(full[1])


@pytest.mark.timeout(600)
def test_tracked_cut_and_path_invariance(built):
    """whole; in pieces that cut inside bursts (deferred bursts); VDL2GPU_F_SERIAL; VDL2GPU_F_FULLSCAN; the burst ending on a push's
    last sample: the same columns to the byte.  Two streams, two channels, bursts on both; sym_ppm on"""
    spec = synth.random_scenario(2_000_000, S.FO8[:2], 1 << 20, seed=125, bursts_per_s=20.0, info_max=500, sym_ppm=60.0)
    raw1 = synth.synth_stream(spec, "cs16")
    spec2 = synth.random_scenario(2_000_000, S.FO8[:2], 1 << 20, seed=126, bursts_per_s=20.0, info_max=500, sym_ppm=-60.0)
    raw = np.stack([raw1, synth.synth_stream(spec2, "cs16")])
    n = raw1.size // 2
    pn = R.pn_bits()
    runs = []
    with _rx(spec, "cs16", nstreams=2, max_push=n, keep_dec=True, tracked=True) as rx:
        rx.push(raw)
        whole = rx.poll()
        _check_exact(rx, whole, pn)
        runs.append(_by_burst(whole))
    assert {(b.stream, b.chn) for b in whole} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    rng = np.random.default_rng(6)
    with _rx(spec, "cs16", nstreams=2, max_push=1 << 18, tracked=True) as rx:
        got, s = [], 0
        while s < n:
            e = min(n, s + int(rng.integers(100_000, 1 << 18)))
            rx.push(raw[:, 2 * s:2 * e])
            got += rx.poll_ready()
            s = e
        got += rx.poll()
        assert rx.stats()["deferrals"] >= 1           # a burst decoded in the push after its trigger
        runs.append(_by_burst(got))
    for kw in ({"serial": True}, {"full_scan": True}):
        with _rx(spec, "cs16", nstreams=2, max_push=1 << 18, tracked=True, **kw) as rx:
            runs.append(_by_burst(rx.run(raw)))
    # a cut right behind a burst's last sample: the push ends on the input sample that completes end_dec
    last = max((b for b in whole if b.stream == 0), key=lambda b: b.end_dec)
    cut = min(n, int((last.end_dec + 1) * 2_000_000 // 84000) + 1)
    with _rx(spec, "cs16", nstreams=2, max_push=n, tracked=True) as rx:
        rx.push(raw[:, :2 * cut])
        first = rx.poll()
        rx.push(raw[:, 2 * cut:]) if cut < n else None
        runs.append(_by_burst(first + rx.poll()))
    assert len(runs[0]) >= 10 and any(b.trk.nseg >= 2 for b in whole)
    for r in runs[1:]:
        assert r == runs[0]


@pytest.mark.timeout(300)
def test_cut_on_the_last_sample_of_a_slow_clock_burst(built):
    """The -50 ppm burst of the table ends with d_last > 0: its last symbol reads past end_dec, where samples count as 0.  With the push
    cut on the input sample that completes end_dec the plane holds nothing there yet, in the one-push run it holds the stream's noise:
    the columns are identical, and the model's"""
    raw, tx = table_case(3, -50)
    spec = synth.StreamSpec(rate=2_000_000, fo=(100_000,), nsamples=raw.size // 2, bursts=[tx])
    n = raw.size // 2
    with _rx(spec, "cs16", max_push=n, keep_dec=True, tracked=True) as rx:
        rx.push(raw)
        (whole,) = rx.poll()
        _check_exact(rx, [whole], R.pn_bits())
    assert whole.trk.d_last > 0 and whole.trk.nseg == 18
    cut = int((whole.end_dec + 1) * 2_000_000 // 84000) + 1
    assert cut < n and cut * 84000 // 2_000_000 == whole.end_dec + 1      # end_dec is the last frame the first push completes
    with _rx(spec, "cs16", max_push=n, tracked=True) as rx:
        rx.push(raw[:2 * cut])
        got = rx.poll()
        rx.push(raw[2 * cut:])
        got += rx.poll()
    assert len(got) == 1 and got[0].end_dec == whole.end_dec and got[0].trk.raw == whole.trk.raw


@pytest.mark.timeout(300)
@pytest.mark.parametrize("fmt", ["cu8", "cf32"])
def test_tracked_other_formats(built, fmt):
    spec = S.eight_channels()
    raw = synth.synth_stream(spec, fmt)
    with _rx(spec, fmt, max_push=spec.nsamples, keep_dec=True, tracked=True) as rx:
        rx.push(raw)
        bursts = rx.poll()
        assert len(bursts) >= 10
        _check_exact(rx, bursts, R.pn_bits())


@pytest.mark.timeout(300)
def test_tracked_api_edges(built):
    spec = S.eight_channels()
    raw = synth.synth_stream(spec, "cu8")
    buf = (lib.BurstT * 4096)()
    tv = (lib.TrkT * 4096)()
    with _rx(spec, "cu8", max_push=spec.nsamples) as rx:        # no F_TRACKED
        rx.push(raw)
        assert rx.L.vdl2gpu_poll_tracked(rx.h, buf, None, None, None, None, None, None, tv, 4096) == EINVAL
        assert rx.L.vdl2gpu_poll_tracked_ready(rx.h, buf, None, None, None, None, None, None, tv, 4096) == EINVAL
        assert b"trk needs VDL2GPU_F_TRACKED" in rx.L.vdl2gpu_last_error(rx.h)
        n = rx.poll_tracked_raw(buf, None, None, None, None, None, None, None, 4096)      # trk == NULL: the plain poll; nothing was consumed
        assert n >= 10
        plain = [bytes(C.string_at(C.addressof(buf[i]), C.sizeof(lib.BurstT))) for i in range(n)]
        # decode_blocks_tracked with trk == NULL is decode_blocks_ex; its EINVAL cases are that call's
        fr = (lib.FrameT * 64)()
        assert rx.L.vdl2gpu_decode_blocks_tracked(rx.h, buf, None, None, None, n, fr, 64, None, None, 2) == EINVAL
        assert rx.L.vdl2gpu_decode_blocks_tracked(rx.h, buf, None, None, tv, n, fr, 64, None, None, 4) == EINVAL
        a = rx.L.vdl2gpu_decode_blocks_tracked(rx.h, buf, None, None, None, n, fr, 64, None, None, 0)
        fa = [bytes(fr[i].data[:fr[i].len]) for i in range(a)]
        b = rx.L.vdl2gpu_decode_blocks_ex(rx.h, buf, None, None, n, fr, 64, None, None, 0)
        assert a == b >= 1 and fa == [bytes(fr[i].data[:fr[i].len]) for i in range(b)]
    with _rx(spec, "cu8", max_push=spec.nsamples, tracked=True) as rx:
        rx.push(raw)
        lv = (lib.LevelT * 4)()
        assert rx.L.vdl2gpu_poll_tracked(rx.h, buf, lv, None, None, None, None, None, tv, 4) == EINVAL     # another column the handle lacks
        m = rx.poll_tracked_raw(buf, None, None, None, None, None, None, tv, 4096)
        assert plain == [bytes(C.string_at(C.addressof(buf[i]), C.sizeof(lib.BurstT))) for i in range(m)]
        assert all(tv[i].nseg >= 1 and not any(tv[i].reserved) for i in range(m))
