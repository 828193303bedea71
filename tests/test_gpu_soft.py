"""VDL2GPU_F_SOFT_RS on the GPU: the flag changes nothing else, the reliability maps are the definition's (tests/soft_ref.py) for every
byte of every burst on every decode path and push cut, and the soft block path -- vdl2gpu_decode_blocks_soft and the pipeline's --
gives the CPU model's frames, which at 19 and 20 dB are more correct frames than the reference's and no frame that was never sent."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import scenarios as S
import soft_cases as SC
import soft_ref as R
from vdlm2dec_amd import lib, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rx(fo, rate, fmt, nstreams=1, plans=None, **kw):
    from vdlm2dec_amd.demod import Receiver, plan_channels
    plan = plans or plan_channels(S.FC, fo)
    return Receiver(rate, plan, fmt=fmt, **kw)


def _model(raw, fmt, rate, fo, fc=S.FC, stream=0):
    """{(stream, chn, trig_dec): (oracle Block, hard, rel)}"""
    out = {}
    for c, f in enumerate(fo):
        for b, hard, rel in R.channel_maps(raw, fmt, rate, f, fc, c):
            assert hard.tobytes() == b.data
            out[(stream, c, b.trig_dec)] = (b, hard, rel)
    return out


def _check_maps(bursts, want):
    assert len(bursts) == len(want) and len(want) >= 5
    for b in bursts:
        _, hard, rel = want[(b.stream, b.chn, b.trig_dec)]
        assert b.data == hard.tobytes()
        assert b.soft is not None and np.array_equal(b.soft, rel), (b.stream, b.chn, b.trig_dec)


def _ragged(rx, raw, per, seed=5, cap=1 << 18):
    rng = np.random.default_rng(seed)
    n, s, got = raw.shape[-1] // per, 0, []
    while s < n:
        e = min(n, s + int(rng.integers(1000, cap)))
        rx.push(raw[..., per * s:per * e])
        got += rx.poll_ready()
        s = e
    return got + rx.poll()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("fmt,rate,fo", [("cu8", 2_000_000, S.FO8), ("cs16", 10_000_000, S.FO8_10MS)])
def test_soft_changes_nothing_else(built, fmt, rate, fo):
    spec = S.eight_channels(rate=rate, fo=fo)
    raw = synth.synth_stream(spec, fmt)
    res = []
    for soft in (False, True):
        with _rx(fo, rate, fmt, max_push=1 << 19, frames=True, levels=True, soft_rs=soft) as rx:
            rng = np.random.default_rng(3)
            s, n = 0, raw.size // 2
            while s < n:
                e = min(n, s + int(rng.integers(5000, 1 << 18)))
                rx.push(raw[2 * s:2 * e])
                s = e
            k = 1 << 14
            buf, lv = (lib.BurstT * k)(), (lib.LevelT * k)()
            sv = (lib.SoftT * k)() if soft else None
            m = rx.poll_soft_raw(buf, lv, sv, k)
            res.append((bytes(C.string_at(C.addressof(buf), m * C.sizeof(lib.BurstT))),
                        bytes(C.string_at(C.addressof(lv), m * C.sizeof(lib.LevelT))), m, rx.stats(), rx.poll_frames()))
    assert res[0][2] >= 10
    assert res[0][:4] == res[1][:4]
    it = iter(res[1][4])
    assert all(f in it for f in res[0][4])      # a subsequence


@pytest.mark.timeout(600)
@pytest.mark.parametrize("kw", [{}, {"serial": True}, {"full_scan": True}, {"flags": lib.F_TEST_NOREGION}],
                         ids=["default", "serial", "fullscan", "repairs"])
def test_maps_equal_the_model(built, kw):
    spec = synth.random_scenario(2_000_000, S.FO8[:4], 1 << 20, seed=93, bursts_per_s=25.0, info_max=300, noise=6.0)
    raw = synth.synth_stream(spec, "cs16")
    with _rx(spec.fo, spec.rate, "cs16", max_push=1 << 18, soft_rs=True, **kw) as rx:
        got = rx.run(raw)
        st = rx.stats()
    if kw.get("flags"):
        assert st["repairs"] + st["serial_redos"] > 0, st
    _check_maps(got, _model(raw, "cs16", spec.rate, spec.fo))


@pytest.mark.timeout(600)
def test_maps_equal_the_model_eight_streams(built):
    from vdlm2dec_amd.demod import plan_channels
    ins = S.distinct_streams(8, nsamples=1 << 19)
    want = {}
    for s, (r, fo, fc) in enumerate(ins):
        want.update(_model(r, "cs16", 2_000_000, fo, fc, stream=s))
    raw = np.stack([r for r, _, _ in ins])
    with _rx(None, 2_000_000, "cs16", plans=[plan_channels(fc, fo) for _, fo, fc in ins], max_push=raw.shape[1] // 2,
             soft_rs=True) as rx:
        rx.push(raw)
        got = rx.poll()
    _check_maps(got, want)


@pytest.mark.timeout(600)
def test_maps_do_not_depend_on_the_push_cut(built):
    spec = synth.random_scenario(2_000_000, S.FO8, 1 << 21, seed=71, bursts_per_s=20.0, info_max=400, noise=5.0)
    raw = synth.synth_stream(spec, "cs16")
    n = raw.size // 2
    runs = []
    for block in (n, 32768):
        with _rx(spec.fo, spec.rate, "cs16", max_push=block, soft_rs=True) as rx:
            runs.append({(b.chn, b.trig_dec): b.soft.tobytes() for b in rx.run(raw, block=block)})
    with _rx(spec.fo, spec.rate, "cs16", max_push=1 << 18, soft_rs=True) as rx:
        runs.append({(b.chn, b.trig_dec): b.soft.tobytes() for b in _ragged(rx, raw, 2)})
    assert len(runs[0]) >= 20
    for r in runs[1:]:
        assert r == runs[0]
    want = _model(raw, "cs16", spec.rate, spec.fo)
    assert {(c, t): v[2].tobytes() for (_, c, t), v in want.items()} == runs[0]


def _frames_of(res, n):
    out = [[] for _ in range(n)]
    for i, f in res:
        out[i].append(f)
    return out


@pytest.mark.timeout(300)
def test_decode_blocks_soft_equals_the_model_on_crafted_rows(built):
    cs = SC.cases()
    blocks = [(nbrow, nlbyte, data.tobytes()) for nbrow, nlbyte, data, _, _, _, _, _ in cs]
    maps = [rel for _, _, _, rel, _, _, _, _ in cs]
    with _rx((100_000,), 2_000_000, "cu8", max_push=1 << 16) as rx:
        got = _frames_of(rx.decode_blocks(blocks, soft=maps), len(cs))
        hard = _frames_of(rx.decode_blocks(blocks), len(cs))
        same = _frames_of(rx.decode_blocks(blocks, soft=None), len(cs))
    from oracle import oracle as O
    assert hard == same == [O.frames_of_block(b[0], b[1], b[2]) for b in blocks]
    want = [R.soft_frames(data, rel, nbrow, nlbyte) for nbrow, nlbyte, data, rel, _, _, _, _ in cs]
    assert got == want
    sent = [O.frames_of_block(nbrow, nlbyte, s.tobytes()) for nbrow, nlbyte, _, _, s, _, _, _ in cs]
    assert sum(g == s and h != s for g, s, h in zip(got, sent, hard)) >= 20        # rescued


def _scenario(esn0, seed, n=160):
    spec_ = importlib.util.spec_from_file_location("ber_curve", os.path.join(ROOT, "scripts", "ber_curve.py"))
    bc = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(bc)
    return bc.scenario(n, esn0, seed)[0], bc


@pytest.mark.timeout(900)
@pytest.mark.parametrize("esn0,seed", [(19.0, 9002), (20.0, 9003)])
def test_soft_frames_ground_truth(built, esn0, seed):
    from oracle import oracle as O
    spec, bc = _scenario(esn0, seed)
    raw = synth.synth_stream(spec, "cs16")
    sent = {}
    for b in spec.bursts:
        nbrow, nlbyte, rows = synth.received_rows(b.payload())
        sent.setdefault(b.chan, set()).update(O.frames_of_block(nbrow, nlbyte, rows))
    with _rx(spec.fo, spec.rate, "cs16", max_push=spec.nsamples, frames=True, soft_rs=True) as rx:
        rx.push(raw)
        got = rx.poll()
        pipe = sorted((c, f) for _, c, f in rx.poll_frames())
        soft = rx.decode_blocks(got, soft=[b.soft for b in got])
        hard = rx.decode_blocks(got)
    model = _model(raw, "cs16", spec.rate, spec.fo)
    _check_maps(got, model)
    soft_f = sorted((got[i].chn, f) for i, f in soft)
    hard_f = sorted((got[i].chn, f) for i, f in hard)
    want = sorted((b.chn, f) for (_, c, _), (b, hard_b, rel) in model.items()
                  for f in R.soft_frames(hard_b, rel, b.nbrow, b.nlbyte))
    assert pipe == soft_f == want
    ok_soft = {x for x in soft_f if x[1] in sent[x[0]]}
    ok_hard = {x for x in hard_f if x[1] in sent[x[0]]}
    assert all(x[1] in sent[x[0]] for x in soft_f), "a frame that was never sent"
    assert ok_hard <= ok_soft and len(ok_soft) > len(ok_hard)
