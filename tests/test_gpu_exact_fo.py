"""VDL2GPU_F_EXACT_FO on the GPU: channel offsets off the 25 kHz grid, rotated inside the three K1 kernels where they dump.

Every row of exactfo_model.ROWS is one short burst per channel.  The planes are compared bit for bit with the numpy model of
tests/exactfo_model.py (P3), the records -- df bits, trigger, end and sample stamps -- with the oracle's demodulator run over the
model's planes (P2), the frames with that demodulator's frames (P1); tests/test_exact_fo.py checks on the CPU that every channel
decodes what synth sent.  Each row runs as one whole push, as ragged pushes with a run of 1-sample pushes among them (the phase
index is carried from the handle's sample count), and through the general kernel alone (VDL2GPU_NO_K1_FAST)."""
import math

import numpy as np
import pytest

import exactfo_model as X
import offgrid_model as M
import scenarios as S
import test_gpu_offgrid_rates as G
import test_gpu_rates as TR

pytestmark = pytest.mark.gpu

# the kernel that must have taken the whole periods of a whole push (vdl2gpu_debug_k1), per row of X.ROWS
FAST = ["k1_fast", "k1_pp", "k1_pp", "k1_pp", "k1_pp", None]


def _rx(rate, fos, fmt, **kw):
    from vdlm2dec_amd.demod import Receiver, plan_channels
    if fos and isinstance(fos[0], tuple):
        return Receiver(rate, [plan_channels(S.FC, f) for f in fos], fmt=fmt, **kw)
    return Receiver(rate, plan_channels(S.FC, fos), fmt=fmt, **kw)


def _want_frames(want, stream=0):
    return [(stream, c, f) for c, fr in enumerate(want["frames"]) for f in fr]


def _sizes(per, n, rng):
    """ragged pushes (test_gpu_rates._ragged) with a run of 1-sample pushes behind the first of them"""
    out = TR._ragged(per, n - 8, rng)
    out[1:1] = [1, 1, 1, 1, 1, 3]
    assert sum(out) == n
    return out


def _pushed(rx, raw, fmt, sizes, nch):
    """push the recording in parts: the planes put together from the parts' planes, and every record"""
    parts, got, pos = [[] for _ in range(nch)], [], 0
    for k in sizes:
        rx.push(raw[X.PER[fmt] * pos:X.PER[fmt] * (pos + k)])
        for c in range(nch):
            parts[c].append(rx.debug_dec(0, c))
        got += rx.poll_ready()
        pos += k
    return [np.concatenate(p) for p in parts], got + rx.poll()


def _same_planes(got, want, what):
    for c, (g, d) in enumerate(zip(got, want)):
        assert len(g) == len(d) and np.array_equal(M.bits(g), M.bits(d)), (what, c)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("row", range(len(X.ROWS)), ids=X.IDS)
def test_planes_bursts_and_frames(built, oracle, monkeypatch, row):
    rate, fmt, fos = X.ROWS[row]
    clk = rate // 4000
    want = X.expected(oracle, row)
    raw, n = want["raw"], want["spec"].nsamples
    assert all(len(f) >= 1 for f in want["frames"])          # nothing below passes empty
    monkeypatch.setenv("VDL2GPU_STAGE_EVERY", "1")
    monkeypatch.delenv("VDL2GPU_NO_K1_FAST", raising=False)
    # one whole push
    with _rx(rate, fos, fmt, max_push=n, keep_dec=True, frames=True, exact_fo=True) as rx:
        rx.push(raw)
        G._check_planes(rx, want["planes"], "whole")                            # P3
        G._check_bursts(rx.poll(), want["blocks"], clk)                         # P2
        assert sorted(rx.poll_frames()) == sorted(_want_frames(want))           # P1
        k = rx.debug_k1()
        for name in ("k1_fast", "k1_pp"):
            assert (k[name] > 0) == (FAST[row] == name) or FAST[row] is None, k
        assert k["general_global" if G._table_in_lds(rate) else "general_lds"] == 0, k
    # ragged pushes and single samples: the carried phase index
    sizes = _sizes(4 * clk, n, np.random.default_rng(rate))
    with _rx(rate, fos, fmt, max_push=max(sizes), keep_dec=True, exact_fo=True) as rx:
        planes, got = _pushed(rx, raw, fmt, sizes, len(fos))
        k = rx.debug_k1()
    _same_planes(planes, want["planes"], "ragged")
    G._check_bursts(got, want["blocks"], clk)
    assert k["general_lds" if G._table_in_lds(rate) else "general_global"] >= 6, k      # the short pushes, at least
    if FAST[row]:
        assert k[FAST[row]] > 0, k
    # the general kernel alone, with its table where the rate puts it
    monkeypatch.setenv("VDL2GPU_NO_K1_FAST", "1")
    with _rx(rate, fos, fmt, max_push=n, keep_dec=True, exact_fo=True) as rx:
        rx.push(raw)
        G._check_planes(rx, want["planes"], "general")
        G._check_bursts(rx.poll(), want["blocks"], clk)
        k = rx.debug_k1()
    lds = G._table_in_lds(rate)
    assert lds == (rate != 15_360_000)
    assert k == {"general_lds": int(lds), "general_global": int(not lds), "k1_pp": 0, "k1_fast": 0}, k


@pytest.mark.timeout(300)
def test_every_offset_on_the_grid_is_the_handle_without_the_flag(built, monkeypatch):
    rate, fmt, _ = X.ROWS[0]
    fos = (-300_000, 25_000, 250_000, 100_000)
    spec, raw = X.scenario(rate, fmt, fos)
    monkeypatch.setenv("VDL2GPU_STAGE_EVERY", "1")
    monkeypatch.delenv("VDL2GPU_NO_K1_FAST", raising=False)
    out = []
    for flag in (False, True):
        with _rx(rate, fos, fmt, max_push=spec.nsamples, keep_dec=True, exact_fo=flag) as rx:
            rx.push(raw)
            planes = [rx.debug_dec(0, c) for c in range(len(fos))]
            recs = sorted(G._gfields(b) + (b.trig_sample, b.end_sample) for b in rx.poll())
            assert rx.debug_k1()["k1_fast"] > 0
            out.append((planes, recs))
    _same_planes(out[1][0], out[0][0], "on the grid")
    assert out[0][1] == out[1][1] and len(out[0][1]) >= 3


@pytest.mark.timeout(300)
@pytest.mark.parametrize("row", (0, 1, 3), ids=[X.IDS[r] for r in (0, 1, 3)])
def test_without_the_flag_an_offset_off_the_grid_is_what_it_was(built, monkeypatch, row):
    """the reference's table of the off-grid Fo itself, jumps included: k1_fast, k1_pp and both general kernels"""
    rate, fmt, fos = X.ROWS[row]
    spec, raw = X.scenario(rate, fmt, fos)
    want = [M.channelise(raw, fmt, rate, fo) for fo in fos]
    monkeypatch.setenv("VDL2GPU_STAGE_EVERY", "1")
    for general in (False, True):
        if general:
            monkeypatch.setenv("VDL2GPU_NO_K1_FAST", "1")
        else:
            monkeypatch.delenv("VDL2GPU_NO_K1_FAST", raising=False)
        with _rx(rate, fos, fmt, max_push=spec.nsamples, keep_dec=True) as rx:
            rx.push(raw)
            G._check_planes(rx, want, ("no flag", general))
            k = rx.debug_k1()
            assert general or k[FAST[row]] > 0, k
            rx.poll()


@pytest.mark.timeout(300)
def test_two_streams_with_their_own_residuals(built, oracle, monkeypatch):
    """2 streams x 2 channels, four different Fd: 4100, 0 (a slot left alone beside one that is rotated), -12500, -8400"""
    rate, fmt = 2_000_000, "cs16"
    plans = ((-295_900, 100_000), (12_500, 241_600))
    assert [X.split(f)[1] for p in plans for f in p] == [4_100, 0, -12_500, -8_400]
    specs = [X.scenario(rate, fmt, p, seed=2 + s) for s, p in enumerate(plans)]
    n = min(sp.nsamples for sp, _ in specs)
    raws = [r[:2 * n] for _, r in specs]
    planes = [[X.channelise(r, fmt, rate, fo) for fo in p] for r, p in zip(raws, plans)]
    blocks = [[M.demod_blocks(oracle, pl, S.FC + fo, chn=c) for c, (pl, fo) in enumerate(zip(pls, p))] for pls, p in zip(planes, plans)]
    assert all(sum(len(b) for b in bl) >= 1 for bl in blocks)
    monkeypatch.setenv("VDL2GPU_STAGE_EVERY", "1")
    monkeypatch.delenv("VDL2GPU_NO_K1_FAST", raising=False)
    sizes = [8000 * 5 + 123, 1, 8000 * 4]
    sizes.append(n - sum(sizes))
    for what, szs in (("whole", [n]), ("parts", sizes)):
        with _rx(rate, plans, fmt, max_push=max(szs), keep_dec=True, exact_fo=True) as rx:
            parts, got, pos = {(s, c): [] for s in range(2) for c in range(2)}, [], 0
            for k in szs:
                rx.push(np.stack([r[2 * pos:2 * (pos + k)] for r in raws]))
                for key in parts:
                    parts[key].append(rx.debug_dec(*key))
                got += rx.poll_ready()
                pos += k
            got += rx.poll()
            assert rx.debug_k1()["k1_fast"] > 0
        for (s, c), p in parts.items():
            g, d = np.concatenate(p), planes[s][c]
            assert len(g) == len(d) and np.array_equal(M.bits(g), M.bits(d)), (what, s, c)
        for s in range(2):
            G._check_bursts(got, blocks[s], rate // 4000, s)


@pytest.mark.timeout(300)
def test_levels_frames_and_soft_rs_with_the_flag(built, oracle, monkeypatch):
    rate, fmt, fos = X.ROWS[0]
    want = X.expected(oracle, 0)
    raw, n = want["raw"], want["spec"].nsamples
    monkeypatch.setenv("VDL2GPU_STAGE_EVERY", "1")
    monkeypatch.delenv("VDL2GPU_NO_K1_FAST", raising=False)
    runs = []
    for sizes in ([n], _sizes(2000, n, np.random.default_rng(7))):
        with _rx(rate, fos, fmt, max_push=max(sizes), keep_dec=True, frames=True, levels=True, soft_rs=True, exact_fo=True) as rx:
            _, got = _pushed(rx, raw, fmt, sizes, len(fos))
            assert sorted(rx.poll_frames()) == sorted(_want_frames(want))
        G._check_bursts(got, want["blocks"], rate // 4000)
        lv = {}
        for b in got:
            assert b.level is not None and b.soft is not None and b.soft.shape == (8, 255)
            assert math.isfinite(b.level.sig_dbfs) and math.isfinite(b.level.sig_power) and b.level.sig_power > 0 and b.level.nsym > 0
            lv[(b.chn, b.end_dec)] = (M.bits(np.float32([b.level.sig_dbfs, b.level.noise_dbfs, b.level.sig_power, b.level.noise_power])).tolist(),
                                      b.level.sym_first_dec, b.level.nsym, b.level.subphase, b.level.noise_blocks, b.soft.tobytes())
        runs.append(lv)
    assert runs[0] == runs[1] and len(runs[0]) >= len(fos)
