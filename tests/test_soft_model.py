"""The CPU model of soft-decision RS erasures (tests/soft_ref.py) without a GPU: its hard bytes are the oracle's, the row rule does
what include/vdl2gpu.h says on crafted rows, and on the Es/N0 curve it gains frames and never makes up one."""
import importlib.util
import os

import numpy as np
import pytest

import scenarios as S
import soft_cases as SC
import soft_ref as R
from vdlm2dec_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reliability_table():
    g = R.GREY.astype(np.float64)
    for w in range(3):
        for i in range(257):
            assert R.REL[w, i] == min(255, int(np.floor(abs(g[w, i] - 0.5) * 512)))
    assert R.REL.max() == 255 and R.REL.min() == 0


@pytest.mark.parametrize("name,fmt,fo", [("regimes", "cu8", None), ("eight", "cs16", None), ("noisy", "cs16", S.FO8[:4])])
def test_model_hard_bytes_are_the_oracles(oracle, name, fmt, fo):
    if name == "regimes":
        spec = S.regimes(noise=4.0)
    elif name == "eight":
        spec = S.eight_channels(rate=10_000_000, fo=S.FO8_10MS)
    else:
        spec = synth.random_scenario(2_000_000, fo, 1 << 20, seed=93, bursts_per_s=25.0, info_max=300, noise=6.0)
    raw = synth.synth_stream(spec, fmt)
    n = 0
    for c, f in enumerate(spec.fo):
        for b, hard, rel in R.channel_maps(raw, fmt, spec.rate, f, S.FC, c):
            assert hard.tobytes() == b.data
            g = R.geom(b.nbrow, b.nlbyte)
            assert int((rel < 255).sum()) <= g[4] + g[5]
            n += 1
    assert n >= 10


def test_scatter_is_a_bijection_onto_the_transmitted_bytes():
    for nbrow in range(1, 9):
        for nlbyte in (0, 1, 2, 3, 30, 31, 67, 68, 249):
            g = R.geom(nbrow, nlbyte)
            pos = {R.scatter(b, g) for b in range(g[4] + g[5])}
            assert len(pos) == g[4] + g[5]
            for r in range(nbrow):
                by, eras, p = R.row_params(r, nbrow, nlbyte)
                assert all((r, c) in pos for c in range(249, 249 + p))
                assert not any((r, c) in pos for c in range(249 + p, 255))


def test_crafted_rows(oracle):
    """Full rows: 4 errors on the 4 least reliable bytes are always rescued (2 erased, 2 corrected) unless the reference's own rs()
    miscorrects the row first (then it is not touched); 5 are rescued by the trial with 4 erasures whenever the one with 2 does not
    end on a wrong codeword.  Short last rows (2 fixed erasures): 2 or 3 errors.  Errors on reliable bytes are never rescued (the
    trials then end on a wrong codeword or fail) and never give a frame that was not sent."""
    rescued = {}
    for nbrow, nlbyte, data, rel, sent, r, nerr, least in SC.cases():
        blk, how = R.row_rule(data, rel, nbrow, nlbyte)
        want = oracle.frames_of_block(nbrow, nlbyte, sent.tobytes())
        hard = oracle.frames_of_block(nbrow, nlbyte, data.tobytes())
        got = oracle.frames_of_block(nbrow, nlbyte, blk.tobytes())
        assert got == hard or got == want
        assert all(f in want for f in got)
        # rows the reference decodes are never touched; nothing but row r changes
        ref = np.frombuffer(data.tobytes(), np.uint8).reshape(8, 255).copy()
        for rr in range(nbrow):
            by, eras, _ = R.row_params(rr, nbrow, nlbyte)
            R.rs_decode(ref[rr], eras)
        for rr in range(nbrow):
            if how[rr] in ("ref", "fail"):
                assert np.array_equal(blk[rr], ref[rr])
            else:
                assert rr == r and R.syndromes_zero(blk[rr])
        if least and nerr == 4 and how[r] != "ref":
            assert how[r] == "s2" and got == want and got != hard
        key = (nerr, least)
        rescued.setdefault(key, [0, 0])
        rescued[key][0] += got == want and got != hard
        rescued[key][1] += 1
    assert rescued[(4, True)][0] >= 30 and rescued[(5, True)][0] >= 10 and rescued[(3, True)][0] >= 1
    assert rescued[(4, False)][0] == rescued[(5, False)][0] == 0
    nb = {c[0] for c in SC.cases()}
    assert nb == set(range(1, 9))


def _ber_curve():
    spec_ = importlib.util.spec_from_file_location("ber_curve", os.path.join(ROOT, "scripts", "ber_curve.py"))
    bc = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(bc)
    return bc


@pytest.mark.timeout(600)
def test_curve_gains_frames_and_makes_none_up(oracle):
    """ber_curve.py's scenario at 18, 19 and 20 dB (its seeds for --esn0 17 18 19 20 21): soft mode keeps every hard-mode frame, adds
    some, and every frame it gives was sent."""
    bc = _ber_curve()
    gain = 0
    for esn0, seed in ((18.0, 9001), (19.0, 9002), (20.0, 9003)):
        spec, _ = bc.scenario(160, esn0, seed)
        raw = synth.synth_stream(spec, "cs16")
        sent = {}
        for b in spec.bursts:
            nbrow, nlbyte, rows = synth.received_rows(b.payload())
            sent.setdefault(b.chan, set()).update(oracle.frames_of_block(nbrow, nlbyte, rows))
        hard, soft = set(), set()
        for c, fo in enumerate(spec.fo):
            for b, h, rel in R.channel_maps(raw, "cs16", spec.rate, fo, S.FC, c):
                hf = oracle.frames_of_block(b.nbrow, b.nlbyte, b.data)
                sf = R.soft_frames(h, rel, b.nbrow, b.nlbyte)
                assert all(f in sent[c] for f in sf), "a frame that was never sent"
                hard.update((c, f) for f in hf if f in sent[c])
                soft.update((c, f) for f in sf)
        assert hard <= soft
        gain += len(soft) - len(hard)
    assert gain >= 5
