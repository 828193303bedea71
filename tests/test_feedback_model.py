"""The CPU model of the decision-feedback rows (tests/feedback_ref.py): the definition of include/vdl2gpu.h on hand-made index
sequences, and what the rule is worth on two scenarios of scripts/ber_curve.py at 18 dB.  The GPU tests (tests/test_gpu_feedback.py)
then hold the kernels to the model by equality.

Figures of the exact rule (this model): scenario(40, 18.0, seed=9300): reference 12 sent frames, with the feedback rows 21, 9 rows
taken from them, none never sent; scenario(160, 18.0, seed=9002): reference 28, feedback 68."""
import os
import sys

import numpy as np

import feedback_ref as F
import soft_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))


# --------------------------------------------------------------------------------------------------------------- the definition
def test_constant_residual_is_removed_by_mbar():
    """every slice m steps off its sector's centre: mbar == m, the residuals r_k are all 0 and o_k = idx_k - mbar"""
    rng = np.random.default_rng(1)
    for m in (-16, -7, -1, 0, 1, 9, 15):
        idx = [int(32 * s + 16 + m) for s in rng.integers(0, 8, 200)]
        mbar, o, r = F.recursion(idx)
        assert mbar == m
        assert r == [0] * len(idx)
        assert o == [(v - m) % 256 for v in idx]


def test_index_256():
    """idx = 256 is the slice at +pi: e = -16 like idx = 0, and o and r take it modulo 256"""
    a = F.recursion([256, 48, 256, 112, 80])
    b = F.recursion([0, 48, 0, 112, 80])
    assert a == b
    mbar, o, r = F.recursion([256] * 40)
    assert mbar == -16 and o == [16] * 40 and r == [0] * 40
    assert all(0 <= v <= 255 for v in a[1])


def test_negative_floors():
    """both divisions floor towards minus infinity"""
    # mbar: n = 4, S = -3 -> (2 S + n) / (2 n) = -2 / 8 -> -1 (truncation gives 0); S = -2 -> 0 / 8 -> 0; S = -6 -> -8 / 8 -> -1
    for idx, want in (([15, 15, 15, 16], -1), ([15, 15, 16, 16], 0), ([14, 14, 15, 15], -1), ([17, 17, 17, 16], 1), ([10, 10, 10, 10], -6)):
        assert F.recursion(idx)[0] == want, idx
    # c: residuals -1, 0 (mbar 0 over a long centred tail): c = 3 (-1) = -3 -> floor((-3 + 2) / 4) = -1 (truncation gives 0)
    idx = [15, 48] + [16] * 62          # S = -1, n = 64 -> mbar = floor(62 / 128) = 0
    mbar, o, r = F.recursion(idx)
    assert mbar == 0 and r[0] == -1
    assert o[1] == 48 - 1 and r[1] == 0                 # the fed-back step moved the slice by -1; it stayed in sector 1, so r = 48 - 16 - 32 = 0
    # c = 3 r1 + 2 r2 + r3 = 0 - 2 + 0 -> floor(0 / 4) = 0 one step later
    assert o[2] == 16
    # c = -2 - 1 ... explicit small case against the formula itself
    r1, r2, r3 = -3, -2, -1
    assert (3 * r1 + 2 * r2 + r3 + 2) // 4 == -3         # -12 / 4 = -3 exactly; -13 // 4 = -4:
    assert (3 * -3 + 2 * -2 + 0 + 2) // 4 == -3          # -11 / 4 -> -3 (floor), truncation gives -2


def test_one_payload_byte():
    """nbrow 1, nlbyte 1: one data byte and (nlbyte <= 2) no parity -- 8 bits in symbols 8 .. 10, n = 3"""
    g = R.geom(1, 1)
    assert (g[4], g[5]) == (1, 0)
    kmax = (25 + 8 - 1) // 3
    assert kmax == 10
    pn = np.zeros(25 + 8 * 2100, np.uint8)
    idx = [16 + 5, 112 + 5, 208 + 5]
    mbar, o, r = F.recursion(idx)
    assert mbar == 5 and o == [16, 112, 208] and r == [0, 0, 0]
    rows = F.rows_of(o, 1, 1, pn)
    assert np.count_nonzero(rows[1:]) == 0 and np.count_nonzero(rows[0, 1:]) == 0
    assert np.array_equal(rows, F.rows_of(idx, 1, 1, pn))          # 5 steps off the centre is still the same sector
    # the byte itself: bit q = 25 + i from table q % 3 at the index of symbol q / 3
    q = 25 + np.arange(8)
    want = sum(int(float(R.GREY[q[i] % 3, o[q[i] // 3 - 8]]) > 0.5) << i for i in range(8))
    assert rows[0, 0] == want


def test_row_rule_order(oracle):
    """a row the reference decodes is kept even where the feedback row differs; a row it cannot decode is taken from a feedback row
    that decodes; with neither the soft trials run on the received row"""
    import rs_cases
    good = rs_cases.codewords()[0].copy()
    data = np.zeros((8, 255), np.uint8)
    fb = np.zeros((8, 255), np.uint8)
    bad = good.copy()
    bad[[3, 50, 99, 200]] ^= 0x5a                           # four errors: rs() gives up
    data[0], fb[0] = bad, good
    data[1], fb[1] = good, bad                              # the reference decodes: fb is ignored
    data[2] = good
    out, how = F.row_rule(data, fb, None, 3, 249)
    assert how == [F.ROW_FEEDBACK, F.ROW_CLEAN, F.ROW_CLEAN]
    assert np.array_equal(out[0], good) and np.array_equal(out[1], good)
    out, how = F.row_rule(data, None, None, 3, 249)
    assert how == [F.ROW_FAIL, F.ROW_CLEAN, F.ROW_CLEAN]


# ------------------------------------------------------------------------------------------------------------- what it is worth
def _count(nbursts, seed):
    import ber_curve as B
    from vdlm2dec_amd import synth
    spec, _ = B.scenario(nbursts, 18.0, seed=seed)
    raw = synth.synth_stream(spec, "cs16")
    sent, hard, feed, taken, recs = F.scenario_frames(spec, raw, B.FO, B.FC)
    return sent, hard, feed, taken, recs, spec


def test_scenario_40_bursts_18db(oracle):
    sent, hard, feed, taken, recs, spec = _count(40, 9300)
    print("samples", spec.nsamples, "records", len(recs), "hard", len(hard & sent), "feedback", len(feed & sent), "rows taken", taken, "never sent", len(feed - sent))
    assert len(hard & sent) == 12
    assert len(feed & sent) >= 19
    assert feed >= hard
    assert len(feed - sent) == 0 and len(hard - sent) == 0


def test_scenario_160_bursts_18db(oracle):
    sent, hard, feed, taken, recs, _ = _count(160, 9002)
    print("hard", len(hard & sent), "feedback", len(feed & sent), "rows taken", taken, "never sent", len(feed - sent))
    assert len(hard & sent) == 28
    assert len(feed & sent) >= 60
    assert feed >= hard
    assert len(feed - sent) == 0
