"""The DEFINITION of vdl2gpu_trk_t and of the block path's second attempt (include/vdl2gpu.h), without a GPU: the numpy restatement
tests/tracked_ref.py on the CPU model's 84 kS/s plane.

The table (one 7-row burst a stream: 1625 random info bytes, cs16 at 2 MS/s, fo 100 kHz, amp 30, noise 1.7; seeds 0..3):
    sym_ppm   RS rows the reference fails, of 7   frames the reference delivers   frames with the tracked rows
       0      0 0 0 0                             4 of 4                          4 of 4
     +50      1 2 2 0                             1 of 4                          4 of 4
     -50      4 0 2 6                             1 of 4                          4 of 4
    +100      5 7 6 7                             0 of 4                          4 of 4
The exact model delivers the sent frame in all 16 cases; where the reference delivers none, attempt B takes all seven rows."""
import numpy as np
import pytest

import feedback_ref as F
import soft_ref as R
import tracked_ref as T

FC = 136_975_000
RATE, FO = 2_000_000, 100_000
REF_FAILS = {0: (0, 0, 0, 0), 50: (1, 2, 2, 0), -50: (4, 0, 2, 6), 100: (5, 7, 6, 7)}


def table_case(seed: int, ppm: float, noise: float = 1.7, n: int = 1625):
    """(raw cs16 stream, the transmitted Burst) of one case of the table"""
    from vdlm2dec_amd import synth
    rng = np.random.default_rng(100 + seed)
    t0 = 0.004 + rng.uniform(0, 1 / 10500)
    info = rng.integers(0, 256, n, dtype=np.uint8)
    cfo = rng.uniform(-300, 300)
    b = synth.Burst(chan=0, t0=float(t0), info=bytes(info.tolist()), amp=30.0, cfo=float(cfo), sym_ppm=float(ppm))
    ns = (int((t0 + b.duration() + 0.006) * RATE) + 32767) // 32768 * 32768
    return synth.synth_stream(synth.StreamSpec(rate=RATE, fo=(FO,), nsamples=ns, bursts=[b], noise=noise, seed=seed), "cs16"), b


_rows = {}


def table(oracle):
    """every case once per process: {(ppm, seed): dict(block, x, rb, col, sent, ref_frames, frames, taken, fails)}"""
    from vdlm2dec_amd import synth
    if _rows:
        return _rows
    pn = R.pn_bits()
    for ppm in REF_FAILS:
        for seed in range(4):
            raw, tx = table_case(seed, ppm)
            ch = oracle.OracleChannel(RATE, FO, FC + FO, tap_dec=True)
            ch.feed(raw, "cs16")
            x, trigs, blocks = ch.dec(), ch.triggers(), ch.blocks()
            ch.close()
            assert len(blocks) == 1
            b = blocks[0]
            clk = {t["dec_index"]: t["clk"] for t in trigs if t["accepted"] == 1}[b.trig_dec]
            nbrow, nlbyte, rows = synth.received_rows(tx.payload())
            col = T.burst_column(x, b.nbrow, b.nlbyte, b.df, b.end_dec, pn)
            frames, rep, taken = T.second_attempt(b.data, col["data"], None, None, b.nbrow, b.nlbyte)
            roots = F.report(b.data, None, None, b.nbrow, b.nlbyte)["row_roots"]
            _rows[(ppm, seed)] = dict(block=b, x=x, rb=R.timing(clk)[1], col=col, sent=oracle.frames_of_block(nbrow, nlbyte, rows),
                                      ref_frames=oracle.frames_of_block(b.nbrow, b.nlbyte, b.data), frames=frames, taken=taken, rep=rep,
                                      fails=sum(r < 0 for r in roots[:b.nbrow]))
    return _rows


def test_forced_reference_timing_gives_the_oracles_bytes(built, oracle):
    """with d = -rb in every segment the indices are the reference's: the assertion feedback_ref.tap_rows makes"""
    pn = R.pn_bits()
    t = table(oracle)
    for key in ((0, 0), (50, 1), (-50, 3), (100, 2)):
        c = t[key]
        b = c["block"]
        assert b.nbrow == 7
        forced = T.burst_column(c["x"], b.nbrow, b.nlbyte, b.df, b.end_dec, pn, forced=-c["rb"])
        assert forced["data"].tobytes() == b.data, key
        assert forced["nseg"] == 18 and forced["d_min"] == forced["d_max"] == -c["rb"]


def test_the_table(built, oracle):
    t = table(oracle)
    for ppm, want in REF_FAILS.items():
        fails = tuple(t[(ppm, s)]["fails"] for s in range(4))
        print(ppm, "reference fails", fails, "reference delivers", sum(t[(ppm, s)]["ref_frames"] == t[(ppm, s)]["sent"] for s in range(4)),
              "tracked delivers", sum(t[(ppm, s)]["frames"] == t[(ppm, s)]["sent"] for s in range(4)),
              "d", [(t[(ppm, s)]["col"]["d_first"], t[(ppm, s)]["col"]["d_last"]) for s in range(4)])
        assert fails == want, (ppm, fails)                       # the reference's counts are exactly the table's
    delivered = {ppm: sum(bool(t[(ppm, s)]["ref_frames"]) for s in range(4)) for ppm in REF_FAILS}
    assert delivered == {0: 4, 50: 1, -50: 1, 100: 0}
    for key, c in t.items():
        assert len(c["sent"]) == 1
        assert c["frames"] == c["sent"], key                     # all 16: every frame the reference delivers, and the 10 it does not
        if c["ref_frames"]:
            assert c["ref_frames"] == c["sent"] and c["taken"] == []      # attempt A passed: B is not run
        else:
            assert c["taken"] == list(range(7)) and c["rep"]["row_how"][:7] == (T.ROW_TRACKED,) * 7 and c["rep"]["rows_rescued"] == 7
            assert c["rep"]["row_roots"] == F.report(c["block"].data, None, None, 7, c["block"].nlbyte)["row_roots"]
    # the drift that was tracked has the sign and the size of the clock offset: 18 segments of 256 symbols at 50 ppm walk 7.4 quarter samples
    for (ppm, seed), c in t.items():
        walk = c["col"]["d_last"] - c["col"]["d_first"]
        if ppm == 0:
            assert all(abs(d - c["col"]["d"][0]) <= 2 for d in c["col"]["d"]), (seed, c["col"]["d"])
        else:
            assert abs(walk - (-ppm * 1e-6 * 17 * 256 * 32)) <= 3, (ppm, seed, walk)


def test_tie_order_on_crafted_indices():
    """a later candidate wins only with a strictly smaller cost; segment 0 tries 0, -1, -2, -3, a later one d, d - 1, d + 1"""
    assert T.choose([5, 5, 5, 5]) == 0 and T.choose([5, 4, 4, 3]) == 3 and T.choose([5, 4, 4, 4]) == 1 and T.choose([3, 4, 2]) == 2
    assert T.choose([3, 3, 2]) == 2 and T.choose([3, 2, 2]) == 1
    n = 600                                                      # three segments: 256, 256, 88
    asked = []

    def idx_of(costs_by_d):
        def f(d, i0, i1):
            asked.append((i0 // 256, d))
            v = np.full(i1 - i0, 16, np.int64)                  # e = 0 everywhere ...
            v[0] = 16 + costs_by_d.get((i0 // 256, d), 3)       # ... but one symbol whose e is the crafted number
            return v
        return f

    _, ds = T.track(idx_of({}), n)                               # all equal: the first candidate of every segment
    assert ds == [0, 0, 0] and asked == [(0, 0), (0, -1), (0, -2), (0, -3), (1, 0), (1, -1), (1, 1), (2, 0), (2, -1), (2, 1)]
    _, ds = T.track(idx_of({(0, -2): 1, (0, -3): 1, (1, -3): 2, (1, -1): 2, (2, -3): 3, (2, -4): 3, (2, -2): 1}), n)
    assert ds == [-2, -3, -2]        # 0: -2 ties -3, the earlier wins; 1: d - 1 = -3 ties d + 1 = -1, d - 1 is tried first; 2: d + 1 alone is smaller
    # idx 256 is idx 0 one turn on: e = (256 & 31) - 16 = -16
    assert T.cost([256]) == 256 and T.cost([40]) == 64 and T.cost([16, 48, 80]) == 0


def test_tie_order_cost_arithmetic():
    idx, ds = T.track(lambda d, i0, i1: np.full(i1 - i0, 256 if d == -1 else 40, np.int64), 300)
    assert ds == [0, 0] and (idx == 40).all()                    # 64 a symbol beats 256 a symbol; the first of the equal ones wins


def test_zero_rule_past_end_dec(built, oracle):
    """samples at stream times greater than end_dec count as 0 whatever the plane holds there: the column of a burst with d > 0 at its
    end does not change when garbage follows the burst's last symbol, and it does change when the rule is not applied"""
    pn = R.pn_bits()
    c = table(oracle)[(-50, 3)]                                  # d_last = +8: the last symbol reads two samples past end_dec
    b = c["block"]
    assert c["col"]["d_last"] > 0
    x = c["x"].copy()
    rng = np.random.default_rng(5)
    x[b.end_dec + 1:] = (rng.normal(0, 4000, len(x) - b.end_dec - 1) + 1j * rng.normal(0, 4000, len(x) - b.end_dec - 1)).astype(np.complex64)
    again = T.burst_column(x, b.nbrow, b.nlbyte, b.df, b.end_dec, pn)
    assert T.column_bytes(again) == T.column_bytes(c["col"])
    # without the rule (end_dec moved out) the last symbol's index sees the garbage
    i1, _ = T.burst_track(x, b.nbrow, b.nlbyte, b.df, b.end_dec)
    g = R.geom(b.nbrow, b.nlbyte)
    kmax = (25 + 8 * (g[4] + g[5]) - 1) // 3
    t = b.end_dec - 8 * (kmax - np.arange(7, kmax + 1))
    d = c["col"]["d_last"]
    ph_zero = T.phase_at(T.zeroed(x, b.end_dec), 4 * t[-2:] + d)
    ph_raw = T.phase_at(x, 4 * t[-2:] + d)
    assert ph_zero[0] == ph_raw[0] and ph_zero[1] != ph_raw[1]
    assert len(i1) == kmax - 7
