"""The host's arithmetic on stream time where a receiver that runs for days takes it: vdl2gpu_plan and vdl2gpu_exact_fo_index around
2^31 and 2^32 input samples, 2^31 and 2^32 decimated frames and 2^40 input samples against Python integers, and the stream epoch of
the test build (VDL2GPU_TEST_EPOCH; tests/epoch_rule.py states which T0 are admissible, tests/test_gpu_epoch.py runs them): refused
by vdl2gpu_create before any device call, so all of this runs without a GPU.  (tests/test_exact_fo.py holds the index at 0, 2 R and
2^40 already; what is added here are the 32-bit boundaries of both time axes.)"""
import ctypes as C

import pytest

import epoch_rule as E
from vdlm2dec_amd import demod, lib

# SDRCLK -> a sample rate whose LO table goes with it (22: custom SDRCLK at 2 MS/s)
CLK_RATE = {22: 2_000_000, 500: 2_000_000, 512: 2_048_000, 2500: 10_000_000, 7680: 30_720_000}


def _around(clk):
    win, per = (clk + 20) // 21, 4 * clk
    centres = [1 << 31, 1 << 32, (1 << 31) * clk // 21, (1 << 32) * clk // 21, 1 << 40]
    return sorted({c + s * d for c in centres for d in (0, 1, win, per) for s in (-1, 1)}), win, per


@pytest.mark.parametrize("clk", sorted(CLK_RATE))
def test_plan_equals_big_integer_arithmetic(built, clk):
    L = E.lo_len(CLK_RATE[clk])
    totals, win, per = _around(clk)
    for total in totals:
        for n in (0, 1, win, per - 1, 16 * clk + 7, (1 << 31) + 5):
            t21 = 21 * total
            done, c0 = divmod(t21, clk)
            first = (done * clk + 20) // 21
            want = (c0, total % L, total - first, (c0 + 21 * n) // clk)
            assert demod.plan(total, n, clk, L) == want, (total, n)
            assert 0 <= want[2] <= win
        # the outputs of two pushes that meet at `total` are the outputs of one push over both
        a = demod.plan(total - per - 3, per + 3, clk, L)[3] + demod.plan(total, 2 * per + 1, clk, L)[3]
        assert a == demod.plan(total - per - 3, 3 * per + 4, clk, L)[3]


@pytest.mark.parametrize("rate", (2_000_000, 2_048_000, 30_720_000))
def test_exact_fo_index_at_the_32_bit_boundaries(built, rate):
    m2, clk = 2 * rate, rate // 4000
    totals, win, _ = _around(clk)
    for fd in (-12_500, 12_499):
        for a in totals:
            for e in (a, a + win - 1, a + win):
                assert demod.exact_fo_index(a, e, rate, fd) == ((fd % m2) * ((a + e) % m2)) % m2, (a, e, fd)
        # the per-push base (vdl2gpu_push): the phase index per Hz of the schedule period that begins at input qin
        for total in totals:
            qin = 21 * total // clk // 21 * clk
            assert demod.exact_fo_index(qin, qin, rate, 1) == (2 * qin) % m2


def test_the_epoch_rule():
    q = E.quantum(2_000_000)
    assert q == 8000 and E.d0(q, 500) == 336
    assert E.quantum(2_000_000, quirk=True) == 4_096_000 and E.quantum(2_000_000, pure_shift=True) == 4_000_000
    assert E.quantum(100_000, 42) == 672 and E.d0(672, 42) == 336
    assert E.quantum(10_000_000) == 40_000 and E.quantum(5_000_000) == 20_000
    for rate in (2_048_000, 15_360_000, 30_720_000):
        qq = E.quantum(rate)
        assert qq % E.lo_len(rate) == 0 and qq % (16 * (rate // 4000)) == 0 and E.d0(qq, rate // 4000) % 336 == 0
    assert E.admissible(0, 2_000_000) and E.admissible(8000 * 12345, 2_000_000) and not E.admissible(8000 * 12345 + 80, 2_000_000)
    assert not E.admissible(8000, 2_000_000, quirk=True) and E.admissible(4_096_000, 2_000_000, quirk=True)

    class B:            # an oracle block's stamps
        def __init__(self, trig_dec, end_dec):
            self.trig_dec, self.end_dec = trig_dec, end_dec
    blocks = [B(3000, 3500), B(5000, 9000), B(12000, 12600)]
    for name, bnd in E.BOUNDARIES.items():
        t0 = E.epoch_for(bnd, 5000, 500, q)
        assert E.admissible(t0, 2_000_000)
        assert name == "big40" or blocks[1] not in E.crossing(bnd, t0 + q, 500, blocks)[1]      # the largest such T0
        before, across, after = E.crossing(bnd, t0, 500, blocks)
        if name == "big40":
            assert t0 - q < 1 << 40 <= t0 and (before, across, after) == ([], [], blocks)
        else:
            assert (before, across, after) == ([blocks[0]], [blocks[1]], [blocks[2]]), name


def _create(L, rate, flags=0, fmt=0, sdrclk=0):
    chan = (lib.ChanT * 1)(lib.ChanT(0, 136_975_000, 0))
    cfg = lib.ConfigT(struct_size=C.sizeof(lib.ConfigT), sdrinrate=rate, sdrclk=sdrclk, fmt=fmt, nbch=1, nstreams=1, chan=chan,
                      max_push=32768, flags=flags)
    h = C.c_void_p()
    rc = L.vdl2gpu_create(C.byref(cfg), C.byref(h))
    if rc == 0:
        L.vdl2gpu_destroy(h)
    return rc


@pytest.mark.parametrize("rate,flags,sdrclk", [(2_000_000, 0, 0), (2_000_000, lib.F_RTL_QUIRK, 0), (2_048_000, 0, 0), (15_360_000, 0, 0),
                                               (100_000, 0, 42), (2_000_000, lib.F_EXACT_FO, 0)])
def test_create_refuses_an_inadmissible_epoch_before_any_device_call(built, monkeypatch, rate, flags, sdrclk):
    """the test build returns VDL2GPU_EINVAL for a T0 off the rule whatever the machine (a handle, or ENODEV without a GPU, for one
    on it); the product library never reads the variable"""
    prod, test = lib.load(), lib.load(testhooks=True)
    clk = sdrclk or rate // 4000
    quirk = bool(flags & lib.F_RTL_QUIRK)
    q = E.quantum(rate, sdrclk, quirk)
    good = [0, q, ((1 << 32) // q) * q, ((1 << 40) // q) * q, (1 << 56) // q * q]
    bad = [1, q - 1, q // 2, (1 << 32) // q * q + 1, ((1 << 56) // q + 1) * q]
    bad += [q + x for x in (16 * clk, E.lo_len(rate)) if x != q]        # one condition of the rule met, not all
    if quirk:
        bad += [8000 * 3, 32768 * 3]
    for t0 in good + bad:
        assert E.admissible(t0, rate, sdrclk, quirk) == (t0 in good), t0
        monkeypatch.setenv("VDL2GPU_TEST_EPOCH", str(t0))
        rc = _create(test, rate, flags, sdrclk=sdrclk)
        assert (rc == E.EINVAL) == (t0 in bad) and rc in (0, -5, E.EINVAL), (t0, rc)
        assert _create(prod, rate, flags, sdrclk=sdrclk) in (0, -5), t0
    for text in ("", "x", "-8000", "+8000", " 8000", "8000x", " 8000 ", "1e6", "99999999999999999999999"):
        monkeypatch.setenv("VDL2GPU_TEST_EPOCH", text)
        assert _create(test, rate, flags, sdrclk=sdrclk) == E.EINVAL, text
        assert _create(prod, rate, flags, sdrclk=sdrclk) in (0, -5), text


def test_create_refuses_a_first_ticket_that_is_no_32_bit_number(built, monkeypatch):
    """VDL2GPU_TEST_TICKET0 is parsed as strictly as the epoch: decimal digits, at most 2^32 - 1; the product library reads neither"""
    prod, test = lib.load(), lib.load(testhooks=True)
    monkeypatch.delenv("VDL2GPU_TEST_EPOCH", raising=False)
    for text, ok in (("0", True), ("3", True), (str((1 << 32) - 1), True), (str(1 << 32), False), ("", False), ("x", False), ("-1", False),
                     ("+1", False), (" 7", False), ("7 ", False), ("0x10", False), ("99999999999999999999999", False)):
        monkeypatch.setenv("VDL2GPU_TEST_TICKET0", text)
        rc = _create(test, 2_000_000)
        assert (rc in (0, -5)) == ok and (ok or rc == E.EINVAL), (text, rc)
        assert _create(prod, 2_000_000) in (0, -5), text


def test_python_mirror_keeps_64_bit_stamps():
    for T, names in ((lib.BurstT, ("trig_dec", "end_dec", "trig_sample", "end_sample")), (lib.LevelT, ("sym_first_dec",)),
                     (lib.FrameT, ("trig_dec", "end_dec"))):
        v = T()
        for n in names:
            setattr(v, n, (1 << 40) + 12345)
            assert getattr(v, n) == (1 << 40) + 12345, (T.__name__, n)
    st = lib.StatsT()
    st.samples_in = st.dec_samples = (1 << 63) + 5
    assert st.samples_in == st.dec_samples == (1 << 63) + 5
