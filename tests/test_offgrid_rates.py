"""Sample rates off the 25 kHz grid, the host side (no GPU): the table length, the table, what vdl2gpu_create accepts, and the two
yardsticks of tests/offgrid_model.py pinned to the oracle where the oracle is valid."""
import ctypes as C

import numpy as np
import pytest

import offgrid_model as M
import scenarios as S
from vdlm2dec_amd import synth

OFFGRID_LEN = {2_048_000: 2048, 1_024_000: 1024, 2_560_000: 512, 1_920_000: 384, 2_880_000: 576, 3_840_000: 768, 7_680_000: 1536,
               15_360_000: 3072, 30_720_000: 6144}
EINVAL, ENODEV = -1, -5


def test_lo_len(built):
    import test_gpu_rates as TR
    from vdlm2dec_amd import lib
    L = lib.load()
    for rate in sorted({r for r, *_ in TR.MATRIX} | {r for r, *_ in TR.LAYOUTS} | {2_400_000, 5_000_000, 6_000_000, 10_000_000}):
        assert rate % 25000 == 0 and L.vdl2gpu_lo_len(rate) == rate // 25000, rate
    for rate, n in OFFGRID_LEN.items():
        assert L.vdl2gpu_lo_len(rate) == n, rate


@pytest.mark.parametrize("rate", [2_048_000, 30_720_000])
def test_lo_table_over_its_true_period(built, oracle, rate):
    """vdl2gpu_lo_table fills vdl2gpu_lo_len entries of wf[n] = cexpf(-n * Fo * I): where the oracle's table reaches (rate // 25000
    entries of the same formula) the two are bit-equal, and every entry is libm's sinf / cosf of the float-narrowed phase
    (float)(-n) * (float)((double)((float)fo / (float)rate) * 2 pi), as the helper documents."""
    from vdlm2dec_amd import lib
    from vdlm2dec_amd.demod import lo_table
    L = lib.load()
    libm = C.CDLL("libm.so.6")
    libm.sinf.restype = libm.cosf.restype = C.c_float
    libm.sinf.argtypes = libm.cosf.argtypes = [C.c_float]
    n = OFFGRID_LEN[rate]
    rng = np.random.default_rng(rate)
    fos = [-450000, -50000, 100000, 25000, 975000, -123457, 1] + [int(v) for v in rng.integers(-rate // 2, rate // 2, 40)]
    for k, fo in enumerate(fos):
        t = lo_table(rate, fo)
        assert len(t) == n
        ch = oracle.OracleChannel(rate, fo, 136_000_000 + fo)
        o = ch.lo_table()
        ch.close()
        assert len(o) == rate // 25000 and np.array_equal(M.bits(o), M.bits(t[:len(o)])), fo
        if k < 9:
            w = np.float32(np.float64(np.float32(fo) / np.float32(rate)) * 2.0 * np.pi)
            y = (-np.arange(n)).astype(np.float32) * w
            want = np.array([[libm.cosf(float(v)), libm.sinf(float(v))] for v in y], np.float32)
            assert np.array_equal(M.bits(want), M.bits(t).reshape(-1, 2)), fo
    buf = np.empty(2 * n, np.float32)
    assert L.vdl2gpu_lo_table(rate, 100000, buf.ctypes.data_as(C.c_void_p), n - 1) == EINVAL
    assert L.vdl2gpu_lo_table(rate, 100000, buf.ctypes.data_as(C.c_void_p), rate // 25000) == EINVAL
    assert L.vdl2gpu_lo_table(rate, 100000, buf.ctypes.data_as(C.c_void_p), n) == n


def _create(rate, sdrclk=0, fmt=1, flags=0, fo=0):
    import torch  # noqa: F401  (the library binds to torch's HIP runtime)
    from vdlm2dec_amd import lib
    L = lib.load()
    chan = (lib.ChanT * 1)(lib.ChanT(0, 136_975_000 + fo, fo))
    cfg = lib.ConfigT(struct_size=C.sizeof(lib.ConfigT), sdrinrate=rate, sdrclk=sdrclk, fmt=fmt, nbch=1, nstreams=1, chan=chan,
                      max_push=1 << 16, flags=flags)
    h = C.c_void_p()
    rc = L.vdl2gpu_create(C.byref(cfg), C.byref(h))
    if rc == 0:
        L.vdl2gpu_destroy(h)
    return rc


@pytest.mark.parametrize("rate", sorted(OFFGRID_LEN))
def test_create_accepts_offgrid_rates(built, rate):
    """past the configuration checks: a handle on a GPU, ENODEV without one"""
    import torch
    assert _create(rate) == (0 if torch.cuda.is_available() else ENODEV)
    assert _create(rate, fo=-300_000) != EINVAL


@pytest.mark.parametrize("rate,sdrclk,fmt,flags", [
    (61_440_000, 0, 1, 0),          # windows of 732 samples: the window part of the LDS alone is 234 KB
    (2_000_001, 0, 1, 0), (2_049_000, 0, 1, 0),     # 2.049 MS/s: SDRCLK 512, 2048 inputs a period, a table of 2049
    (2_048_000, 500, 1, 0),         # a custom SDRCLK whose period (2000 inputs) is no whole number of tables
    (2_048_000, 0, 0, 32),          # VDL2GPU_F_RTL_QUIRK (cu8) off the grid
    (2_048_500, 0, 1, 0), (99_000, 0, 1, 0), (44_000_000, 0, 1, 0),
])
def test_create_rejects_offgrid(built, rate, sdrclk, fmt, flags):
    assert _create(rate, sdrclk, fmt, flags) == EINVAL


def test_2050k_is_on_the_grid(built):
    """2.05 MS/s is 82 x 25 kHz: a rate on the grid, accepted before this feature (a table of 82, the general kernel, like 2.025
    MS/s in test_gpu_rates.py) and therefore after it -- on the grid nothing changes.  Its off-grid neighbour 2.049 MS/s is the
    rate whose period is no whole number of tables (test_create_rejects_offgrid)."""
    assert 2_050_000 % 25_000 == 0 and _create(2_050_000) != EINVAL


def test_create_offgrid_ceiling(built):
    """at the default SDRCLK the window part, 320 * maxwin bytes, fits 160 KiB up to maxwin = 512: SDRCLK 10752, 43.008 MS/s"""
    assert _create(42_928_000) != EINVAL and _create(43_008_000) != EINVAL and _create(43_012_000) == EINVAL
    assert _create(2_048_000, 10752) != EINVAL      # 43008 inputs a period = 21 tables of 2048; maxwin 512
    assert _create(2_048_000, 11264) == EINVAL      # 22 tables, maxwin 537
    # windows many tables long (maxwin 512 against L = 128 and 21): accepted, the global-table kernel wraps its index by a true
    # modulo (tests/test_gpu_offgrid_rates.py::test_windows_longer_than_the_table); a period that is no whole tables is not
    assert _create(128_000, 10752) != EINVAL and _create(105_000, 10752) != EINVAL
    assert _create(128_000, 10751) == EINVAL and _create(105_000, 10753) == EINVAL


@pytest.mark.parametrize("rate,sdrclk,ok", [
    (25_700_000, 0, True), (25_725_000, 0, False), (2_000_000, 10416, True), (2_000_000, 10417, False),
    (100_000, 10731, True), (100_000, 10732, False), (2_000_000, 1_000_000, False), (4_000_000_000, 0, False),
])
def test_on_grid_acceptance_is_unchanged(built, rate, sdrclk, ok):
    """the cases of test_abi.py::test_create_rejects_what_the_channeliser_cannot_launch: on the grid the whole LDS, table included"""
    rc = _create(rate, sdrclk)
    assert (rc != EINVAL) == ok, rc
    assert _create(2_000_000, 0, 0, 32) != EINVAL       # and the quirk stays what it was there


# ------------------------------------------------------------------------------------------------- the channeliser model
def _oracle_dec(O, raw, fmt, rate, fo):
    ch = O.OracleChannel(rate, fo, S.FC + fo, tap_dec=True)
    a, f = M.oracle_input(raw, fmt)
    ch.feed(a, f)
    d, b = ch.dec(), ch.blocks()
    ch.close()
    return d, b


@pytest.mark.parametrize("rate,fmt,fos", [
    (2_000_000, "cu8", (-450_000, 300_000)), (2_400_000, "cs16", (-600_000, 850_000)), (5_000_000, "f32", (600_000, 2_000_000)),
    (10_000_000, "cs8", (-2_250_000, 2_300_000)), (2_000_000, "s16", (250_000, 800_000)), (2_000_000, "cf32", (-50_000, 25_000)),
    (2_048_000, "cu8", (0,)), (7_680_000, "cs16", (0,)), (2_048_000, "f32", (0,)),
])
def test_model_equals_oracle_where_the_oracle_is_valid(built, oracle, rate, fmt, fos):
    """On the grid with off-centre channels, and off it at Fo = 0 (the oracle's short table is all 1 - 0j there, and so is every
    entry of the long one): the model's plane is the oracle's vo_dec_tap, bit for bit."""
    spec = S.regimes(rate=rate, fo=fos, seed=rate // 1000, infos=(3, 40), gap=0.001)
    raw = synth.synth_stream(spec, fmt)
    for fo in fos:
        d, _ = _oracle_dec(oracle, raw, fmt, rate, fo)
        m = M.channelise(raw, fmt, rate, fo)
        assert len(m) == len(d) and np.array_equal(M.bits(m), M.bits(d)), fo


# ------------------------------------------------------------------------------------------------- the demodulator-only oracle
@pytest.mark.parametrize("rate,fmt", [(2_000_000, "cu8"), (10_000_000, "cs16"), (5_000_000, "f32")])
def test_demod_only_oracle_reproduces_the_oracle(built, oracle, rate, fmt):
    """The oracle's own planes fed back through an oracle at 84 kS/s, SDRCLK 21, Fo = 0 give the oracle's own blocks: nbrow, nlbyte,
    df bits, ppm bits, trig_dec, end_dec and every data byte.  (A sample passes that channeliser as x * (1 - 0j) / 1: unchanged but
    for the sign of a zero, which no later stage tells apart -- the blocks are equal in every field.)"""
    fos = {"cu8": (-450_000, 300_000), "cs16": (-2_250_000, 475_000), "f32": (425_000, 2_200_000)}[fmt]
    spec = S.regimes(rate=rate, fo=fos, seed=77, infos=(1, 3, 28, 66, 120, 250))
    raw = synth.synth_stream(spec, fmt)
    total = 0
    for c, fo in enumerate(fos):
        d, blocks = _oracle_dec(oracle, raw, fmt, rate, fo)
        again = M.demod_blocks(oracle, d, S.FC + fo)
        assert [M.block_fields(b) for b in again] == [M.block_fields(b) for b in blocks], fo
        total += len(blocks)
    assert total >= 5


# ------------------------------------------------------------------------------------------------- scenarios of the GPU tests
def test_gpu_scenarios_decode_on_the_cpu(built, oracle):
    """Every scenario of tests/test_gpu_offgrid_rates.py decodes at least one CRC-clean frame on every channel through the model
    and the demodulator-only oracle: the GPU comparison there has something to compare."""
    import test_gpu_offgrid_rates as G
    for rate, fmt, nch in G.SCENARIOS:
        spec, raw = G.scenario(rate, fmt, nch)
        want = G.expected(oracle, raw, fmt, rate, spec.fo)
        for c in range(nch):
            frames = [f for b in want["blocks"][c] for f in oracle.frames_of_block(b.nbrow, b.nlbyte, b.data)]
            assert len(frames) >= 1, (rate, fmt, c)


def test_receiver_and_synth_cli_take_2048k(built, tmp_path):
    import torch
    from vdlm2dec_amd import lib
    from vdlm2dec_amd.demod import Receiver, plan_channels
    out, truth = tmp_path / "a.cu8", tmp_path / "a.json"
    assert synth._cli([str(out), "--rate", "2048000", "--seconds", "0.05", "--fo", "-300000", "100000", "--truth", str(truth)]) == 0
    assert out.stat().st_size == 2 * ((int(0.05 * 2_048_000) + 32767) // 32768 * 32768)
    try:
        with Receiver(2_048_000, plan_channels(S.FC, (-300_000, 100_000)), fmt="cu8") as rx:
            assert torch.cuda.is_available() and rx.h
    except lib.Vdl2GpuError as e:
        assert not torch.cuda.is_available() and "no HIP device" in str(e)      # past the configuration checks
