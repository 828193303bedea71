"""VDL2GPU_F_EXACT_FO on the CPU: the two host helpers against Python integers and numpy float64, the model of
tests/exactfo_model.py against offgrid_model where the flag changes nothing, and the GPU test's scenarios through the oracle's
demodulator -- every channel decodes with the rotation, and the channels half a grid step off do not without it."""
import numpy as np
import pytest

import exactfo_model as X
import offgrid_model as M
import scenarios as S
from vdlm2dec_amd import demod

RATES = (100_000, 2_000_000, 2_048_000, 30_720_000)
FDS = (-12_500, -1, 1, 4_100, 12_499)


def test_split_of_an_offset(built):
    for fo, want in ((0, (0, 0)), (12_499, (0, 12_499)), (12_500, (25_000, -12_500)), (-12_500, (0, -12_500)),
                     (-12_501, (-25_000, 12_499)), (-24_999, (-25_000, 1)), (4_100, (0, 4_100)), (-295_900, (-300_000, 4_100)),
                     (1_004_100, (1_000_000, 4_100)), (237_500, (250_000, -12_500))):
        assert X.split(fo) == want == demod.exact_fo_split(fo), fo
        assert want[0] % 25_000 == 0 and -12_500 <= want[1] < 12_500


@pytest.mark.parametrize("rate", RATES)
def test_index_equals_big_integer_arithmetic(built, rate):
    rng = np.random.default_rng(rate)
    m2 = 2 * rate
    edge = [0, 1, m2 - 1, m2, m2 + 1, (1 << 40) - 1, 1 << 40]
    pairs = [(a, e) for a in edge for e in edge] + [(int(a), int(a + w)) for a, w in zip(rng.integers(0, 1 << 40, 200), rng.integers(0, 600, 200))]
    for fd in FDS:
        for a, e in pairs:
            assert demod.exact_fo_index(a, e, rate, fd) == ((fd % m2) * ((a + e) % m2)) % m2, (a, e, fd)


@pytest.mark.parametrize("rate", RATES)
def test_tables_within_an_ulp_of_float64(built, rate):
    """glibc's and numpy's double cos / sin may differ in the last place, so the narrowed values by one float32 ulp"""
    hi, lo = demod.exact_fo_tables(rate)
    assert len(hi) == -(-2 * rate // 4096) and len(lo) == 4096
    for tab, k in ((hi, 4096 * np.arange(len(hi), dtype=np.float64)), (lo, np.arange(4096, dtype=np.float64))):
        th = -np.pi * k / rate
        for got, ref in ((tab.real, np.cos(th).astype(np.float32)), (tab.imag, np.sin(th).astype(np.float32))):
            assert np.all(np.abs(got.astype(np.float64) - ref) <= np.spacing(np.abs(ref)).astype(np.float64))
    assert hi[0] == 1 and lo[0] == 1
    assert np.all(np.abs(np.abs(X.cmul(hi[:, None], lo[None, ::64]).astype(np.complex128)) - 1) < 2e-7)


def test_schedule_increments(built):
    """what the kernels step by: within a schedule period of 21 outputs k advances by fd * (nf_j + nf_j+1), across periods by
    2 * fd * SDRCLK, all mod 2R"""
    for rate, fd in ((2_000_000, 4_100), (2_048_000, -12_500), (100_000, 1)):
        clk, m2 = rate // 4000, 2 * rate
        k = X.indices(60 * clk, rate, fd)
        ends = M.window_ends(60 * clk, clk, demod._lib.load().vdl2gpu_lo_len(rate))
        nf = np.diff(np.concatenate([[-1], ends]))
        f = fd % m2
        assert all((k[j + 1] - k[j]) % m2 == f * int(nf[j] + nf[j + 1]) % m2 for j in range(len(k) - 1))
        assert all((k[j + 21] - k[j]) % m2 == 2 * f * clk % m2 for j in range(len(k) - 21))


def test_model_without_a_residual_is_the_plain_model(built):
    rng = np.random.default_rng(5)
    raw = rng.integers(-3000, 3000, 2 * 40_000, dtype=np.int16)
    for fo in (0, 100_000, -475_000):
        assert np.array_equal(M.bits(X.channelise(raw, "cs16", 2_000_000, fo)), M.bits(M.channelise(raw, "cs16", 2_000_000, fo)))
    # ... and with one it is not, but has the same magnitudes to within the rounding of two complex products
    a, b = X.channelise(raw, "cs16", 2_000_000, 104_100), M.channelise(raw, "cs16", 2_000_000, 100_000)
    assert not np.array_equal(M.bits(a), M.bits(b))
    assert np.allclose(np.abs(a.astype(np.complex128)), np.abs(b.astype(np.complex128)), rtol=1e-6, atol=1e-3)


@pytest.mark.parametrize("row", range(len(X.ROWS)), ids=X.IDS)
def test_rows_decode_with_the_flag_and_not_without(built, oracle, row):
    """The model's planes through the oracle's demodulator: every channel yields a CRC-clean frame equal to what synth sent.  The
    same recording channelised the present way -- the table of the off-grid Fo itself, which jumps every L samples -- yields no
    frame on the channels with Fd = +-12500."""
    rate, fmt, fos = X.ROWS[row]
    want = X.expected(oracle, row)
    sent = X.sent_frames(want["spec"])
    for c, fo in enumerate(fos):
        got = [f[1:-3] for f in want["frames"][c]]
        assert len(got) >= 1 and all(s in got for s in sent[c]), (rate, c, fo)
        if abs(X.split(fo)[1]) == 12_500:
            jump = M.demod_blocks(oracle, M.channelise(want["raw"], fmt, rate, fo), S.FC + fo, chn=c)
            assert X.frames_of(oracle, jump) == [], (rate, c, fo)
