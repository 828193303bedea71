"""Pin the oracle: the CPU restatement against the real reference built from its own sources
(oracle/_ref, only where /root/reference exists).  Skipped on the GPU box; tests/test_golden.py
carries the same evidence there as committed vectors."""
import os

import numpy as np
import pytest

import scenarios as S
from vdlm2dec_amd import synth


def _compare(O, spec, fmt, tmp_path, quirk=0, sdrclk=0):
    raw = synth.synth_stream(spec, fmt)
    p = str(tmp_path / "iq.raw")
    raw.tofile(p)
    total_blocks = 0
    for c, fo in enumerate(spec.fo):
        rb, rf, taps = O.run_ref(p, fmt, spec.rate, fo, S.FC + fo, str(tmp_path / "o.txt"), quirk, str(tmp_path / "t.bin"),
                                 sdrclk=sdrclk)
        ch = O.OracleChannel(spec.rate, fo, S.FC + fo, chn=c, tap_phase=True, sdrclk=sdrclk)
        ch.feed(raw, fmt + ("_quirk" if quirk else ""))
        ob = ch.blocks()
        assert len(ob) == len(rb)
        fr = []
        for a, b in zip(rb, ob):
            assert (a["nbrow"], a["nlbyte"], a["data"]) == (b.nbrow, b.nlbyte, b.data)
            assert a["df_bits"] == int(np.float32(b.df).view(np.uint32))
            fr += O.frames_of_block(b.nbrow, b.nlbyte, b.data)
        assert [f["frame"] for f in rf] == fr
        at = taps[taps["t"] == 1]
        assert np.array_equal(at["c"].view(np.uint32), ch.phases().view(np.uint32))
        # header soft bits handed to viterbi_add, in order
        total_blocks += len(ob)
        # trigger timing decisions: every roundf() argument at a trigger equals `of`
        rr = taps[taps["t"] == 2]
        tr = ch.triggers()
        ofs = {np.float32(t["of"]).view(np.uint32).item() for t in tr}
        assert ofs <= set(rr["a"].view(np.uint32).tolist())
        ch.close()
    return total_blocks


@pytest.fixture
def O(oracle, have_ref):
    if not have_ref:
        pytest.skip("oracle/_ref not built (no /root/reference on this machine)")
    return oracle


def test_regimes_cu8(O, tmp_path):
    assert _compare(O, S.regimes(seed=101), "cu8", tmp_path) >= 12


def test_regimes_cu8_quirk(O, tmp_path):
    assert _compare(O, S.regimes(seed=102, infos=(5, 40, 70, 250)), "cu8", tmp_path, quirk=1) >= 3


def test_eight_channels_cs16(O, tmp_path):
    assert _compare(O, S.eight_channels(seed=103), "cs16", tmp_path) >= 12


def test_back_to_back_stale_ring(O, tmp_path):
    assert _compare(O, S.back_to_back(), "cu8", tmp_path) >= 3


def test_odd_headers(O, tmp_path):
    _compare(O, S.odd_headers(), "cs16", tmp_path)


def test_corrupted_rows_frames(O, tmp_path):
    assert _compare(O, S.corrupted(), "cu8", tmp_path) == 5


def test_ten_ms_cs16(O, tmp_path):
    assert _compare(O, S.single_short(10_000_000, 2_400_000, seed=104, info_len=33, blocks=6), "cs16", tmp_path) == 1


def test_airspy_real_f32(O, tmp_path):
    assert _compare(O, S.single_short(6_000_000, 1_200_000, seed=105, info_len=14, blocks=5), "f32", tmp_path) == 1


def test_weak_noisy(O, tmp_path):
    # low SNR: sync decisions near threshold, header Viterbi actually corrects, false triggers possible
    spec = S.regimes(seed=106, infos=(20, 50, 90, 30, 10, 77), noise=6.0)
    _compare(O, spec, "cu8", tmp_path)


def test_rate_2025k_cs16_sdrclk_truncates(O, tmp_path):
    """2.025 MS/s: SDRCLK = 2025000 / 4000 = 506.25 truncates to 506, and 4 * 506 is no whole number of L = 81 inputs."""
    assert _compare(O, S.regimes(rate=2_025_000, seed=121, infos=(3, 28, 60, 200, 497)), "cs16", tmp_path) >= 4


def test_rate_2400k_cu8(O, tmp_path):
    assert _compare(O, S.regimes(rate=2_400_000, seed=122, infos=(2, 31, 66, 250)), "cu8", tmp_path) >= 3


def test_rate_100k_cs16_one_channel_at_the_centre(O, tmp_path):
    """the smallest accepted rate: L = 4 LO values, SDRCLK 25, windows of at most 2 inputs"""
    assert _compare(O, S.single_short(100_000, 0, seed=123, info_len=20, blocks=3), "cs16", tmp_path) == 1


@pytest.mark.parametrize("sdrclk", [400, 510])
def test_custom_sdrclk_at_2m(O, tmp_path, sdrclk):
    """SDRCLK given apart from the rate (the global a caller of the decoder may set): a decimated rate of 105 / 82.35 kS/s, so
    the bursts mostly fail; the phases, triggers and whatever is handed over must still be the reference's."""
    _compare(O, S.regimes(seed=124 + sdrclk, infos=(5, 40, 90)), "cs16", tmp_path, sdrclk=sdrclk)


def test_rs_decoder_against_reference_rs(O):
    """vo_rs_decode vs the reference's rs() (rs.c:81) compiled as oracle/_ref/librefrs.so,
    on random codewords with errors + erasures, correctable and not."""
    import ctypes as C
    ref = C.CDLL(os.path.join(O.REF_DIR, "librefrs.so"))
    ref.rs.restype = C.c_int
    ref.rs.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_int]
    L = O.lib()
    rng = np.random.default_rng(7)
    for it in range(4000):
        row = rng.integers(0, 256, 249, dtype=np.uint8)
        cw = np.concatenate([row, np.array(synth.rs_parity(row.tolist()), dtype=np.uint8)])
        nera = int(rng.choice([0, 0, 2, 4]))
        eras = [253, 254] if nera == 2 else ([251, 252, 253, 254] if nera == 4 else [])
        for e in eras:
            cw[e] = 0
        nerr = int(rng.integers(0, 6))
        for pos in rng.choice(251, size=nerr, replace=False):
            cw[pos] ^= int(rng.integers(1, 256))
        a, b = cw.copy(), cw.copy()
        ea = (C.c_int * 6)(*(eras + [0] * (6 - len(eras))))
        eb = (C.c_int * 6)(*(eras + [0] * (6 - len(eras))))
        ra = ref.rs(a.ctypes.data_as(C.c_void_p), ea, nera)
        rb = L.vo_rs_decode(b.ctypes.data_as(C.c_void_p), eb, nera)
        assert ra == rb, (it, nerr, nera)
        assert np.array_equal(a, b), (it, nerr, nera)
        if ra > 0:
            assert list(ea)[:ra] == list(eb)[:rb]


def _ref_outputs(O, raw, fmt, spec, tmp_path, ofast):
    p = str(tmp_path / "iq.raw")
    raw.tofile(p)
    out = []
    for fo in spec.fo:
        rb, rf, _ = O.run_ref(p, fmt, spec.rate, fo, S.FC + fo, str(tmp_path / ("o%d.txt" % ofast)), 0, "", ofast=ofast)
        out.append(([(b["nbrow"], b["nlbyte"], b["df_bits"], b["data"]) for b in rb], [f["frame"] for f in rf]))
    return out


@pytest.mark.parametrize("case", ["regimes_cu8", "eight_cs16", "air_f32", "cs16_10ms"])
def test_reference_built_with_its_own_flags_hands_over_the_same_blocks(O, tmp_path, case):
    """the reference ships -Ofast -march=native (CMakeLists.txt:4); the oracle and the golden
    vectors are pinned to an -O2 build of the same sources.  Fast-math moves the float results by a few ulp (the
    carrier estimate df below), so parity between the two builds is defined where north_star defines it: at the
    decision level.  Both builds must hand over identical msgblk_t decisions (nbrow, nlbyte, every data byte)
    and identical CRC-clean frames; df may differ by a few units in the last place."""
    if not os.path.exists(os.path.join(O.REF_DIR, "ref_rtl_ofast")):
        pytest.skip("oracle/_ref/ref_rtl_ofast not built")
    spec, fmt = {
        "regimes_cu8": (S.regimes(seed=111), "cu8"),
        "eight_cs16": (S.eight_channels(seed=112), "cs16"),
        "air_f32": (S.single_short(5_000_000, 375_000, seed=113, info_len=30, blocks=6), "f32"),
        "cs16_10ms": (S.single_short(10_000_000, -1_250_000, seed=114, info_len=40, blocks=8), "cs16"),
    }[case]
    raw = synth.synth_stream(spec, fmt)
    a = _ref_outputs(O, raw, fmt, spec, tmp_path, False)
    b = _ref_outputs(O, raw, fmt, spec, tmp_path, True)
    assert sum(len(x[0]) for x in a) >= 1
    for (ba, fa), (bb, fb) in zip(a, b):
        assert [(x[0], x[1], x[3]) for x in ba] == [(x[0], x[1], x[3]) for x in bb]      # sliced-bit level
        assert fa == fb                                                                  # CRC-pass level
        for x, y in zip(ba, bb):
            assert abs(int(x[2]) - int(y[2])) <= 16                                      # df: same sign/exponent, a few ulp


def _soak_scenario(seed):
    """the soak's randomised scenarios (scripts/soak.py), small: rate, format, channel count, burst density, lengths"""
    rng = np.random.default_rng(9000 + seed)
    rate = int(rng.choice([2_000_000, 2_000_000, 5_000_000, 10_000_000]))
    fmt = "f32" if (rate == 5_000_000 and seed % 3 == 0) else str(rng.choice(["cu8", "cs16"]))
    nch = int(rng.integers(1, 4))
    pool = S.FO8_AIR_5MS if fmt == "f32" else (S.FO8 if rate == 2_000_000 else S.FO8_10MS)
    fos = [int(x) for x in rng.choice(pool, size=nch, replace=False)]
    ns = int(rng.integers(3, 8)) * 200_000 * (rate // 2_000_000 if rate > 2_000_000 else 1)
    dens = float(rng.choice([8.0, 20.0, 40.0, 80.0])) * rate / 2_000_000 / (rate // 2_000_000 if rate > 2_000_000 else 1)
    spec = synth.random_scenario(rate, fos, ns, seed=9000 + seed, bursts_per_s=dens, info_max=int(rng.choice([30, 120, 400])))
    if seed % 5 == 4:
        spec.noise = 5.0        # low SNR: decisions near their thresholds
    return spec, fmt


def test_ofast_build_hands_over_the_same_blocks_on_the_soak_scenarios(O, tmp_path):
    """The same decision-level comparison (sliced bits and CRC-clean frames equal, df within a few ulp) over 54
    randomised scenarios of the soak's kind -- 2 / 5 / 10 MS/s, cu8 / cs16 / real f32, 1-3 channels, 8-80 bursts
    a second, payloads up to 400 bytes, every fifth at low SNR -- instead of four fixed recordings."""
    if not os.path.exists(os.path.join(O.REF_DIR, "ref_rtl_ofast")):
        pytest.skip("oracle/_ref/ref_rtl_ofast not built")
    nblocks = nscen = 0
    for seed in range(54):
        spec, fmt = _soak_scenario(seed)
        raw = synth.synth_stream(spec, fmt)
        a = _ref_outputs(O, raw, fmt, spec, tmp_path, False)
        b = _ref_outputs(O, raw, fmt, spec, tmp_path, True)
        for (ba, fa), (bb, fb) in zip(a, b):
            assert [(x[0], x[1], x[3]) for x in ba] == [(x[0], x[1], x[3]) for x in bb], seed
            assert fa == fb, seed
            for x, y in zip(ba, bb):
                assert abs(int(x[2]) - int(y[2])) <= 16, seed
            nblocks += len(ba)
        nscen += 1
    assert nscen >= 50 and nblocks >= 300
