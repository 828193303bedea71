"""VDL2GPU_F_SYMCLK without a GPU: the header, the ctypes mirror of vdl2gpu_symclk_t against the compiler, the host arithmetic
vdl2gpu_symclk_from_sums against the header's formulas in numpy float64 (tests/symclk_ref.py) on crafted sums, and the transmitter's
symbol-clock offset, which at zero leaves every stream what it was."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import levels_ref as LR
import scenarios as S
import symclk_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "vdl2gpu.h")
FIELDS = ["sym_first_dec", "nsym", "nseg", "toa_sample", "tau0", "clock_ppm", "tau_rms", "reserved", "e"]


def test_header_declares_the_symclk_record():
    text = open(HDR).read()
    assert re.search(r"#define VDL2GPU_F_SYMCLK 32768u", text)
    assert re.search(r"#define VDL2GPU_HAVE_SYMCLK 1\b", text)
    assert re.search(r"#define VDL2GPU_SYMCLK_SEGS 22\b", text)
    assert "} vdl2gpu_symclk_t;" in text
    assert re.search(r"#define VDL2GPU_ABI_VERSION 6\b", text)
    args = (r"\(vdl2gpu_t \*h, vdl2gpu_burst_t \*out, vdl2gpu_level_t \*lv, vdl2gpu_soft_t \*soft, vdl2gpu_carrier_t \*car, "
            r"vdl2gpu_blockrep_t \*rep,\s*vdl2gpu_fb_t \*fb, vdl2gpu_symclk_t \*clk, int max\);")
    assert re.search(r"int vdl2gpu_poll_symclk" + args, text) and re.search(r"int vdl2gpu_poll_symclk_ready" + args, text)
    body = text[text.index("VDL2GPU_F_SYMCLK; announced by"):text.index("#define VDL2GPU_F_SYMCLK 32768u")]
    for phrase in ("Oerder-Meyr", "sub-phase 0", "xor butterfly", "((g0 + g1) + g2) + g3", "LATER than the grid", "FASTER than 10 500",
                   "centroid delay", "VDL2GPU_F_RTL_QUIRK", "never past end_dec", "744 bytes per record slot"):
        assert phrase in body, phrase


def test_layout_matches_the_compiler(tmp_path):
    from vdlm2dec_amd import lib
    assert lib.F_SYMCLK == 32768 and (lib.SYMCLK_SEG, lib.SYMCLK_SEGS) == (256, 22)
    assert [f for f, _ in lib.SymClkT._fields_] == FIELDS
    src = tmp_path / "clk.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vdl2gpu.h"\nint main(void){printf("%u %d %d %d %zu %zu", VDL2GPU_F_SYMCLK, '
                   'VDL2GPU_HAVE_SYMCLK, VDL2GPU_SYMCLK_SEG, VDL2GPU_SYMCLK_SEGS, sizeof(vdl2gpu_symclk_t), _Alignof(vdl2gpu_symclk_t));'
                   + "".join(f'printf(" %zu", offsetof(vdl2gpu_symclk_t, {f}));' for f in FIELDS) + 'printf("\\n");return 0;}\n')
    exe = tmp_path / "clk"
    subprocess.check_call(["cc", "-std=c11", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got[:4] == [32768, 1, 256, 22]
    # 40 bytes in front of e[22][8]: 40 + 704 = 744, a multiple of the alignment -- no padding
    assert got[4] == C.sizeof(lib.SymClkT) == 744 and got[5] == C.alignment(lib.SymClkT) == 8
    assert got[6:] == [getattr(lib.SymClkT, f).offset for f in FIELDS] == [0, 8, 12, 16, 24, 28, 32, 36, 40]
    # the segments cover the longest burst a header can announce, and the bound VDL2GPU_MAXROWS x VDL2GPU_ROWLEN bytes gives
    assert (R.nsym_of(8, 248) + 255) // 256 == 22 == ((25 + 8 * 8 * 255 + 2) // 3 + 255) // 256


def test_library_exports_the_calls(built):
    from vdlm2dec_amd import lib
    L = lib.load()
    for s in ("vdl2gpu_poll_symclk", "vdl2gpu_poll_symclk_ready", "vdl2gpu_symclk_from_sums"):
        assert s in lib.EXPORTS and hasattr(L, s), s
    assert L.vdl2gpu_poll_symclk(None, None, None, None, None, None, None, None, 0) == -1
    assert L.vdl2gpu_poll_symclk_ready(None, None, None, None, None, None, None, None, 0) == -1


def _rel(a, b):
    return abs(a - b) <= 1e-9 * abs(b)


# (nsym, tau0, slope per symbol): one segment; two; slopes of +-100 ppm (8e-4 a symbol), which over 5446 symbols carry tau past +4 and
# past -4 (the segments wrap); a start next to the wrap; the shortest second segment
CRAFTED = [(75, 1.25, 0.0), (256, -3.5, 0.0), (257, 0.7, 4e-4), (700, -2.2, -2.4e-4), (2547, 3.1, 4e-4), (5446, 2.0, 8e-4),
           (5446, -1.5, -8e-4), (5446, 3.9, 2.5e-4), (4000, -3.95, -1e-4), (513, 0.01, 0.0)]


@pytest.mark.parametrize("nsym,tau0,slope", CRAFTED)
def test_from_sums_equals_the_formulas(built, nsym, tau0, slope):
    from vdlm2dec_amd import demod
    mflt = LR.mflt_taps()
    e = R.cosine_sums(nsym, tau0, slope)
    first = 123_456_789
    for rate in (2_000_000, 10_000_000):
        k = demod.symclk_from_sums(first, nsym, e, rate)
        w_tau0, w_ppm, w_rms, w_toa, w_tau = R.derived(first, nsym, e, rate, mflt)
        nseg = (nsym + 255) // 256
        assert (k.sym_first_dec, k.nsym, k.nseg) == (first, nsym, nseg)
        assert np.array_equal(k.e[:nseg], e[:nseg]) and not k.e[nseg:].any()
        assert _rel(k.toa_sample, w_toa)
        assert k.tau0 == np.float32(w_tau0) or _rel(k.tau0, w_tau0)          # (the record's tau0 is a float; tau_s below are doubles)
        assert len(k.tau_s) == nseg and all(_rel(g, w) for g, w in zip(k.tau_s, w_tau))
        if nseg == 1:
            assert math.isnan(k.clock_ppm) and math.isnan(k.tau_rms) and math.isnan(w_ppm)
            assert k.tau0 == np.float32(k.tau_s[0])
        else:
            assert k.clock_ppm == np.float32(w_ppm) or _rel(k.clock_ppm, w_ppm)
            # ... and the crafted line comes back: the profile is an exact cosine, so the fit's residual is rounding alone
            assert abs(k.clock_ppm - (-slope / 8 * 1e6)) < 1e-2 and k.tau_rms < 1e-5
        assert abs(w_tau0 - tau0) < 1e-5
        # the unwrapped segments follow the line, however far past +-4 it goes
        c = [256 * s + (min(nsym, 256 * s + 256) - 256 * s - 1) / 2 for s in range(nseg)]
        assert np.allclose(k.tau_s, [tau0 + slope * x for x in c], atol=1e-5)
    if abs(slope) >= 8e-4:
        assert max(abs(t) for t in k.tau_s) > 4.0        # this case did wrap


def test_from_sums_maps_to_input_samples(built):
    """toa_sample: D is the centroid of the sub-phase-0 taps (8.25, not 8), the map the mean of the dump schedule"""
    from vdlm2dec_amd import demod
    D = R.centroid_delay(LR.mflt_taps())
    assert abs(D - 8.25) < 0.01
    k = demod.symclk_from_sums(84000, 100, R.cosine_sums(100, 0.0, 0.0), 2_000_000)
    assert abs(k.tau0) < 1e-6
    assert math.isclose(k.toa_sample, (84000 - D + 0.5) * 2_000_000 / 84000 - 0.5, rel_tol=1e-12, abs_tol=1e-4)


def test_from_sums_refuses(built):
    from vdlm2dec_amd import lib
    L = lib.load()
    e = (C.c_float * (22 * 8))(*([1.0] * 176))
    c = lib.SymClkT()
    c.nsym = 7
    for nsym, rate, ep, out in ((0, 2_000_000, e, C.byref(c)), (-1, 2_000_000, e, C.byref(c)), (256 * 22 + 1, 2_000_000, e, C.byref(c)),
                                (100, 0, e, C.byref(c)), (100, 2_000_000, None, C.byref(c)), (100, 2_000_000, e, None)):
        assert L.vdl2gpu_symclk_from_sums(0, nsym, ep, rate, out, None) == -1      # VDL2GPU_EINVAL
        assert c.nsym == 7                                                            # ... and *out untouched
    assert L.vdl2gpu_symclk_from_sums(0, 256 * 22, e, 2_000_000, C.byref(c), None) == 0 and c.nseg == 22
    # all-zero sums (a silent plane): tau_s = 0, nothing is NaN but what must be
    z = (C.c_float * 8)()
    assert L.vdl2gpu_symclk_from_sums(1000, 10, z, 2_000_000, C.byref(c), None) == 0
    assert c.tau0 == 0.0 and math.isnan(c.clock_ppm) and math.isnan(c.tau_rms) and c.reserved == 0


def test_python_mirror(built):
    from vdlm2dec_amd import demod
    assert demod.Burst.__dataclass_fields__["clock"].default is None
    assert [c[0] for c in demod._COLUMNS][-1] == "symclk"
    with pytest.raises(Exception):
        demod.symclk_from_sums(0, 0, np.zeros((1, 8), np.float32), 2_000_000)
    with pytest.raises(ValueError):
        demod.symclk_from_sums(0, 600, np.zeros((2, 8), np.float32), 2_000_000)       # three segments' worth of symbols


def test_sym_ppm_zero_is_the_stream_it_was(built):
    """Burst.sym_ppm = 0 (the default) leaves synth_stream bit-identical: the period is 1 / 10500 to the bit; an offset moves it"""
    from vdlm2dec_amd import synth
    spec = S.eight_channels()
    assert all(b.sym_ppm == 0.0 for b in spec.bursts)
    assert 1.0 / (synth.SYMRATE * (1.0 + 0.0 * 1e-6)) == 1.0 / synth.SYMRATE
    acc0 = np.zeros(200_000, np.complex128)
    acc1 = np.zeros(200_000, np.complex128)
    incr = synth.burst_increments(synth.burst_bits(spec.bursts[0].payload()))
    synth.modulate_into(acc0, incr, 2e6, 0.002, 30.0, 1e5)
    T = 1.0 / synth.SYMRATE      # the statement of the waveform as it stood before the field existed
    n = np.arange(200_000, dtype=np.float64)
    u = (n / 2e6 - 0.002) / T
    want = np.zeros(200_000, np.complex128)
    a = np.exp(1j * np.cumsum(incr) * (np.pi / 4.0))
    kc = np.floor(u).astype(np.int64)
    for j in range(-4, 6):
        k = kc + j
        ok = (k >= 0) & (k < len(a))
        want += np.where(ok, a[np.clip(k, 0, len(a) - 1)] * synth.rc_pulse(u - k), 0.0)
    want *= 30.0 * np.exp(2j * np.pi * 1e5 * (n / 2e6))
    lo = max(0, int(math.floor((0.002 - 4 * T) * 2e6)))
    hi = min(200_000, int(math.ceil((0.002 + (len(a) - 1 + 4) * T) * 2e6)) + 1)
    want[:lo] = 0
    want[hi:] = 0
    assert np.array_equal(acc0.view(np.float64), want.view(np.float64))
    synth.modulate_into(acc1, incr, 2e6, 0.002, 30.0, 1e5, sym_ppm=50.0)
    assert not np.array_equal(acc0, acc1)
    # ... and the golden recordings' digests (tests/test_golden*.py) hold every canned scenario to its bits as well
    b = synth.Burst(chan=0, t0=0.0, info=b"abc", sym_ppm=50.0)
    assert b.sym_ppm == 50.0 and synth.Burst(chan=0, t0=0.0, info=b"abc").sym_ppm == 0.0
