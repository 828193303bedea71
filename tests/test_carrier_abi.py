"""VDL2GPU_F_CARRIER without a GPU: the header, the ctypes mirror of vdl2gpu_carrier_t, the host helper vdl2gpu_carrier_from_sums
against the header's formulas in numpy float64, the handle's refusal without a device, and the CPU statement of the physics check:
the model (tests/carrier_ref.py, pinned by the oracle's bytes) on the scenario tests/test_gpu_carrier.py runs on the GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import carrier_ref as CR
import scenarios as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "vdl2gpu.h")

# The physics scenario (carrier_ref.physics_spec()) through the model alone, as measured by test_physics_on_the_cpu below:
# 22 bursts, 21 of them with rms_rad < 0.1; among those the worst |freq_hz - cfo| is 2.026 Hz.  B is twice that.
MODEL_WORST_HZ = 2.026
B_HZ = 2 * MODEL_WORST_HZ


def test_header_declares_the_carrier_record():
    text = open(HDR).read()
    assert re.search(r"#define VDL2GPU_F_CARRIER 1024u", text)
    assert re.search(r"#define VDL2GPU_HAVE_CARRIER 1", text)
    assert "} vdl2gpu_carrier_t;" in text
    args = r"\(vdl2gpu_t \*h, vdl2gpu_burst_t \*out, vdl2gpu_level_t \*lv, vdl2gpu_soft_t \*soft, vdl2gpu_carrier_t \*car, int max\);"
    assert re.search(r"int vdl2gpu_poll_carrier" + args, text)
    assert re.search(r"int vdl2gpu_poll_carrier_ready" + args, text)
    assert re.search(r"int vdl2gpu_carrier_from_sums\(float df, int Fr, int nsym, int sum_e, unsigned sum_e2, vdl2gpu_carrier_t \*out\);", text)
    assert re.search(r"#define VDL2GPU_ABI_VERSION 6\b", text)
    # what the comment owes the reader: where the pi/8 comes from, that df / ppm stay the reference's, the sign, the caveat
    body = text[text.index("VDL2GPU_F_CARRIER; announced by"):text.index("#define VDL2GPU_F_CARRIER 1024u")]
    for phrase in ("sync-word table", "slope of pi/8", "stay that", "ABOVE the channel centre", "decision-directed", "not to be trusted",
                   "32 bytes per record slot"):
        assert phrase in body, phrase


def test_library_exports_the_calls(built):
    from vdlm2dec_amd import lib
    L = lib.load()
    for s in ("vdl2gpu_poll_carrier", "vdl2gpu_poll_carrier_ready", "vdl2gpu_carrier_from_sums"):
        assert s in lib.EXPORTS and hasattr(L, s), s      # (csrc/vdl2gpu.map exports vdl2gpu_*: no line of its own is needed there)


def test_carrier_layout_matches_the_compiler(tmp_path):
    from vdlm2dec_amd import lib
    assert lib.F_CARRIER == 1024
    fields = [f for f, _ in lib.CarrierT._fields_]
    assert fields == ["nsym", "sum_e", "sum_e2", "reserved", "dphi", "freq_hz", "ppm", "rms_rad"]
    src = tmp_path / "car.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vdl2gpu.h"\nint main(void){printf("%zu %zu", sizeof(vdl2gpu_carrier_t), _Alignof(vdl2gpu_carrier_t));'
                   + "".join(f'printf(" %zu", offsetof(vdl2gpu_carrier_t, {f}));' for f in fields) + 'printf("\\n");return 0;}\n')
    exe = tmp_path / "car"
    subprocess.check_call(["cc", "-std=c11", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got[0] == C.sizeof(lib.CarrierT) == 32
    assert got[1] == C.alignment(lib.CarrierT) == 4
    assert got[2:] == [getattr(lib.CarrierT, f).offset for f in fields] == [0, 4, 8, 12, 16, 20, 24, 28]


def _ulps(a, b):
    """distance of two float32 in units in the last place (same sign or zero)"""
    ia, ib = (int(np.float32(v).view(np.int32)) for v in (a, b))
    return abs(ia - ib)


def test_carrier_from_sums_equals_the_formulas(built):
    from vdlm2dec_amd import lib
    L = lib.load()
    rng = np.random.default_rng(1024)
    cases = [(0.0, 136_975_000, 1, 0, 0), (0.0, 136_975_000, 1, -16, 256), (0.0, 136_975_000, 1, 15, 225),
             (-0.3926991, 118_000_000, 5309, 0, 5309), (0.01, -136_975_000, 100, -50, 900), (0.02, 1, 7, 3, 3)]
    for _ in range(300):
        n = int(rng.integers(1, 5310))       # the longest burst has 5309 symbols behind the header
        e = rng.integers(-16, 16, n)
        cases.append((float(np.float32(rng.uniform(-0.6, 0.6))), int(rng.integers(108_000_000, 137_000_000)), n, int(e.sum()), int((e * e).sum())))
    for df, fr, n, se, se2 in cases:
        c = lib.CarrierT(7, 7, 7, 7, 7.0, 7.0, 7.0, 7.0)
        assert L.vdl2gpu_carrier_from_sums(df, fr, n, se, se2, C.byref(c)) == 0
        assert (c.nsym, c.sum_e, c.sum_e2, c.reserved) == (n, se, se2, 0)
        want = CR.derived(df, fr, n, se, se2)
        for name, w in zip(("dphi", "freq_hz", "ppm", "rms_rad"), want):
            assert _ulps(getattr(c, name), w) <= 1, (name, getattr(c, name), float(w), (df, fr, n, se, se2))
    # a constant e has no spread, whatever the rounding of sum_e2 / nsym - m * m makes of it
    c = lib.CarrierT()
    assert L.vdl2gpu_carrier_from_sums(0.0, 136_975_000, 3, -21, 147, C.byref(c)) == 0 and c.rms_rad == 0.0


def test_carrier_from_sums_refuses(built):
    from vdlm2dec_amd import lib
    L = lib.load()
    c = lib.CarrierT(7, 7, 7, 7, 7.0, 7.0, 7.0, 7.0)
    for df, fr, n in ((0.0, 136_975_000, 0), (0.0, 136_975_000, -3), (0.0, 0, 10)):
        assert L.vdl2gpu_carrier_from_sums(df, fr, n, 0, 0, C.byref(c)) == -1      # VDL2GPU_EINVAL
        assert (c.nsym, c.freq_hz) == (7, 7.0)                                         # ... and *out untouched
    assert L.vdl2gpu_carrier_from_sums(0.0, 136_975_000, 10, 0, 0, None) == -1


def test_python_mirror(built):
    from vdlm2dec_amd import demod
    c = demod.carrier_from_sums(0.01, 136_975_000, 100, -50, 900)
    want = CR.derived(0.01, 136_975_000, 100, -50, 900)
    assert (c.nsym, c.sum_e, c.sum_e2) == (100, -50, 900)
    assert all(_ulps(g, w) <= 1 for g, w in zip((c.dphi, c.freq_hz, c.ppm, c.rms_rad), want))
    assert demod.Burst.__dataclass_fields__["carrier"].default is None
    with pytest.raises(Exception):
        demod.carrier_from_sums(0.0, 0, 10, 0, 0)


def test_carrier_handle_without_gpu_is_enodev(built):
    from vdlm2dec_amd import lib
    L = lib.load()
    assert L.vdl2gpu_poll_carrier(None, None, None, None, None, 0) == -1
    assert L.vdl2gpu_poll_carrier_ready(None, None, None, None, None, 0) == -1
    try:
        import torch
        if torch.cuda.is_available():
            pytest.skip("a GPU is present: tests/test_gpu_carrier.py covers the handle")
    except ImportError:
        pass
    chan = (lib.ChanT * 1)(lib.ChanT(0, 136975000, 100000))
    cfg = lib.ConfigT()
    cfg.struct_size = C.sizeof(lib.ConfigT)
    cfg.sdrinrate, cfg.fmt, cfg.nbch, cfg.nstreams, cfg.chan, cfg.max_push = 2_000_000, 0, 1, 1, chan, 1 << 20
    cfg.flags = lib.F_CARRIER
    h = C.c_void_p()
    assert L.vdl2gpu_create(C.byref(cfg), C.byref(h)) == -5     # VDL2GPU_ENODEV, like any other handle


_phys = {}


def physics_model(cfo=None):
    """[(chn, trig_dec, transmitted cfo, model freq_hz, model rms_rad, one-shot Hz)] of the physics scenario, through the model alone
    (once per process and cfo); tests/test_gpu_carrier.py shares it"""
    if cfo not in _phys:
        from vdlm2dec_amd import synth
        spec = CR.physics_spec(cfo)
        raw = synth.synth_stream(spec, "cs16")
        rows = []
        for (_, c, t), (b, (n, se, se2)) in sorted(CR.stream_sums(raw, "cs16", CR.RATE, spec.fo, S.FC).items()):
            d = CR.derived(b.df, S.FC + spec.fo[c], n, se, se2)
            rows.append((c, t, CR.truth_cfo(spec, c, t), float(d[1]), float(d[3]), 10500.0 * float(b.df) / (2 * np.pi) + 656.25))
        _phys[cfo] = (spec, raw, rows)
    return _phys[cfo]


def test_physics_on_the_cpu(built, oracle):
    """The burst-long estimate against the transmitted offsets, through the model alone: cfo uniform in +-400 Hz, noise 1.7.
    Measured: 22 bursts, 21 with rms_rad < 0.1, worst of those 2.026 Hz (B = 4.052 Hz is twice that), rms error 0.76 Hz against
    9.0 Hz of the one-shot estimate (10500 df / 2 pi + 656.25): a ratio of 11.8."""
    spec, _, rows = physics_model()
    assert len(rows) == len(spec.bursts) >= 15
    good = [r for r in rows if r[4] < 0.1]
    assert len(rows) - len(good) <= 0.1 * len(rows)
    err = np.array([r[3] - r[2] for r in rows])
    one = np.array([r[5] - r[2] for r in rows])
    worst = max(abs(r[3] - r[2]) for r in good)
    print(f"\nphysics, model: {len(rows)} bursts, {len(good)} with rms_rad < 0.1, worst of those {worst:.3f} Hz, rms {np.sqrt((err ** 2).mean()):.3f} Hz, "
          f"one-shot rms {np.sqrt((one ** 2).mean()):.3f} Hz, one-shot mean {one.mean():+.2f} Hz")
    assert abs(worst - MODEL_WORST_HZ) < 0.002          # B_HZ stands on this number: a changed scenario must restate it
    assert np.sqrt((err ** 2).mean()) <= np.sqrt((one ** 2).mean()) / 5
    assert abs(one.mean()) < 5.0                        # the 656.25 Hz is the whole bias of the one-shot estimate
