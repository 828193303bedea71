"""VDL2GPU_F_EXACT_FO in the C ABI: the macros, the flag's validation before any device call, the two host helpers among the
exports and nothing else new in the dynamic symbol table."""
import ctypes as C
import os
import re
import subprocess

from vdlm2dec_amd import demod, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _macros():
    text = open(os.path.join(ROOT, "include", "vdl2gpu.h")).read()
    return dict(re.findall(r"^#define\s+(VDL2GPU_\w+)\s+(\d+)u?\b", text, re.M))


def test_macros(built):
    m = _macros()
    assert m["VDL2GPU_F_EXACT_FO"] == "512" and m["VDL2GPU_HAVE_EXACT_FO"] == "1" and m["VDL2GPU_ABI_VERSION"] == "6"
    assert lib.F_EXACT_FO == 512 and lib.load().vdl2gpu_abi_version() == 6
    others = [int(v) for k, v in m.items() if k.startswith("VDL2GPU_F_") and k != "VDL2GPU_F_EXACT_FO"]
    assert all(512 & v == 0 for v in others)


def _create(flags, fo=4_100, rate=2_000_000, fmt="cu8"):
    L = lib.load()
    chan = (lib.ChanT * 1)(lib.ChanT(0, 136_975_000 + fo, fo))
    cfg = lib.ConfigT()
    cfg.struct_size = C.sizeof(lib.ConfigT)
    cfg.sdrinrate, cfg.fmt, cfg.nbch, cfg.nstreams, cfg.chan, cfg.max_push, cfg.flags = rate, lib.FMT[fmt], 1, 1, chan, 32768, flags
    cfg.device = 1 << 20            # no such device: a configuration that passes validation ends in VDL2GPU_ENODEV, GPU or not
    h = C.c_void_p()
    rc = L.vdl2gpu_create(C.byref(cfg), C.byref(h))
    assert not h.value
    return L.vdl2gpu_strerror(rc).decode(), rc


def test_flag_is_validated_before_any_device_call(built):
    einval = _create(lib.F_RTL_QUIRK, rate=2_048_000)[1]            # (off the rate grid the quirk is refused: a known EINVAL)
    enodev = _create(0)[1]
    assert einval != enodev
    assert _create(lib.F_EXACT_FO)[1] == enodev                     # accepted: the next thing it wants is the device
    assert _create(lib.F_EXACT_FO, rate=2_048_000)[1] == enodev     # at a rate off the grid as well
    assert _create(lib.F_RTL_QUIRK)[1] == enodev
    assert _create(lib.F_EXACT_FO | lib.F_RTL_QUIRK)[1] == einval   # never together
    assert _create(lib.F_EXACT_FO, fo=999_999)[1] == enodev         # |Fo| < sdrinrate / 2
    assert _create(lib.F_EXACT_FO, fo=1_000_000)[1] == einval
    assert _create(lib.F_EXACT_FO, fo=-1_000_000)[1] == einval
    assert _create(0, fo=1_000_000)[1] == enodev                    # (without the flag nothing has changed)


def test_helpers_without_a_device(built):
    L = lib.load()
    assert "vdl2gpu_exact_fo_tables" in lib.EXPORTS and "vdl2gpu_exact_fo_index" in lib.EXPORTS
    assert L.vdl2gpu_exact_fo_tables(2_000_000, None, 0, None) == 977
    buf = (C.c_float * 8)()
    assert L.vdl2gpu_exact_fo_tables(2_000_000, buf, 4, None) < 0   # no room for T_hi
    assert L.vdl2gpu_exact_fo_tables(0, None, 0, None) < 0 and L.vdl2gpu_exact_fo_index(1, 2, 0, 1) < 0
    assert demod.exact_fo_index(0, 22, 2_000_000, 4_100) == 4_100 * 22
    assert demod.exact_fo_index(0, 22, 2_000_000, -1) == 4_000_000 - 22


def test_dynamic_symbols(built):
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib.LIB_PATH], text=True)
    syms = [ln.split()[-1] for ln in out.splitlines() if ln.strip()]
    assert "vdl2gpu_exact_fo_tables" in syms and "vdl2gpu_exact_fo_index" in syms
    assert all(s.startswith("vdl2gpu_") or s == "reversebits" for s in syms), [s for s in syms if not s.startswith("vdl2gpu_")]
