"""VDL2GPU_F_SOFT_RS without a GPU: the header, the ctypes mirror of vdl2gpu_soft_t, the exports and the calls' refusals."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "vdl2gpu.h")


def test_header_declares_soft_rs():
    text = open(HDR).read()
    assert re.search(r"#define VDL2GPU_F_SOFT_RS 256u", text)
    assert re.search(r"#define VDL2GPU_HAVE_SOFT_RS 1", text)
    assert "} vdl2gpu_soft_t;" in text
    assert re.search(r"int vdl2gpu_poll_soft\(vdl2gpu_t \*h, vdl2gpu_burst_t \*out, vdl2gpu_level_t \*lv, vdl2gpu_soft_t \*soft, int max\);",
                     text)
    assert re.search(r"int vdl2gpu_poll_soft_ready\(vdl2gpu_t \*h, vdl2gpu_burst_t \*out, vdl2gpu_level_t \*lv, vdl2gpu_soft_t \*soft, "
                     r"int max\);", text)
    assert re.search(r"int vdl2gpu_decode_blocks_soft\(vdl2gpu_t \*h, const vdl2gpu_burst_t \*blocks, const vdl2gpu_soft_t \*soft, "
                     r"int n,\s+vdl2gpu_frame_t \*frames, int max_frames, int \*dropped\);", text)
    assert re.search(r"#define VDL2GPU_ABI_VERSION 6\b", text)


def test_soft_layout_matches_the_compiler(tmp_path):
    from vdlm2dec_amd import lib
    assert lib.F_SOFT_RS == 256
    fields = [f for f, _ in lib.SoftT._fields_]
    src = tmp_path / "sv.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vdl2gpu.h"\nint main(void){printf("%zu %zu", sizeof(vdl2gpu_soft_t), _Alignof(vdl2gpu_soft_t));'
                   + "".join(f'printf(" %zu", offsetof(vdl2gpu_soft_t, {f}));' for f in fields) + 'printf("\\n");return 0;}\n')
    exe = tmp_path / "sv"
    subprocess.check_call(["cc", "-std=c11", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got[0] == C.sizeof(lib.SoftT) == 2048
    assert got[1] == C.alignment(lib.SoftT) == 1
    assert got[2:] == [getattr(lib.SoftT, f).offset for f in fields] == [0, 2040]


def test_soft_symbols_are_exported(built):
    from vdlm2dec_amd import lib
    for name in ("vdl2gpu_poll_soft", "vdl2gpu_poll_soft_ready", "vdl2gpu_decode_blocks_soft"):
        assert name in lib.EXPORTS
        for so in ("libvdl2gpu.so", "libvdl2gpu_test.so"):
            out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "vdlm2dec_amd", so)], text=True)
            assert name in {ln.split()[-1] for ln in out.splitlines() if ln.strip()}, (so, name)


def test_abi_version_is_still_6(built):
    from vdlm2dec_amd import lib
    assert lib.load().vdl2gpu_abi_version() == 6


def test_soft_calls_without_gpu():
    from vdlm2dec_amd import lib
    L = lib.load()
    try:
        import torch
        if torch.cuda.is_available():
            pytest.skip("a GPU is present: tests/test_gpu_soft.py covers the handle")
    except ImportError:
        pass
    chan = (lib.ChanT * 1)(lib.ChanT(0, 136975000, 100000))
    cfg = lib.ConfigT()
    cfg.struct_size = C.sizeof(lib.ConfigT)
    cfg.sdrinrate, cfg.fmt, cfg.nbch, cfg.nstreams, cfg.chan, cfg.max_push = 2_000_000, 0, 1, 1, chan, 1 << 20
    cfg.flags = lib.F_SOFT_RS
    h = C.c_void_p()
    assert L.vdl2gpu_create(C.byref(cfg), C.byref(h)) == -5     # VDL2GPU_ENODEV, like any other handle
    assert L.vdl2gpu_poll_soft(None, None, None, None, 0) == -1
    assert L.vdl2gpu_poll_soft_ready(None, None, None, None, 0) == -1
    assert L.vdl2gpu_decode_blocks_soft(None, None, None, 0, None, 0, None) == -1
