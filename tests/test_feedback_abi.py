"""VDL2GPU_F_FEEDBACK without a GPU: the header, the ctypes mirror of vdl2gpu_fb_t against the compiler, the declarations against the
export map and the ctypes mirror, and the Python surface."""
import ctypes as C
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "vdl2gpu.h")
NEW = ("vdl2gpu_poll_feedback", "vdl2gpu_poll_feedback_ready", "vdl2gpu_decode_blocks_feedback")


def test_header_declares_the_rows():
    text = open(HDR).read()
    assert re.search(r"#define VDL2GPU_F_FEEDBACK 4096u", text)
    assert re.search(r"#define VDL2GPU_HAVE_FEEDBACK 1\b", text)
    assert re.search(r"#define VDL2GPU_ABI_VERSION 6\b", text)
    assert re.search(r"#define VDL2GPU_ROW_FEEDBACK 6\b", text)
    assert "} vdl2gpu_fb_t;" in text
    args = (r"\(vdl2gpu_t \*h, vdl2gpu_burst_t \*out, vdl2gpu_level_t \*lv, vdl2gpu_soft_t \*soft, vdl2gpu_carrier_t \*car, "
            r"vdl2gpu_blockrep_t \*rep,\s*vdl2gpu_fb_t \*fb, int max\);")
    assert re.search(r"int vdl2gpu_poll_feedback" + args, text)
    assert re.search(r"int vdl2gpu_poll_feedback_ready" + args, text)
    assert re.search(r"int vdl2gpu_decode_blocks_feedback\(vdl2gpu_t \*h, const vdl2gpu_burst_t \*blocks, const vdl2gpu_soft_t \*soft, "
                     r"const vdl2gpu_fb_t \*fb, int n,\s*vdl2gpu_frame_t \*frames, int max_frames, int \*dropped, vdl2gpu_blockrep_t \*rep\);", text)
    # what the comment owes the reader: the rule to the bit, and what stays
    body = text[text.index("VDL2GPU_F_FEEDBACK; announced by"):text.index("#define VDL2GPU_F_FEEDBACK 4096u")]
    for phrase in ("e_k  = (idx_k & 31) - 16", "mbar = floor((2 S + n) / (2 n))", "c   = 3 r_{k-1} + 2 r_{k-2} + r_{k-3}",
                   "o_k = (idx_k - mbar + floor((c + 2) / 4)) mod 256", "r_k = ((idx_k - 16 - 32 (o_k >> 5) - mbar + 128) mod 256) - 128",
                   "towards minus infinity", "whatever kernel, path or repair round", "however the stream", "stay the reference's",
                   "all six syndromes zero", "does not need VDL2GPU_F_FRAMES", "2048 bytes per record slot"):
        assert phrase in body, phrase


def test_layout_matches_the_compiler(tmp_path):
    from vdlm2dec_amd import lib
    assert lib.F_FEEDBACK == 4096 and lib.ROW_FEEDBACK == 6
    assert [f for f, _ in lib.FbT._fields_] == ["data", "reserved"]
    src = tmp_path / "fb.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vdl2gpu.h"\nint main(void){printf("%zu %zu %zu %zu %zu %u %d %d\\n", '
                   "sizeof(vdl2gpu_fb_t), _Alignof(vdl2gpu_fb_t), offsetof(vdl2gpu_fb_t, data), offsetof(vdl2gpu_fb_t, reserved), "
                   "sizeof(vdl2gpu_soft_t), VDL2GPU_F_FEEDBACK, VDL2GPU_HAVE_FEEDBACK, VDL2GPU_ROW_FEEDBACK);return 0;}\n")
    exe = tmp_path / "fb"
    subprocess.check_call(["cc", "-std=c11", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [2048, 1, 0, 2040, 2048, 4096, 1, 6]
    assert C.sizeof(lib.FbT) == 2048 and C.alignment(lib.FbT) == 1
    assert (lib.FbT.data.offset, lib.FbT.reserved.offset) == (0, 2040)


def _declared():
    """name -> argument list (text) of every function include/vdl2gpu.h declares"""
    text = re.sub(r"/\*.*?\*/", " ", open(HDR).read(), flags=re.S)
    return {m.group(1): " ".join(m.group(2).split()) for m in re.finditer(r"\b(vdl2gpu_\w+|reversebits)\s*\(([^;{}]*)\)\s*;", text)}


def test_declarations_equal_the_exports_and_the_ctypes_mirror(built):
    from vdlm2dec_amd import lib
    decl = _declared()
    assert set(NEW) <= set(decl)
    assert set(decl) == set(lib.EXPORTS)                 # the header declares what the mirror lists, no more and no less
    # the export map lets through exactly that family
    m = open(os.path.join(ROOT, "vdlm2dec_amd", "csrc", "vdl2gpu.map")).read()
    assert "vdl2gpu_*;" in m and "reversebits;" in m and re.search(r"local:\s*\*;", m)
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "vdlm2dec_amd", "libvdl2gpu.so")], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split()[-2] in "TW"}
    assert {s for s in exported if s.startswith("vdl2gpu_") or s == "reversebits"} == set(decl)
    # argument counts and the new types of the ctypes mirror
    L = lib.load()
    for name in NEW:
        fn = getattr(L, name)
        assert len(fn.argtypes) == decl[name].count(",") + 1 and fn.restype is C.c_int, name
    assert L.vdl2gpu_poll_feedback.argtypes[6] is C.POINTER(lib.FbT) and L.vdl2gpu_poll_feedback_ready.argtypes[6] is C.POINTER(lib.FbT)
    assert L.vdl2gpu_decode_blocks_feedback.argtypes[3] is C.POINTER(lib.FbT)
    assert L.vdl2gpu_abi_version() == 6
    # a null handle is refused like everywhere else
    assert L.vdl2gpu_poll_feedback(None, None, None, None, None, None, None, 0) == -1
    assert L.vdl2gpu_poll_feedback_ready(None, None, None, None, None, None, None, 0) == -1
    assert L.vdl2gpu_decode_blocks_feedback(None, None, None, None, 0, None, 0, None, None) == -1


def test_python_surface():
    import numpy as np
    from vdlm2dec_amd import demod
    assert demod.Burst.__dataclass_fields__["fb"].default is None
    b = demod.Burst(0, 0, 0, 1, 20, 0.0, 0.0, 0, 0, 0, 0, bytes(2040), fb=np.zeros((8, 255), np.uint8))
    assert b.key() == demod.Burst(0, 0, 0, 1, 20, 0.0, 0.0, 0, 0, 0, 0, bytes(2040)).key()      # not part of key()
    assert inspect.signature(demod.Receiver.__init__).parameters["feedback"].default is False
    assert hasattr(demod.Receiver, "poll_feedback_raw")
    p = inspect.signature(demod.Receiver.decode_blocks).parameters
    assert p["fb"].default is None and p["report"].default is False and p["soft"].default is None
    rx = demod.Receiver.__new__(demod.Receiver)      # no handle: an empty batch never reaches the library
    assert rx.decode_blocks([], fb=[]) == [] and rx.decode_blocks([], fb=[], report=True) == ([], [])
