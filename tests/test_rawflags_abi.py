"""VDL2GPU_F_RAW_FLAGS without a GPU: the header's defines and rule, the ctypes mirror, what vdl2gpu_create and vdl2gpu_decode_blocks_ex
refuse before any device call, the Python surface, and the unchanged export list."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "vdl2gpu.h")


def test_header_defines_the_flag_and_states_the_rule():
    text = open(HDR).read()
    assert re.search(r"#define VDL2GPU_F_RAW_FLAGS 16384u", text)
    assert re.search(r"#define VDL2GPU_HAVE_RAW_FLAGS 1\b", text)
    assert re.search(r"#define VDL2GPU_BLK_RAW_FLAGS 4u", text)
    assert re.search(r"#define VDL2GPU_ABI_VERSION 6\b", text)
    body = text[text.index("VDL2GPU_F_RAW_FLAGS; announced by"):text.index("#define VDL2GPU_F_RAW_FLAGS 16384u")]
    for phrase in ("t == 6", "t == 5", "t7[q] == 1", "m1", "first q > flag_at with !F[q]", "flag_at itself is unchanged", "q >= m1 with F[q]",
                   "cand == too_short + bad_fcs + frames", "cand counts the true flags", "8q + 6",
                   "the same frames and the same report with and without this mode", "re-aligned at bit level", "VDL2GPU_F_ALL_FRAMES"):
        assert phrase in body, phrase
    allf = text[text.index("VDL2GPU_F_ALL_FRAMES; announced by"):text.index("#define VDL2GPU_F_ALL_FRAMES 8192u")]
    assert "VDL2GPU_F_RAW_FLAGS" in allf and "beside one with it" not in allf        # the all-frames rule points to the cure
    proto = text[text.index("#define VDL2GPU_BLK_ALL_FRAMES 1u") - 900:text.index("int vdl2gpu_decode_blocks_ex(")]
    assert "VDL2GPU_BLK_RAW_FLAGS" in proto and "0, 1 or 5" in proto


def test_values_match_the_compiler(tmp_path):
    from vdlm2dec_amd import lib
    assert lib.F_RAW_FLAGS == 16384 and lib.BLK_RAW_FLAGS == 4
    src = tmp_path / "rf.c"
    src.write_text('#include <stdio.h>\n#include "vdl2gpu.h"\n'
                   'int main(void){printf("%u %d %u %u %u %d %zu\\n", VDL2GPU_F_RAW_FLAGS, VDL2GPU_HAVE_RAW_FLAGS, VDL2GPU_BLK_RAW_FLAGS, '
                   "VDL2GPU_F_ALL_FRAMES, VDL2GPU_BLK_ALL_FRAMES, VDL2GPU_ABI_VERSION, sizeof(vdl2gpu_blockrep_t));return 0;}\n")
    exe = tmp_path / "rf"
    subprocess.check_call(["cc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [lib.F_RAW_FLAGS, 1, lib.BLK_RAW_FLAGS, lib.F_ALL_FRAMES, lib.BLK_ALL_FRAMES, 6, 48]


def test_create_refuses_the_flag_without_all_frames(built):
    from vdlm2dec_amd import lib
    L = lib.load()
    chan = (lib.ChanT * 1)(lib.ChanT(0, 136_975_000, -50_000))
    cfg = lib.ConfigT(struct_size=C.sizeof(lib.ConfigT), sdrinrate=2_000_000, fmt=0, nbch=1, nstreams=1, chan=chan,
                      max_push=32768, flags=lib.F_RAW_FLAGS | lib.F_FRAMES)
    h = C.c_void_p()
    assert L.vdl2gpu_create(C.byref(cfg), C.byref(h)) == -1
    assert "VDL2GPU_F_RAW_FLAGS needs VDL2GPU_F_ALL_FRAMES" in L.vdl2gpu_last_error(None).decode()
    # behind the existing refusals, whose messages and order stay
    cfg.flags = lib.F_RAW_FLAGS | lib.F_ALL_FRAMES
    assert L.vdl2gpu_create(C.byref(cfg), C.byref(h)) == -1
    assert "VDL2GPU_F_ALL_FRAMES needs VDL2GPU_F_FRAMES" in L.vdl2gpu_last_error(None).decode()
    cfg.flags = lib.F_RAW_FLAGS | lib.F_BLOCK_REPORT
    assert L.vdl2gpu_create(C.byref(cfg), C.byref(h)) == -1
    assert "VDL2GPU_F_BLOCK_REPORT needs VDL2GPU_F_FRAMES" in L.vdl2gpu_last_error(None).decode()


def test_modes_refused_before_any_device_call(built):
    from vdlm2dec_amd import lib
    L = lib.load()
    fake = C.c_void_p(1)        # never dereferenced: the mode word is looked at first
    blk, fr = (lib.BurstT * 1)(), (lib.FrameT * 1)()
    for mode in (lib.BLK_RAW_FLAGS, 6, 7, 0x80000004):
        assert L.vdl2gpu_decode_blocks_ex(fake, blk, None, None, 1, fr, 1, None, None, mode) == -1, mode
    assert L.vdl2gpu_decode_blocks_ex(None, blk, None, None, 1, fr, 1, None, None, lib.BLK_ALL_FRAMES | lib.BLK_RAW_FLAGS) == -1
    assert lib.BLK_ALL_FRAMES | lib.BLK_RAW_FLAGS == 5


def test_python_surface():
    from vdlm2dec_amd import demod
    p = inspect.signature(demod.Receiver.__init__).parameters
    assert p["raw_flags"].default is False and p["all_frames"].default is False
    p = inspect.signature(demod.Receiver.decode_blocks).parameters
    assert p["raw_flags"].default is False and p["all_frames"].default is False
    rx = demod.Receiver.__new__(demod.Receiver)      # no handle: neither call reaches the library
    with pytest.raises(ValueError, match="raw_flags"):
        rx.decode_blocks([], raw_flags=True)
    assert rx.decode_blocks([], all_frames=True, raw_flags=True) == []
    with pytest.raises(ValueError, match="raw_flags"):
        demod.Receiver(2_000_000, demod.plan_channels(136_975_000, [-50000]), frames=True, raw_flags=True)


def test_exports_are_unchanged(built):
    from vdlm2dec_amd import lib
    assert not any("raw" in n for n in lib.EXPORTS)       # the mode needs no call of its own
    for so in ("libvdl2gpu.so", "libvdl2gpu_test.so"):
        out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "vdlm2dec_amd", so)], text=True)
        names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
        assert not any("k4_frames" in n for n in names), so                            # no kernel stub
        assert {n for n in names if n.startswith(("vdl2gpu_", "reversebits"))} <= set(lib.EXPORTS), so
        assert "vdl2gpu_decode_blocks_ex" in names
