"""VDL2GPU_F_ALL_FRAMES without a GPU: the header's defines and rule, vdl2gpu_decode_blocks_ex against the compiler, the export list and
the ctypes mirror, what is refused before any device call, and the transmitter's unchanged defaults."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "vdl2gpu.h")


def test_header_defines_the_flag_and_states_the_rule():
    text = open(HDR).read()
    assert re.search(r"#define VDL2GPU_F_ALL_FRAMES 8192u", text)
    assert re.search(r"#define VDL2GPU_HAVE_ALL_FRAMES 1\b", text)
    assert re.search(r"#define VDL2GPU_BLK_ALL_FRAMES 1u", text)
    assert re.search(r"#define VDL2GPU_ABI_VERSION 6\b", text)
    assert re.search(r"int vdl2gpu_decode_blocks_ex\(vdl2gpu_t \*h, const vdl2gpu_burst_t \*blocks, const vdl2gpu_soft_t \*soft, "
                     r"const vdl2gpu_fb_t \*fb, int n,\s*vdl2gpu_frame_t \*frames, int max_frames, int \*dropped, vdl2gpu_blockrep_t \*rep, "
                     r"uint32_t mode\);", text)
    body = text[text.index("VDL2GPU_F_ALL_FRAMES; announced by"):text.index("#define VDL2GPU_F_ALL_FRAMES 8192u")]
    for phrase in ("s_0 = m1, s_{j+1} = q_j + 1", "= q_j - s_j + 2", "l_j == 2", "l_j >= 13", "0xf0b8", "B[s_j .. q_j - 1]",
                   "data = 0x7e, B[s_j .. q_j], len = l_j", "rank among the passing", "needs VDL2GPU_F_FRAMES", "are not formed in this mode",
                   "the first 12 in stream order", "bytes behind the last flag are ignored", "nothing is re-aligned at bit level",
                   "cand == too_short + bad_fcs + frames", "(end_dec, stream, chn, seq)", "data byte 0x7e"):
        assert phrase in body, phrase
    st = text[text.index("uint64_t frames_dropped;"):text.index("uint64_t repairs;")]
    assert "VDL2GPU_F_ALL_FRAMES" in st and "13th passing segment" in st


def test_values_and_declaration_match_the_compiler(tmp_path):
    from vdlm2dec_amd import lib
    assert lib.F_ALL_FRAMES == 8192 and lib.BLK_ALL_FRAMES == 1
    flags = [getattr(lib, n) for n in dir(lib) if n.startswith("F_")]
    assert len(set(flags)) == len(flags) and all(f & (f - 1) == 0 for f in flags)       # one bit each, none shared
    inc = "-I" + os.path.join(ROOT, "include")
    proto = tmp_path / "proto.c"
    # (the assignment to a pointer of the written-out type is the compiler's check of the declaration; compiled, never linked)
    proto.write_text('#include "vdl2gpu.h"\n'
                     "int (*fn)(vdl2gpu_t *, const vdl2gpu_burst_t *, const vdl2gpu_soft_t *, const vdl2gpu_fb_t *, int, vdl2gpu_frame_t *, int, int *, "
                     "vdl2gpu_blockrep_t *, uint32_t) = vdl2gpu_decode_blocks_ex;\n")
    subprocess.check_call(["cc", "-std=c11", "-Wall", "-Werror", inc, "-c", str(proto), "-o", str(tmp_path / "proto.o")])
    src = tmp_path / "af.c"
    src.write_text('#include <stdio.h>\n#include "vdl2gpu.h"\n'
                   'int main(void){printf("%u %d %u %d %zu\\n", VDL2GPU_F_ALL_FRAMES, VDL2GPU_HAVE_ALL_FRAMES, VDL2GPU_BLK_ALL_FRAMES, '
                   "VDL2GPU_ABI_VERSION, sizeof(vdl2gpu_blockrep_t));return 0;}\n")
    exe = tmp_path / "af"
    subprocess.check_call(["cc", "-std=c11", "-Wall", "-Werror", inc, str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [8192, 1, 1, 6, 48]


def test_export_and_ctypes_mirror(built):
    from vdlm2dec_amd import lib
    assert "vdl2gpu_decode_blocks_ex" in lib.EXPORTS
    for so in ("libvdl2gpu.so", "libvdl2gpu_test.so"):
        out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "vdlm2dec_amd", so)], text=True)
        names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
        assert "vdl2gpu_decode_blocks_ex" in names and not any("k4_frames" in n for n in names), so      # the call, and no kernel stub
    L = lib.load()
    fn = L.vdl2gpu_decode_blocks_ex
    assert fn.restype is C.c_int and len(fn.argtypes) == 10 and fn.argtypes[9] is C.c_uint32
    assert fn.argtypes[:9] == L.vdl2gpu_decode_blocks_feedback.argtypes
    assert L.vdl2gpu_abi_version() == 6


def test_refused_before_any_device_call(built):
    """the flag without VDL2GPU_F_FRAMES, a null handle and an unknown mode bit: VDL2GPU_EINVAL, whatever the machine"""
    from vdlm2dec_amd import lib
    L = lib.load()
    chan = (lib.ChanT * 1)(lib.ChanT(0, 136_975_000, -50_000))
    cfg = lib.ConfigT(struct_size=C.sizeof(lib.ConfigT), sdrinrate=2_000_000, fmt=0, nbch=1, nstreams=1, chan=chan,
                      max_push=32768, flags=lib.F_ALL_FRAMES)
    h = C.c_void_p()
    assert L.vdl2gpu_create(C.byref(cfg), C.byref(h)) == -1
    msg = L.vdl2gpu_last_error(None).decode()
    assert "VDL2GPU_F_ALL_FRAMES needs VDL2GPU_F_FRAMES" in msg
    cfg.flags = lib.F_ALL_FRAMES | lib.F_BLOCK_REPORT          # (the report's own refusal comes first, as before)
    assert L.vdl2gpu_create(C.byref(cfg), C.byref(h)) == -1
    assert "VDL2GPU_F_BLOCK_REPORT needs VDL2GPU_F_FRAMES" in L.vdl2gpu_last_error(None).decode()
    assert L.vdl2gpu_decode_blocks_ex(None, None, None, None, 0, None, 0, None, None, lib.BLK_ALL_FRAMES) == -1
    fake = C.c_void_p(1)        # never dereferenced: the mode word is looked at first
    blk, fr = (lib.BurstT * 1)(), (lib.FrameT * 1)()
    for mode in (2, 3, 0x80000000):
        assert L.vdl2gpu_decode_blocks_ex(fake, blk, None, None, 1, fr, 1, None, None, mode) == -1, mode


def test_python_surface():
    from vdlm2dec_amd import demod
    assert inspect.signature(demod.Receiver.__init__).parameters["all_frames"].default is False
    p = inspect.signature(demod.Receiver.decode_blocks).parameters
    assert p["all_frames"].default is False
    rx = demod.Receiver.__new__(demod.Receiver)      # no handle: an empty batch never reaches the library
    assert rx.decode_blocks([], all_frames=True) == [] and rx.decode_blocks([], all_frames=True, report=True) == ([], [])


def test_transmitter_defaults_are_unchanged():
    """hdlc_payload(f) is hdlc_payload_multi([f]); a Burst without infos sends the bytes it sent: the frame, FCS and flags written out here"""
    from vdlm2dec_amd import synth
    rng = np.random.default_rng(3)
    for n in (0, 1, 5, 40, 300):
        f = synth.avlc_frame(bytes(rng.integers(0, 256, n, dtype=np.uint8).tolist()))
        assert synth.hdlc_payload_multi([f]) == synth.hdlc_payload(f)
    import blocks_craft as K
    for chan, info in ((0, b"hello"), (3, bytes(range(256))), (7, b"\xff" * 30 + b"\x7e" * 3)):
        b = synth.Burst(chan=chan, t0=0.0, info=info)
        f = synth.avlc_frame(info, src=(1 << 24) | (0x400000 + chan * 0x111 + len(info)))
        assert b.frames() == [f] and b.payload() == K.frame(f)          # blocks_craft's builder: flag, stuffed frame + FCS, flag, padding
    spec = synth.random_scenario(2_000_000, synth.DEFAULT_FO_8CH, 1 << 19, seed=4)
    assert all(b.infos is None for b in spec.bursts)
    assert "frames_per_burst" in inspect.signature(synth.random_scenario).parameters


def test_transmitter_sends_several_frames():
    from vdlm2dec_amd import synth
    import blocks_craft as K
    a, b, c = (synth.avlc_frame(bytes([i]) * (3 + i)) for i in range(3))
    one = synth.hdlc_payload_multi([a, b, c])
    bits = lambda f: K.stuff(K.bits_of(f + bytes([synth.fcs16(f) & 0xff, synth.fcs16(f) >> 8])))      # noqa: E731
    assert one == K.bytes_of(K.FLAG + bits(a) + K.FLAG + bits(b) + K.FLAG + bits(c) + K.FLAG)
    assert synth.hdlc_payload_multi([a, b], flags_between=3) == K.bytes_of(K.FLAG + bits(a) + K.FLAG * 3 + bits(b) + K.FLAG)
    bu = synth.Burst(chan=2, t0=0.0, info=b"", infos=[b"x", b"x", b"yy"])
    fr = bu.frames()
    assert len(fr) == 3 and len({f[4:8] for f in fr}) == 3          # distinct src addresses
    assert bu.payload() == synth.hdlc_payload_multi(fr)
    spec = synth.random_scenario(2_000_000, synth.DEFAULT_FO_8CH, 1 << 19, seed=4, frames_per_burst=3)
    assert spec.bursts and all(len(b.infos) == 3 and b.infos[0] == b.info for b in spec.bursts)
