"""VDL2GPU_F_BLOCK_REPORT without a GPU: the header, the ctypes mirror of vdl2gpu_blockrep_t against the compiler, the exports, the
flag rule of vdl2gpu_create (refused before any device call, with a text), and the Python surface."""
import ctypes as C
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "vdl2gpu.h")

FIELDS = ["row_roots", "row_how", "row_changed", "bytes_changed", "rows_failed", "rows_rescued", "stuffed", "nbytes", "flag_at",
          "cand", "too_short", "bad_fcs", "frames", "status"]
OFFSETS = [0, 8, 16, 24, 26, 28, 30, 32, 34, 36, 38, 40, 42, 44]


def test_header_declares_the_report():
    text = open(HDR).read()
    assert re.search(r"#define VDL2GPU_F_BLOCK_REPORT 2048u", text)
    assert re.search(r"#define VDL2GPU_HAVE_BLOCK_REPORT 1\b", text)
    assert re.search(r"#define VDL2GPU_ABI_VERSION 6\b", text)
    assert "} vdl2gpu_blockrep_t;" in text
    for i, name in enumerate(("NONE", "CLEAN", "REF", "SOFT2", "SOFT4", "FAIL")):
        assert re.search(rf"#define VDL2GPU_ROW_{name} {i}\b", text), name
    args = (r"\(vdl2gpu_t \*h, vdl2gpu_burst_t \*out, vdl2gpu_level_t \*lv, vdl2gpu_soft_t \*soft, vdl2gpu_carrier_t \*car, "
            r"vdl2gpu_blockrep_t \*rep, int max\);")
    assert re.search(r"int vdl2gpu_poll_report" + args, text)
    assert re.search(r"int vdl2gpu_poll_report_ready" + args, text)
    assert re.search(r"int vdl2gpu_decode_blocks_report\(vdl2gpu_t \*h, const vdl2gpu_burst_t \*blocks, const vdl2gpu_soft_t \*soft, int n,\s*"
                     r"vdl2gpu_frame_t \*frames, int max_frames, int \*dropped, vdl2gpu_blockrep_t \*rep\);", text)
    # what the comment owes the reader
    body = text[text.index("VDL2GPU_F_BLOCK_REPORT; announced by"):text.index("#define VDL2GPU_F_BLOCK_REPORT 2048u")]
    for phrase in ("function of the burst record alone", "reliability map", "whatever kernel, path or repair round", "however the stream was cut",
                   "stays the received rows", "48 bytes per record slot", "needs VDL2GPU_F_FRAMES", "error too short", "error crc"):
        assert phrase in body, phrase


def test_layout_matches_the_compiler(tmp_path):
    from vdlm2dec_amd import lib
    assert lib.F_BLOCK_REPORT == 2048
    assert [f for f, _ in lib.BlockRepT._fields_] == FIELDS
    src = tmp_path / "rep.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vdl2gpu.h"\nint main(void){printf("%zu %zu", sizeof(vdl2gpu_blockrep_t), _Alignof(vdl2gpu_blockrep_t));'
                   + "".join(f'printf(" %zu", offsetof(vdl2gpu_blockrep_t, {f}));' for f in FIELDS)
                   + 'printf(" %d %d %d %d %d %d", VDL2GPU_ROW_NONE, VDL2GPU_ROW_CLEAN, VDL2GPU_ROW_REF, VDL2GPU_ROW_SOFT2, VDL2GPU_ROW_SOFT4, VDL2GPU_ROW_FAIL);'
                   + 'printf("\\n");return 0;}\n')
    exe = tmp_path / "rep"
    subprocess.check_call(["cc", "-std=c11", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got[0] == C.sizeof(lib.BlockRepT) == 48
    assert got[1] == C.alignment(lib.BlockRepT) == 4
    assert got[2:2 + len(FIELDS)] == [getattr(lib.BlockRepT, f).offset for f in FIELDS] == OFFSETS
    assert got[2 + len(FIELDS):] == [lib.ROW_NONE, lib.ROW_CLEAN, lib.ROW_REF, lib.ROW_SOFT2, lib.ROW_SOFT4, lib.ROW_FAIL] == list(range(6))


def test_library_exports_the_calls(built):
    from vdlm2dec_amd import lib
    L = lib.load()
    for s in ("vdl2gpu_poll_report", "vdl2gpu_poll_report_ready", "vdl2gpu_decode_blocks_report"):
        assert s in lib.EXPORTS and hasattr(L, s), s
    assert L.vdl2gpu_abi_version() == 6
    # a null handle is refused like everywhere else
    assert L.vdl2gpu_poll_report(None, None, None, None, None, None, 0) == -1
    assert L.vdl2gpu_poll_report_ready(None, None, None, None, None, None, 0) == -1
    assert L.vdl2gpu_decode_blocks_report(None, None, None, 0, None, 0, None, None) == -1


def _config(lib, flags):
    chan = (lib.ChanT * 1)(lib.ChanT(0, 136975000, 100000))
    cfg = lib.ConfigT()
    cfg.struct_size = C.sizeof(lib.ConfigT)
    cfg.sdrinrate, cfg.fmt, cfg.nbch, cfg.nstreams, cfg.chan, cfg.max_push = 2_000_000, 0, 1, 1, chan, 1 << 20
    cfg.flags = flags
    return cfg, chan


def test_report_without_frames_is_einval_before_any_device_call(built):
    """VDL2GPU_EINVAL whether there is a GPU or not -- a configuration this machine could not serve otherwise gives VDL2GPU_ENODEV or
    a handle, so EINVAL says the check stands in front of every device call -- and vdl2gpu_last_error(NULL) says why"""
    from vdlm2dec_amd import lib
    L = lib.load()
    for extra in (0, lib.F_LEVELS, lib.F_SOFT_RS | lib.F_CARRIER):
        cfg, _chan = _config(lib, lib.F_BLOCK_REPORT | extra)
        h = C.c_void_p()
        assert L.vdl2gpu_create(C.byref(cfg), C.byref(h)) == -1
        assert not h.value
        text = L.vdl2gpu_last_error(None).decode()
        assert "VDL2GPU_F_BLOCK_REPORT" in text and "VDL2GPU_F_FRAMES" in text
    # the text belongs to the last create: another refusal clears it
    cfg, _chan = _config(lib, 0)
    cfg.nbch = 0
    assert L.vdl2gpu_create(C.byref(cfg), C.byref(h)) == -1
    assert L.vdl2gpu_last_error(None).decode() == "null handle"


def test_python_surface():
    from vdlm2dec_amd import demod, lib
    assert demod.Burst.__dataclass_fields__["report"].default is None
    b = demod.Burst(0, 0, 0, 1, 20, 0.0, 0.0, 0, 0, 0, 0, bytes(2040), report=demod.BlockReport.from_c(lib.BlockRepT()))
    assert b.key() == demod.Burst(0, 0, 0, 1, 20, 0.0, 0.0, 0, 0, 0, 0, bytes(2040)).key()      # not part of key()
    c = lib.BlockRepT()
    c.row_roots[1], c.row_how[1], c.row_changed[1], c.flag_at, c.frames, c.status = -1, 5, 7, -1, 3, 1
    r = demod.BlockReport.from_c(c)
    assert (r.row_roots[1], r.row_how[1], r.row_changed[1], r.flag_at, r.frames, r.status) == (-1, 5, 7, -1, 3, 1)
    assert len(r.row_roots) == len(r.row_how) == len(r.row_changed) == 8
    assert inspect.signature(demod.Receiver.__init__).parameters["block_report"].default is False
    assert hasattr(demod.Receiver, "poll_report_raw")


def test_decode_blocks_keeps_its_return_shape():
    """report=False (the default) returns the list of frames as before, also for an empty batch; report=True a pair"""
    from vdlm2dec_amd import demod
    p = inspect.signature(demod.Receiver.decode_blocks).parameters
    assert p["report"].default is False and list(p)[:4] == ["self", "blocks", "max_frames", "soft"]
    rx = demod.Receiver.__new__(demod.Receiver)      # no handle: an empty batch never reaches the library
    assert rx.decode_blocks([]) == [] and rx.decode_blocks([], report=False) == []
    assert rx.decode_blocks([], report=True) == ([], [])
