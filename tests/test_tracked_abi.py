"""VDL2GPU_F_TRACKED without a GPU: the header, the ctypes mirror of vdl2gpu_trk_t against the compiler, the exports, the Python
mirror."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "vdl2gpu.h")
FIELDS = ["data", "d_first", "d_last", "d_min", "d_max", "nseg", "reserved"]


def test_header_declares_the_tracked_column():
    text = open(HDR).read()
    assert re.search(r"#define VDL2GPU_F_TRACKED 65536u", text)
    assert re.search(r"#define VDL2GPU_HAVE_TRACKED 1\b", text)
    assert re.search(r"#define VDL2GPU_ROW_TRACKED 7\b", text)
    assert re.search(r"#define VDL2GPU_TRK_SEGS 22\b", text) and "} vdl2gpu_trk_t;" in text
    assert re.search(r"#define VDL2GPU_ABI_VERSION 6\b", text)
    args = (r"\(vdl2gpu_t \*h, vdl2gpu_burst_t \*out, vdl2gpu_level_t \*lv, vdl2gpu_soft_t \*soft, vdl2gpu_carrier_t \*car, "
            r"vdl2gpu_blockrep_t \*rep,\s*vdl2gpu_fb_t \*fb, vdl2gpu_symclk_t \*clk, vdl2gpu_trk_t \*trk, int max\);")
    assert re.search(r"int vdl2gpu_poll_tracked" + args, text) and re.search(r"int vdl2gpu_poll_tracked_ready" + args, text)
    assert re.search(r"int vdl2gpu_decode_blocks_tracked\(vdl2gpu_t \*h, const vdl2gpu_burst_t \*blocks, const vdl2gpu_soft_t \*soft, "
                     r"const vdl2gpu_fb_t \*fb,\s*const vdl2gpu_trk_t \*trk, int n,", text)
    body = text[text.index("VDL2GPU_F_TRACKED; announced by"):text.index("#define VDL2GPU_F_TRACKED 65536u")]
    for phrase in ("quarter samples", "GREATER THAN end_dec count as 0", "0, -1, -2, -3", "strictly smaller cost", "PER BURST",
                   "attempt A", "attempt B", "VDL2GPU_ROW_TRACKED", "2^-16 chance", "2048 bytes per record slot"):
        assert phrase in body, phrase


def test_layout_matches_the_compiler(tmp_path):
    from vdlm2dec_amd import lib
    assert lib.F_TRACKED == 65536 and (lib.TRK_SEG, lib.TRK_SEGS, lib.ROW_TRACKED) == (256, 22, 7)
    assert [f for f, _ in lib.TrkT._fields_] == FIELDS
    src = tmp_path / "trk.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vdl2gpu.h"\nint main(void){printf("%u %d %d %d %d %zu", VDL2GPU_F_TRACKED, '
                   'VDL2GPU_HAVE_TRACKED, VDL2GPU_TRK_SEG, VDL2GPU_TRK_SEGS, VDL2GPU_ROW_TRACKED, sizeof(vdl2gpu_trk_t));'
                   + "".join(f'printf(" %zu", offsetof(vdl2gpu_trk_t, {f}));' for f in FIELDS) + 'printf("\\n");return 0;}\n')
    exe = tmp_path / "trk"
    subprocess.check_call(["cc", "-std=c11", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got[:5] == [65536, 1, 256, 22, 7]
    assert got[5] == C.sizeof(lib.TrkT) == 2048
    assert got[6:] == [getattr(lib.TrkT, f).offset for f in FIELDS] == [0, 2040, 2041, 2042, 2043, 2044, 2045]
    # 22 segments of 256 symbols cover the payload symbols of the longest burst: kmax - 7 with 8 x 255 bytes
    assert ((25 + 8 * 8 * 255 - 1) // 3 - 7 + 255) // 256 == 22


def test_library_exports_the_calls(built):
    from vdlm2dec_amd import lib
    L = lib.load()
    for s in ("vdl2gpu_poll_tracked", "vdl2gpu_poll_tracked_ready", "vdl2gpu_decode_blocks_tracked"):
        assert s in lib.EXPORTS and hasattr(L, s), s
    assert L.vdl2gpu_poll_tracked(None, None, None, None, None, None, None, None, None, 0) == -1
    assert L.vdl2gpu_poll_tracked_ready(None, None, None, None, None, None, None, None, None, 0) == -1
    assert L.vdl2gpu_decode_blocks_tracked(None, None, None, None, None, 0, None, 0, None, None, 0) == -1


def test_python_mirror(built):
    from vdlm2dec_amd import demod
    assert demod.Burst.__dataclass_fields__["trk"].default is None
    assert [c[0] for c in demod._ALL_COLUMNS][-1] == "tracked" and demod._ALL_COLUMNS[:len(demod._COLUMNS)] == demod._COLUMNS
    import inspect
    assert "tracked" in inspect.signature(demod.Receiver.__init__).parameters
    assert "trk" in inspect.signature(demod.Receiver.decode_blocks).parameters
