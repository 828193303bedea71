"""The C-ABI shared library: loads, exports everything include/vdl2gpu.h declares, host-only helpers
agree with the oracle, and it refuses to run without a GPU (no CPU fallback)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exports_every_declared_symbol(built):
    from vdlm2dec_amd import lib
    L = lib.load()
    hdr = open(os.path.join(ROOT, "include", "vdl2gpu.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(vdl2gpu_[a-z0-9_]+|reversebits)\s*\(", hdr))
    declared = {d for d in declared if not d.endswith("_t")}
    assert declared == set(lib.EXPORTS)
    for name in declared:
        assert hasattr(L, name), name
    assert L.vdl2gpu_abi_version() == 6


def test_exports_nothing_but_the_c_abi(built):
    """The product library is linked into C programs (dropin/): it exports the C ABI and the one symbol of d8psk.c
    that out.c still calls -- no kernel stubs, no C++ runtime symbols (-fvisibility=hidden + csrc/vdl2gpu.map; round 5 exported
    53 symbols, every __device_stub__ among them)."""
    import subprocess
    from vdlm2dec_amd import lib
    for so in ("libvdl2gpu.so", "libvdl2gpu_test.so"):
        out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "vdlm2dec_amd", so)], text=True)
        names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
        assert names == set(lib.EXPORTS), (so, sorted(names ^ set(lib.EXPORTS)))


def test_struct_layouts_match_header(built):
    from vdlm2dec_amd import lib
    assert C.sizeof(lib.BurstT) == 64 + 8 * 255          # data at offset 64, see vdl2gpu_kernels.h
    assert lib.BurstT.data.offset == 64
    assert C.sizeof(lib.ChanT) == 12                      # == thread_param_t, vdlm2.h:49-52
    assert C.sizeof(lib.ConfigT) == 56


def test_reversebits_exported_for_host_path(built, oracle):
    from vdlm2dec_amd import lib
    L, O = lib.load(), oracle.lib()
    for v, n in ((0x2A, 6), (0x55, 7), (0x12345, 17), (1, 1)):
        assert L.reversebits(v, n) == O.vo_reversebits(v, n)


def test_burst_to_msgblk_layout(built):
    """msgblk_t on LP64 (vdlm2.h:39-47): chn@8 Fr@12 ppm@32 nbrow@36 nlbyte@40 data@44, 16624 bytes."""
    from vdlm2dec_amd import lib
    L = lib.load()
    b = lib.BurstT()
    b.chn, b.Fr, b.nbrow, b.nlbyte, b.ppm = 3, 136975000, 2, 17, -4.75
    for r in range(8):
        for i in range(255):
            b.data[r][i] = (r * 255 + i) & 0xFF
    blk = (C.c_uint8 * 16624)()
    assert L.vdl2gpu_burst_to_msgblk(C.byref(b), blk, 16624) == 0
    raw = bytes(blk)
    assert np.frombuffer(raw[8:16], "<i4").tolist() == [3, 136975000]
    assert np.frombuffer(raw[32:36], "<f4")[0] == np.float32(-4.75)
    assert np.frombuffer(raw[36:44], "<i4").tolist() == [2, 17]
    assert raw[44:44 + 8 * 255] == bytes(b.data)
    assert raw[:8] == b"\0" * 8 and raw[16:32] == b"\0" * 16 and set(raw[44 + 2040:]) == {0}
    assert L.vdl2gpu_burst_to_msgblk(C.byref(b), blk, 100) == -1


@pytest.mark.parametrize("rate", [2_000_000, 5_000_000, 6_000_000, 10_000_000, 100_000, 2_025_000, 2_400_000, 2_500_000, 25_700_000])
def test_lo_table_equals_reference_formula(built, oracle, rate):
    """Host LO table (sincosf) == the oracle's cexpf table (d8psk.c:353-357), bit for bit."""
    from vdlm2dec_amd.demod import lo_table
    rng = np.random.default_rng(rate)
    fos = [-450000, -50000, 100000, 25000, 975000, -123457, 1] + [int(v) for v in rng.integers(-rate // 2, rate // 2, 40)]
    for fo in fos:
        ch = oracle.OracleChannel(rate, fo, 136_000_000 + fo)
        assert np.array_equal(ch.lo_table().view(np.uint32), lo_table(rate, fo).view(np.uint32)), fo
        ch.close()


def test_create_rejects_bad_config_and_missing_gpu(built):
    import torch
    from vdlm2dec_amd import lib
    from vdlm2dec_amd.demod import Receiver, ThreadParam
    L = lib.load()
    assert L.vdl2gpu_create(None, None) == -1
    with pytest.raises(lib.Vdl2GpuError):
        Receiver(2_000_000, [ThreadParam(0, 1, 1)], fmt="cu8", max_push=0)
    with pytest.raises(lib.Vdl2GpuError):
        Receiver(2_000_001, [ThreadParam(0, 1, 1)], fmt="cu8")
    if not torch.cuda.is_available():
        # the product must fail loudly, never fall back to a CPU path
        with pytest.raises(lib.Vdl2GpuError, match="no HIP device"):
            Receiver(2_000_000, [ThreadParam(0, 136975000, -50000)], fmt="cu8")


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "vdlm2dec_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".c", ".cpp")):
                txt = open(os.path.join(dirpath, f), errors="ignore").read()
                assert "oracle" not in txt.replace("the oracle", "").replace("oracle's", "") or f in ("vdl2_math.h",), \
                    f"{f} mentions the oracle"


def test_test_handicaps_exist_only_in_the_test_build(built):
    """libvdl2gpu.so (the product) rejects VDL2GPU_F_TEST_NOREGION and has no code for the VDL2GPU_PRIM_DROP /
    VDL2GPU_SPLIT_SAMPLES / VDL2GPU_TEST_EPOCH / VDL2GPU_TEST_TICKET0 handicaps; libvdl2gpu_test.so (-DVDL2GPU_TESTHOOKS) is what the tests load for them.
    The flag is checked before any device is touched, so this runs without a GPU."""
    from vdlm2dec_amd import lib
    prod, test = lib.load(), lib.load(testhooks=True)
    for name in lib.EXPORTS:
        assert hasattr(test, name), name
    chan = (lib.ChanT * 1)(lib.ChanT(0, 136_975_000, -50_000))
    cfg = lib.ConfigT(struct_size=C.sizeof(lib.ConfigT), sdrinrate=2_000_000, fmt=0, nbch=1, nstreams=1, chan=chan,
                      max_push=32768, flags=lib.F_TEST_NOREGION)
    h = C.c_void_p()
    assert prod.vdl2gpu_create(C.byref(cfg), C.byref(h)) == -1          # VDL2GPU_EINVAL, whatever the machine
    rc = test.vdl2gpu_create(C.byref(cfg), C.byref(h))
    assert rc in (0, -5)                                                    # accepted: a handle, or ENODEV without a GPU
    if rc == 0:
        test.vdl2gpu_destroy(h)
    blob = open(lib.LIB_PATH, "rb").read()
    assert b"VDL2GPU_PRIM_DROP" not in blob and b"VDL2GPU_SPLIT_SAMPLES" not in blob and b"VDL2GPU_TEST_ITEM" not in blob
    tblob = open(lib.LIB_TEST_PATH, "rb").read()
    assert b"VDL2GPU_PRIM_DROP" in tblob and b"VDL2GPU_TEST_ITEM_GRID" in tblob and b"VDL2GPU_TEST_ITEM_COMMON" in tblob
    assert b"VDL2GPU_FRAME_ARENA" not in blob and b"VDL2GPU_FRAME_ARENA" in tblob       # the frame arena's size (tests/test_gpu_full.py)
    for name in (b"VDL2GPU_TEST_EPOCH", b"VDL2GPU_TEST_TICKET0"):       # the stream epoch and k1_fast's first ticket (tests/test_gpu_epoch.py)
        assert name not in blob and name in tblob, name
    assert _getenv_outside_create(_host_sources()) == []                    # every knob is read once, in create_impl


def _host_sources() -> dict:
    """vdl2gpu.hip and every header of its directory that it includes, directly or through another: {file name: text}"""
    import re
    csrc = os.path.join(ROOT, "vdlm2dec_amd", "csrc")
    out, todo = {}, ["vdl2gpu.hip"]
    while todo:
        f = todo.pop()
        if f in out or not os.path.exists(os.path.join(csrc, f)):
            continue
        out[f] = open(os.path.join(csrc, f)).read()
        todo += re.findall(r'#include "([^"]+)"', out[f])
    return out


def _getenv_outside_create(sources: dict) -> list:
    """Files of the library that call getenv anywhere but in the bodies of create_impl and vdl2gpu_create (vdl2gpu.hip)."""
    def cut(text, head):
        a = text.index(head + "\n{\n")
        return text[:a] + text[text.index("\n}\n", a) + 3:]
    sources = dict(sources)
    hip = cut(sources["vdl2gpu.hip"], "static int create_impl(vdl2gpu_t *h)")
    sources["vdl2gpu.hip"] = cut(hip, 'extern "C" int vdl2gpu_create(const vdl2gpu_config_t *cfg, vdl2gpu_t **out)')
    return sorted(f for f, text in sources.items() if "getenv" in text)


def test_a_getenv_in_a_push_helper_is_caught():
    """the check above is not vacuous: a getenv in a function push_impl calls, or in a header, is found"""
    src = _host_sources()
    assert "vdl2gpu_kernels.h" in src and "vdl2gpu_k1.h" in src
    a = dict(src)
    a["vdl2gpu.hip"] = a["vdl2gpu.hip"].replace("static int enqueue_front(vdl2gpu_t *h, hipStream_t fs, long long dec_base, PushTiming &pt)\n{\n",
                                                  "static int enqueue_front(vdl2gpu_t *h, hipStream_t fs, long long dec_base, PushTiming &pt)\n{\n\tif (getenv(\"X\"))\n\t\treturn 0;\n")
    assert a["vdl2gpu.hip"] != src["vdl2gpu.hip"] and _getenv_outside_create(a) == ["vdl2gpu.hip"]
    b = dict(src)
    b["vdl2gpu_k1.h"] += "\nstatic inline int k1_env() { return getenv(\"X\") != nullptr; }\n"
    assert _getenv_outside_create(b) == ["vdl2gpu_k1.h"]


def _layout_check_source(lay: dict) -> str:
    """the checks of oracle/ref_layout_check.c with the reference's offsetof()/sizeof() replaced by their recorded values"""
    m, t = lay["msgblk_t"], lay["thread_param_t"]
    checks = [(f"VDL2GPU_MSGBLK_OFF_{k.upper()} == {m[k]}", f"msgblk_t.{k}") for k in ("chn", "Fr", "tv", "ppm", "nbrow", "nlbyte", "data")]
    checks += [(f"VDL2GPU_MSGBLK_SIZE == {m['size']}", "sizeof(msgblk_t)"),
               (" && ".join(f"{m['widths'][k]} == 4" for k in ("chn", "Fr", "ppm", "nbrow", "nlbyte")), "msgblk_t field widths"),
               (f"VDL2GPU_ROWLEN == {m['row_len']} && {m['data_bytes']} >= VDL2GPU_MAXROWS * VDL2GPU_ROWLEN", "msgblk_t.data rows"),
               (f"sizeof(vdl2gpu_chan_t) == {t['size']} && offsetof(vdl2gpu_chan_t, Fr) == {t['Fr']} && offsetof(vdl2gpu_chan_t, Fo) == {t['Fo']}",
                "thread_param_t"),
               (f"VDL2GPU_MAXCH == {lay['MAXNBCHANNELS']}", "MAXNBCHANNELS")]
    return "#include <stddef.h>\n#include \"vdl2gpu.h\"\n" + "".join(f"_Static_assert({c}, \"{msg}\");\n" for c, msg in checks)


def test_msgblk_offsets_are_checked_against_the_reference_header(tmp_path):
    """oracle/ref_layout_check.c (_Static_assert against the reference's own vdlm2.h) is part of `make -C oracle ref`;
    with one constant of include/vdl2gpu.h changed it must refuse to compile.  The same checks run everywhere against the
    reference's layout as recorded in tests/golden/layout/msgblk_layout.json; against its vdlm2.h itself where its sources are at hand."""
    import json
    import subprocess
    lay = json.load(open(os.path.join(ROOT, "tests", "golden", "layout", "msgblk_layout.json")))
    chk = tmp_path / "layout_check.c"
    chk.write_text(_layout_check_source(lay))
    hdr = open(os.path.join(ROOT, "include", "vdl2gpu.h")).read()
    (tmp_path / "changed").mkdir()
    (tmp_path / "changed" / "vdl2gpu.h").write_text(hdr.replace("VDL2GPU_MSGBLK_OFF_NBROW 36", "VDL2GPU_MSGBLK_OFF_NBROW 40"))
    for inc, good in ((os.path.join(ROOT, "include"), True), (str(tmp_path / "changed"), False)):
        r = subprocess.run(["gcc", "-std=c11", "-I" + inc, "-w", "-c", "-o", str(tmp_path / "l.o"), str(chk)], capture_output=True, text=True)
        assert (r.returncode == 0) == good, r.stderr
        assert good or "msgblk_t.nbrow" in r.stderr
    if not os.path.isdir("/root/reference"):
        return
    src = os.path.join(ROOT, "oracle", "ref_layout_check.c")
    ok = subprocess.run(["gcc", "-std=c11", "-DWITH_RTL", "-I/root/reference", "-I" + os.path.join(ROOT, "include"), "-w",
                         "-c", "-o", str(tmp_path / "a.o"), src], capture_output=True, text=True)
    assert ok.returncode == 0, ok.stderr
    hdr = open(os.path.join(ROOT, "include", "vdl2gpu.h")).read().replace("VDL2GPU_MSGBLK_OFF_NBROW 36", "VDL2GPU_MSGBLK_OFF_NBROW 40")
    (tmp_path / "vdl2gpu.h").write_text(hdr)
    bad = subprocess.run(["gcc", "-std=c11", "-DWITH_RTL", "-I/root/reference", "-I" + str(tmp_path), "-w",
                          "-c", "-o", str(tmp_path / "b.o"), src], capture_output=True, text=True)
    assert bad.returncode != 0 and "msgblk_t.nbrow" in bad.stderr


def _plane_frames(max_push, sdrclk):
    """create_impl's frames per channel plane (vdl2gpu.hip: plane_frames)"""
    return (49152 + 21 * max_push // sdrclk + 2 + 64 + 15) // 16 * 16


@pytest.mark.parametrize("sdrclk", [0, 22])
def test_create_rejects_planes_of_4_gib(built, sdrclk):
    """k1_fast addresses a stream's 8 planes with 32-bit byte offsets, so vdl2gpu_create refuses a max_push whose planes would
    reach 4 GiB -- before any device call.  The largest max_push below the limit passes that check (a handle on a GPU, ENODEV
    without one); one more sample, which adds a frame, is VDL2GPU_EINVAL on any machine.  With a GPU present only the rejected
    half runs: a handle just below the limit would allocate more than 12 GB for nothing."""
    import torch
    from vdlm2dec_amd import lib
    clk = sdrclk or 2_000_000 // 4000
    lo, hi = 1, 1 << 40                  # the smallest max_push whose planes reach 4 GiB
    while lo < hi:
        m = (lo + hi) // 2
        if _plane_frames(m, clk) * 8 * 8 >= 1 << 32:
            hi = m
        else:
            lo = m + 1
    assert _plane_frames(lo - 1, clk) == (1 << 26) - 16 and _plane_frames(lo, clk) == 1 << 26
    assert lo == {500: 1_596_657_881, 22: 70_252_947}[clk]     # the values include/vdl2gpu.h states
    L = lib.load()
    chan = (lib.ChanT * 1)(lib.ChanT(0, 136_975_000, -50_000))

    def create(max_push):
        cfg = lib.ConfigT(struct_size=C.sizeof(lib.ConfigT), sdrinrate=2_000_000, sdrclk=sdrclk, fmt=1, nbch=1, nstreams=1,
                          chan=chan, max_push=max_push)
        h = C.c_void_p()
        rc = L.vdl2gpu_create(C.byref(cfg), C.byref(h))
        if rc == 0:
            L.vdl2gpu_destroy(h)
        return rc

    for mp in (lo, lo + 12345, 1 << 27 if sdrclk == 22 else 1 << 31, (1 << 64) - 1):
        assert create(mp) == -1, mp                                         # VDL2GPU_EINVAL
    if not torch.cuda.is_available():
        assert create(lo - 1) == -5                                         # VDL2GPU_ENODEV: past the check, at the device


def _k1_lds(rate, sdrclk):
    """dynamic LDS of the general channeliser k1_channelise (vdl2gpu.hip: k1_smem_bytes)"""
    L, maxwin = rate // 25000, (sdrclk + 20) // 21
    return ((L + maxwin) * 8 + 32 * maxwin) * 8


@pytest.mark.parametrize("rate,sdrclk,ok", [
    (25_700_000, 0, True), (25_725_000, 0, False),          # the default SDRCLK: the ceiling rate include/vdl2gpu.h states
    (2_000_000, 10416, True), (2_000_000, 10417, False),    # 2 MS/s with a custom SDRCLK: 10416 takes exactly 160 KiB
    (100_000, 10731, True), (100_000, 10732, False),
    (2_000_000, 1_000_000, False), (4_000_000_000, 0, False),
])
def test_create_rejects_what_the_channeliser_cannot_launch(built, rate, sdrclk, ok):
    """k1_channelise holds the LO table and a pass's input windows in dynamic LDS, which grows with the rate and SDRCLK; a
    gfx950 workgroup may have 160 KiB.  vdl2gpu_create refuses a pair above that before any device call (VDL2GPU_EINVAL on any
    machine) instead of failing at the first push.  A pair at or below it passes the check: a handle on a GPU, ENODEV without one."""
    import torch
    from vdlm2dec_amd import lib
    clk = sdrclk or rate // 4000
    assert (_k1_lds(rate, clk) <= 160 * 1024) == ok
    if ok and rate == 2_000_000:
        assert _k1_lds(rate, clk) == 160 * 1024
    L = lib.load()
    chan = (lib.ChanT * 1)(lib.ChanT(0, 136_975_000, 0))
    cfg = lib.ConfigT(struct_size=C.sizeof(lib.ConfigT), sdrinrate=rate, sdrclk=sdrclk, fmt=1, nbch=1, nstreams=1,
                      chan=chan, max_push=1 << 16)
    h = C.c_void_p()
    rc = L.vdl2gpu_create(C.byref(cfg), C.byref(h))
    if rc == 0:
        L.vdl2gpu_destroy(h)
    if not ok:
        assert rc == -1                                                     # VDL2GPU_EINVAL
    else:
        assert rc == (0 if torch.cuda.is_available() else -5)               # a handle, or VDL2GPU_ENODEV: past the check
