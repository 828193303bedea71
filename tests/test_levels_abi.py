"""VDL2GPU_F_LEVELS without a GPU: the header, the ctypes mirror of vdl2gpu_level_t, the handle's refusal without a device, and
the numpy restatement of the definitions (tests/levels_ref.py) against a brute-force loop."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import levels_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "vdl2gpu.h")


def test_header_declares_levels():
    text = open(HDR).read()
    assert re.search(r"#define VDL2GPU_F_LEVELS 128u", text)
    assert re.search(r"#define VDL2GPU_HAVE_LEVELS 1", text)
    assert "} vdl2gpu_level_t;" in text
    assert re.search(r"int vdl2gpu_poll_levels\(vdl2gpu_t \*h, vdl2gpu_burst_t \*out, vdl2gpu_level_t \*lv, int max\);", text)
    assert re.search(r"int vdl2gpu_poll_levels_ready\(vdl2gpu_t \*h, vdl2gpu_burst_t \*out, vdl2gpu_level_t \*lv, int max\);", text)
    assert re.search(r"#define VDL2GPU_ABI_VERSION 6\b", text)


def test_level_layout_matches_the_compiler(tmp_path):
    from vdlm2dec_amd import lib
    assert lib.F_LEVELS == 128
    fields = [f for f, _ in lib.LevelT._fields_]
    src = tmp_path / "lv.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vdl2gpu.h"\nint main(void){printf("%zu %zu", sizeof(vdl2gpu_level_t), _Alignof(vdl2gpu_level_t));'
                   + "".join(f'printf(" %zu", offsetof(vdl2gpu_level_t, {f}));' for f in fields) + 'printf("\\n");return 0;}\n')
    exe = tmp_path / "lv"
    subprocess.check_call(["cc", "-std=c11", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got[0] == C.sizeof(lib.LevelT) == 40
    assert got[1] == C.alignment(lib.LevelT) == 8
    assert got[2:] == [getattr(lib.LevelT, f).offset for f in fields]


def test_levels_handle_without_gpu_is_enodev():
    from vdlm2dec_amd import lib
    L = lib.load()
    try:
        import torch
        if torch.cuda.is_available():
            pytest.skip("a GPU is present: tests/test_gpu_levels.py covers the handle")
    except ImportError:
        pass
    chan = (lib.ChanT * 1)(lib.ChanT(0, 136975000, 100000))
    cfg = lib.ConfigT()
    cfg.struct_size = C.sizeof(lib.ConfigT)
    cfg.sdrinrate, cfg.fmt, cfg.nbch, cfg.nstreams, cfg.chan, cfg.max_push = 2_000_000, 0, 1, 1, chan, 1 << 20
    cfg.flags = lib.F_LEVELS
    h = C.c_void_p()
    assert L.vdl2gpu_create(C.byref(cfg), C.byref(h)) == -5     # VDL2GPU_ENODEV, like any other handle
    assert L.vdl2gpu_poll_levels(None, None, None, 0) == -1
    assert L.vdl2gpu_poll_levels_ready(None, None, None, 0) == -1


def _brute(x, mflt, first, nsym, c):
    def S(n, cc):
        acc = 0j
        j = 0
        while cc + 4 * j <= 64:
            acc += complex(x[n - 16 + j]) * float(mflt[cc + 4 * j])
            j += 1
        return acc
    sig = sum(abs(S(first + 8 * k, c)) ** 2 for k in range(nsym)) / nsym
    means = []
    for b in range(8):
        if first - 512 - 8 * (32 * b + 31) - 16 < 0:
            continue
        means.append(sum(abs(S(first - 512 - 8 * i, 0)) ** 2 for i in range(32 * b, 32 * b + 32)) / 32)
    means.sort()
    if not means:
        return sig, float("nan"), 0
    k = len(means)
    noise = means[k // 2] if k % 2 else 0.5 * (means[k // 2 - 1] + means[k // 2])
    return sig, noise, k


@pytest.mark.parametrize("first,nblocks", [(4000, 8), (2568, 8), (2567, 7), (1500, 3), (800, 1), (776, 1), (775, 0), (100, 0)])
def test_restatement_matches_brute_force(first, nblocks):
    rng = np.random.default_rng(first)
    x = (rng.standard_normal(6000) + 1j * rng.standard_normal(6000)) * rng.uniform(0.5, 3.0, 6000)
    mflt = R.mflt_taps()
    for c, nsym in ((0, 1), (1, 37), (3, 90), (2, 200)):
        want = _brute(x, mflt, first, nsym, c)
        got = R.levels(x, mflt, first, nsym, c)
        assert got[2] == want[2] == nblocks
        assert math.isclose(got[0], want[0], rel_tol=1e-12)
        if nblocks:
            assert math.isclose(got[1], want[1], rel_tol=1e-12)
        else:
            assert math.isnan(got[1]) and math.isnan(want[1])


def test_scale_k_reads_zero_dbfs_for_a_full_scale_tone():
    mflt = R.mflt_taps()
    for fmt, rate in (("cu8", 2_000_000), ("cs16", 10_000_000), ("cf32", 2_000_000)):
        x = np.full(400, R.FS[fmt], np.complex128)      # integrate-and-dump (an average) of a full-scale tone at the centre
        sig, _, _ = R.levels(x, mflt, 300, 5, 0)
        assert abs(10 * math.log10(sig / R.scale_k(fmt, rate, mflt))) < 1e-9
