"""The two 2-byte formats receivers deliver natively, VDL2GPU_FMT_CS8 (interleaved signed 8-bit I,Q) and VDL2GPU_FMT_S16R (real
signed 16-bit), as far as a machine without a GPU can see them: the C ABI accepts them before any device call, the Python tables
mirror the header, the synthesiser writes them, and the CPU restatement of the reference decodes every burst of the streams the
GPU tests (tests/test_gpu_formats.py) feed -- so that none of those can pass for want of something to compare."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import scenarios as S
from vdlm2dec_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENODEV = -1, -5


def _create(fmt, flags=0):
    from vdlm2dec_amd import lib
    L = lib.load()
    chan = (lib.ChanT * 1)(lib.ChanT(0, 136_975_000, -50_000))
    cfg = lib.ConfigT(struct_size=C.sizeof(lib.ConfigT), sdrinrate=2_000_000, fmt=fmt, nbch=1, nstreams=1, chan=chan,
                      max_push=32768, flags=flags)
    h = C.c_void_p()
    rc = L.vdl2gpu_create(C.byref(cfg), C.byref(h))
    if rc == 0:
        L.vdl2gpu_destroy(h)
    return rc


def _header_enum():
    hdr = open(os.path.join(ROOT, "include", "vdl2gpu.h")).read()
    return hdr, {k: int(v) for k, v in re.findall(r"\b(VDL2GPU_FMT_[A-Z0-9]+)\s*=\s*(\d+)", hdr)}


@pytest.mark.parametrize("fmt", [4, 5])
def test_create_accepts_the_new_formats(built, fmt):
    rc = _create(fmt)
    assert rc != EINVAL                     # a handle, or VDL2GPU_ENODEV on a machine without a GPU
    assert rc in (0, ENODEV)


@pytest.mark.parametrize("fmt", [6, -1, 7, 255])
def test_create_rejects_unknown_formats(built, fmt):
    assert _create(fmt) == EINVAL           # whatever the machine: before any device call


@pytest.mark.parametrize("fmt", [4, 5])
def test_rtl_quirk_stays_cu8_only(built, fmt):
    from vdlm2dec_amd import lib
    assert _create(fmt, lib.F_RTL_QUIRK) == EINVAL
    assert _create(0, lib.F_RTL_QUIRK) != EINVAL


def test_python_tables_mirror_the_header():
    from vdlm2dec_amd import lib
    hdr, enum = _header_enum()
    assert enum == {"VDL2GPU_FMT_CU8": 0, "VDL2GPU_FMT_CS16": 1, "VDL2GPU_FMT_CF32": 2, "VDL2GPU_FMT_F32R": 3,
                    "VDL2GPU_FMT_CS8": 4, "VDL2GPU_FMT_S16R": 5}
    name = {"cu8": "CU8", "cs16": "CS16", "cf32": "CF32", "f32": "F32R", "cs8": "CS8", "s16": "S16R"}
    assert lib.FMT == {k: enum["VDL2GPU_FMT_" + v] for k, v in name.items()}
    assert lib.SAMPLE_BYTES == {"cu8": 2, "cs16": 4, "cf32": 8, "f32": 4, "cs8": 2, "s16": 2}
    assert re.search(r"#define\s+VDL2GPU_HAVE_FMT_CS8_S16R\s+1\b", hdr)
    assert re.search(r"#define\s+VDL2GPU_ABI_VERSION\s+6\b", hdr)      # nothing existing changes meaning
    # the byte sizes the library itself uses (fmt_bytes): one case per enumerator
    src = open(os.path.join(ROOT, "vdlm2dec_amd", "csrc", "vdl2gpu.hip")).read()
    body = src[src.index("static size_t fmt_bytes(int fmt)"):]
    body = body[:body.index("default:")]
    sizes = {k: int(v) for k, v in re.findall(r"case (VDL2GPU_FMT_[A-Z0-9]+): return (\d+);", body)}
    assert sizes == {"VDL2GPU_FMT_" + v: lib.SAMPLE_BYTES[k] for k, v in name.items()}


def test_quantise_cs8():
    rng = np.random.default_rng(4)
    x = (rng.normal(0, 60, 4096) + 1j * rng.normal(0, 60, 4096)).astype(np.complex64)
    x[:4] = [300 - 300j, -300 + 300j, 127.4 - 128.6j, 0.49 - 0.51j]          # both rails, and rounding
    q = synth.quantise(x, "cs8")
    assert q.dtype == np.int8 and q.shape == (2 * len(x),)
    assert q[:8].tolist() == [127, -128, -128, 127, 127, -128, 0, -1]
    assert np.array_equal(q[0::2], np.clip(np.rint(x.real), -128, 127).astype(np.int8))
    assert np.array_equal(q[1::2], np.clip(np.rint(x.imag), -128, 127).astype(np.int8))
    assert q.min() == -128 and q.max() == 127
    # not cu8 with the offset taken out: the 127.37 is cu8's alone
    cu8 = synth.quantise(x, "cu8").astype(np.int32) - 127
    assert not np.array_equal(cu8, q.astype(np.int32))


def test_quantise_s16():
    rng = np.random.default_rng(5)
    x = (rng.normal(0, 40, 4096) + 1j * rng.normal(0, 40, 4096)).astype(np.complex64)
    x[:3] = [200 + 5j, -200 - 5j, 127.998 + 0j]                             # 256 * 200 is beyond both rails
    q = synth.quantise(x, "s16")
    assert q.dtype == np.int16 and q.shape == (len(x),)
    assert q[:3].tolist() == [32767, -32768, 32767]
    assert np.array_equal(q, synth.quantise(x, "cs16")[0::2])
    assert np.array_equal(q, np.clip(np.rint(256.0 * x.real), -32768, 32767).astype(np.int16))


@pytest.mark.parametrize("fmt,dtype", [("cs8", np.int8), ("s16", np.int16)])
def test_synth_cli_writes_two_bytes_a_sample(tmp_path, fmt, dtype):
    import json
    iq, truth = str(tmp_path / ("x." + fmt)), str(tmp_path / "x.json")
    r = subprocess.run([sys.executable, "-m", "vdlm2dec_amd.synth", iq, "--fmt", fmt, "--seconds", "0.1", "--fo", "100000", "250000",
                        "--seed", "5", "--truth", truth], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    t = json.load(open(truth))
    assert t["fmt"] == fmt and os.path.getsize(iq) == 2 * t["nsamples"]
    assert np.fromfile(iq, dtype).size == (2 if fmt == "cs8" else 1) * t["nsamples"]


# what the GPU tests feed: (scenario, new format, the float twin's format, bursts sent)
def _twin(raw, fmt):
    return raw.astype(np.float32), {"cs8": "cf32", "s16": "f32"}[fmt]


@pytest.mark.parametrize("name,fmt,sent", [("regimes", "cs8", 12), ("eight", "cs8", 16), ("air5m", "s16", 16)])
def test_oracle_decodes_every_burst_of_the_gpu_tests_inputs(oracle, name, fmt, sent):
    spec = {"regimes": S.regimes, "eight": S.eight_channels,
            "air5m": lambda: S.eight_channels(rate=5_000_000, fo=S.FO8_AIR_5MS)}[name]()
    assert len(spec.bursts) == sent
    tw, tfmt = _twin(synth.synth_stream(spec, fmt), fmt)
    got = oracle.run_oracle(tw, tfmt, spec.rate, spec.fo, S.FC)
    assert len(got) == sent
    assert sorted(b.chn for b in got) == sorted(b.chan for b in spec.bursts)
