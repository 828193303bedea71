"""What the compiler made of k1_channelise<FMT, true>, the general channeliser with its LO table in global memory (rates off the
25 kHz grid whose table does not fit LDS): listed for all six formats, no spills, no scratch -- in the build's resource report and
in the ISA itself -- and the LDS kernels beside them keep their names."""
import os
import subprocess

import pytest

from test_build_resources import resources  # noqa: F401  (the fixture: kernel_resources.txt as build_hip() wrote it)
from test_fmt_resources import _body

FMTS = range(6)


def _glo(fmt):
    return f"_Z13k1_channeliseILi{fmt}ELb1EEv8K1Params"


@pytest.mark.parametrize("fmt", FMTS)
def test_global_table_variant_is_listed_and_uses_no_scratch(resources, fmt):  # noqa: F811
    r = resources[_glo(fmt)]
    assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] == 0
    assert r["LDS Size [bytes/block]"] == 0                         # all of its LDS is dynamic: the launch sizes it
    assert r["Occupancy [waves/SIMD]"] >= 4                         # 256 threads: a workgroup is one wavefront per SIMD
    assert f"_Z13k1_channeliseILi{fmt}EEv8K1Params" in resources    # the LDS kernel under its old name


def test_global_table_variant_isa(tmp_path):
    """The ISA of the six instantiations: no scratch instruction and a zero private segment; the LO values arrive by vector loads
    of 8 bytes a lane (global_load_dwordx2) and leave LDS as 8-byte reads; stores to memory are vector stores only."""
    import __graft_entry__ as g
    asm = tmp_path / "vdl2gpu.s"
    flags = [f for f in g.HIPCC_FLAGS if f not in ("-shared", "-fPIC") and not f.startswith("-Wl,")]
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + flags + ["-S", "--cuda-device-only", "-w",
                           os.path.join(g.CSRC, "vdl2gpu.hip"), "-o", str(asm)])
    text = asm.read_text().splitlines()
    for fmt in FMTS:
        body = _body(text, _glo(fmt))
        ops = [ln.split()[0] for ln in body if ln and not ln.startswith((".", ";", "//")) and not ln.endswith(":")]
        assert not [o for o in ops if o.startswith(("scratch_", "buffer_"))], fmt
        assert "global_load_dwordx2" in ops, fmt
        stores = {o for o in ops if "store" in o}
        assert stores and all(o.startswith("global_store_") for o in stores), (fmt, stores)
        meta = next(i for i, ln in enumerate(text) if ln.strip() == f".amdhsa_kernel {_glo(fmt)}")
        seg = next(ln for ln in text[meta:meta + 80] if ".amdhsa_private_segment_fixed_size" in ln)
        assert seg.split()[-1] == "0", (fmt, seg)
