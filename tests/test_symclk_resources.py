"""What the compiler made of the two kernels VDL2GPU_F_SYMCLK adds (csrc/vdl2gpu_symclk.hip, a translation unit of its own with a
resource record of its own): listed there and in no other record, the committed copy is this build's, no spills, no scratch, and the
sums kernel's LDS (the staged span with its padding, and the wavefronts' partial sums) never what limits workgroups per CU."""
import os

import pytest

from test_allframes_resources import _read, _z, allres  # noqa: F401  (the record's reader; the fixture: kernel_resources_allframes.txt)
from test_build_resources import resources  # noqa: F401  (the fixture: kernel_resources.txt as build_hip() wrote it)
from test_rawflags_resources import rawres  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("k_symclk_sums", "k_export_symclk")
LDS_PER_CU = 163840         # gfx950
SIMDS = 4


@pytest.fixture(scope="module")
def clkres(built):
    return _read(os.path.join(ROOT, "vdlm2dec_amd", "kernel_resources_symclk.txt"))


def _line(res, kernel):
    hit = [k for k in res if kernel in k]
    assert len(hit) == 1, (kernel, hit)
    return res[hit[0]]


def test_the_two_kernels_are_listed_in_their_own_record(clkres, rawres, allres, resources):  # noqa: F811
    assert len(clkres) == 2 and all(any(k in name for name in clkres) for k in KERNELS)
    assert not any("symclk" in k for k in list(resources) + list(allres) + list(rawres))      # the other records keep their sets of names
    committed = _read(os.path.join(ROOT, "profiles", "r24_kernel_resources_symclk.txt"))
    assert committed == clkres                                                                 # the committed copy is this build's


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_spills_no_scratch(clkres, kernel):
    r = _line(clkres, kernel)
    assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] == 0


def test_the_sums_kernel_lds(clkres):
    r = _line(clkres, "k_symclk_sums")
    # 2064 samples with a word of padding behind every eight (2321 float2) and 4 x 8 partial sums
    assert 2321 * 8 + 4 * 8 * 4 <= r["LDS Size [bytes/block]"] <= 2321 * 8 + 4 * 8 * 4 + 16      # (the second array is aligned)
    # four wavefronts a workgroup, one on each SIMD: `occupancy` workgroups must find room in the CU's LDS
    assert LDS_PER_CU // r["LDS Size [bytes/block]"] >= r["Occupancy [waves/SIMD]"]
    assert _line(clkres, "k_export_symclk")["LDS Size [bytes/block]"] == 0
