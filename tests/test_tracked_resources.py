"""What the compiler made of the kernels VDL2GPU_F_TRACKED adds (csrc/vdl2gpu_tracked.hip, a translation unit of its own with a
resource record of its own): listed there and in no other record, the committed copy is this build's, no spills and no scratch in
the slicing kernel and the export, no scratch and no vector spill in the block kernels, and the slicing kernel's LDS (a segment's span with its padding, the burst's
table indices) is never what limits workgroups per CU."""
import os

import pytest

from test_allframes_resources import _read, _z, allres  # noqa: F401  (the record's reader; the fixture: kernel_resources_allframes.txt)
from test_build_resources import resources  # noqa: F401  (the fixture: kernel_resources.txt as build_hip() wrote it)
from test_rawflags_resources import rawres  # noqa: F401
from test_symclk_resources import clkres  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("k_tracked_rows", "k_export_tracked")
BLOCK_KERNELS = tuple("k4_frames_trk" + m + r + f + "8K4Params" for m in ("", "_all", "_raw") for r in ("", "_rep") for f in ("", "_fb"))
LDS_PER_CU = 163840         # gfx950
VGPRS_PER_SIMD = 512


@pytest.fixture(scope="module")
def trkres(built):
    return _read(os.path.join(ROOT, "vdlm2dec_amd", "kernel_resources_tracked.txt"))


def _line(res, kernel):
    hit = [k for k in res if kernel in k]
    assert len(hit) == 1, (kernel, hit)
    return res[hit[0]]


def test_the_kernels_are_listed_in_their_own_record(trkres, clkres, rawres, allres, resources):  # noqa: F811
    assert len(trkres) == len(KERNELS) + len(BLOCK_KERNELS) == 14
    assert all(any(k in name for name in trkres) for k in KERNELS + BLOCK_KERNELS)
    others = list(resources) + list(allres) + list(rawres) + list(clkres)
    assert not any("tracked" in k or "_trk" in k for k in others)      # the other records keep their sets of names
    committed = _read(os.path.join(ROOT, "profiles", "r25_kernel_resources_tracked.txt"))
    assert committed == trkres                                          # the committed copy is this build's


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_spills_no_scratch(trkres, kernel):
    r = _line(trkres, kernel)
    assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] == 0


@pytest.mark.parametrize("kernel", BLOCK_KERNELS)
def test_block_kernels_no_scratch(trkres, kernel):
    # (scalar registers parked in vector lanes they have, as every k4_frames* has: profiles/r22_kernel_resources.txt)
    r = _line(trkres, kernel)
    assert r["VGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] == 0


def test_the_slicing_kernel_lds(trkres):
    r = _line(trkres, "k_tracked_rows")
    # 2066 samples with a word of padding behind every eight (2324 float2), 22 x 256 indices of two bytes, the taps and the atanf table
    # (72 + 40 floats), 4 x 4 partial sums, the four phases of the symbol in front of the segment
    want = 2324 * 8 + 22 * 256 * 2 + (72 + 40) * 4 + 4 * 4 * 4 + 4 * 4
    assert want <= r["LDS Size [bytes/block]"] <= want + 16
    # four wavefronts a workgroup, one on each SIMD: as many workgroups as the registers allow wavefronts on a SIMD must find room in LDS
    by_regs = min(8, VGPRS_PER_SIMD // (-(-(r["VGPRs"] + r["AGPRs"]) // 8) * 8))
    assert LDS_PER_CU // r["LDS Size [bytes/block]"] >= by_regs
    assert _line(trkres, "k_export_tracked")["LDS Size [bytes/block]"] == 0
