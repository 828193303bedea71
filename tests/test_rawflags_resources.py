"""What the compiler made of the four kernels VDL2GPU_F_RAW_FLAGS adds (csrc/vdl2gpu_rawflags.hip, a translation unit of its own with a
resource record of its own): listed there and in no other record, no spills, no scratch, at least the occupancy of the k4_frames_all*
sibling, at most its LDS + 256 bytes (the marks), and LDS never what limits workgroups per CU."""
import os

import pytest

from test_allframes_resources import _read, _z, allres  # noqa: F401  (the record's reader; the fixture: kernel_resources_allframes.txt)
from test_build_resources import resources  # noqa: F401  (the fixture: kernel_resources.txt as build_hip() wrote it)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = {"k4_frames_raw": "k4_frames_all", "k4_frames_raw_rep": "k4_frames_all_rep", "k4_frames_raw_fb": "k4_frames_all_fb",
         "k4_frames_raw_rep_fb": "k4_frames_all_rep_fb"}
LDS_PER_CU = 163840         # gfx950
SIMDS = 4


@pytest.fixture(scope="module")
def rawres(built):
    return _read(os.path.join(ROOT, "vdlm2dec_amd", "kernel_resources_rawflags.txt"))


def test_the_four_kernels_are_listed_in_their_own_record(rawres, allres, resources):  # noqa: F811
    assert set(rawres) == {_z(k) for k in PAIRS}
    assert not any("k4_frames_raw" in k for k in list(resources) + list(allres))       # the other records keep their sets of names
    committed = _read(os.path.join(ROOT, "profiles", "r23_kernel_resources_rawflags.txt"))
    assert committed == rawres                                                          # the committed copy is this build's


@pytest.mark.parametrize("kernel", sorted(PAIRS))
def test_no_spills_the_siblings_occupancy_and_lds(rawres, allres, kernel):  # noqa: F811
    r, sib = rawres[_z(kernel)], allres[_z(PAIRS[kernel])]
    assert r["VGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] == 0
    assert r["Occupancy [waves/SIMD]"] >= sib["Occupancy [waves/SIMD]"]
    assert r["LDS Size [bytes/block]"] <= sib["LDS Size [bytes/block]"] + 256
    # one wavefront a workgroup: `occupancy` of them on each SIMD must find room in the CU's LDS
    assert LDS_PER_CU // r["LDS Size [bytes/block]"] >= SIMDS * r["Occupancy [waves/SIMD]"]
