"""What the compiler made of the four kernels VDL2GPU_F_ALL_FRAMES adds (csrc/vdl2gpu_allframes.hip, a translation unit of its own with
a resource record of its own): listed there and nowhere else, no spills, no scratch, at least the occupancy of the sibling without ALL and
exactly its LDS."""
import os

import pytest

from test_build_resources import resources  # noqa: F401  (the fixture: kernel_resources.txt as build_hip() wrote it)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = {"k4_frames_all": "k4_frames", "k4_frames_all_rep": "k4_frames_rep", "k4_frames_all_fb": "k4_frames_fb",
         "k4_frames_all_rep_fb": "k4_frames_rep_fb"}


def _read(path):
    out = {}
    for ln in open(path):
        if ln.startswith("#") or not ln.strip():
            continue
        name, rest = ln.rstrip("\n").split(" ", 1)
        out[name] = {k.strip(): int(v) for k, v in (f.rsplit("=", 1) for f in _fields(rest))}
    return out


def _fields(rest):
    """'A=1 B C [x]=2' -> ['A=1', 'B C [x]=2']: a field's name may hold blanks, its value is an integer"""
    out, cur = [], []
    for tok in rest.split(" "):
        cur.append(tok)
        if "=" in tok and tok.rsplit("=", 1)[1].lstrip("-").isdigit():
            out.append(" ".join(cur))
            cur = []
    assert not cur, rest
    return out


@pytest.fixture(scope="module")
def allres(built):
    return _read(os.path.join(ROOT, "vdlm2dec_amd", "kernel_resources_allframes.txt"))


def _z(name):
    return f"_Z{len(name)}{name}8K4Params"


def test_the_four_kernels_are_listed_in_their_own_record(allres, resources):  # noqa: F811
    assert set(allres) == {_z(k) for k in PAIRS}
    assert not any("k4_frames_all" in k for k in resources)         # the library's record keeps its set of names
    committed = _read(os.path.join(ROOT, "profiles", "r22_kernel_resources_allframes.txt"))
    assert committed == allres                                       # the committed copy is this build's


@pytest.mark.parametrize("kernel", sorted(PAIRS))
def test_no_spills_the_siblings_occupancy_and_lds(allres, resources, kernel):  # noqa: F811
    r, sib = allres[_z(kernel)], resources[_z(PAIRS[kernel])]
    assert r["VGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] == 0
    assert r["Occupancy [waves/SIMD]"] >= sib["Occupancy [waves/SIMD]"]
    assert r["LDS Size [bytes/block]"] == sib["LDS Size [bytes/block]"]
