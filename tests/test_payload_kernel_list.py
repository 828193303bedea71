"""The payload kernels are defined from one list (K2D_PAYLOAD_KERNELS, vdl2gpu_resolve.h): the build has exactly the sixteen kernels it
had when they were written out one by one, each once, and every line's flag columns are the ones its name says."""
import os
import re

from test_build_resources import resources  # noqa: F401  (the fixture: kernel_resources.txt as build_hip() wrote it)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAIN = ["k2d_payload", "k2d_payload_lev", "k2d_payload_soft", "k2d_payload_lev_soft",
         "k2d_payload_car", "k2d_payload_lev_car", "k2d_payload_soft_car", "k2d_payload_lev_soft_car"]
SIXTEEN = sorted([f"_Z{len(k)}{k}8K2Params" for k in PLAIN] + [f"_Z{len(k) + 3}{k}_fb8K2ParamsP12vdl2gpu_fb_t" for k in PLAIN])


def test_the_build_has_the_sixteen_payload_kernels_each_once(resources):  # noqa: F811
    listed = [ln.split(" ", 1)[0] for ln in open(os.path.join(ROOT, "vdlm2dec_amd", "kernel_resources.txt")) if re.match(r"_Z\d+k2d_payload", ln)]
    assert sorted(listed) == SIXTEEN
    assert sorted(k for k in resources if re.match(r"_Z\d+k2d_payload", k)) == SIXTEEN


def test_every_line_of_the_list_has_the_flags_of_its_name():
    src = open(os.path.join(ROOT, "vdlm2dec_amd", "csrc", "vdl2gpu_resolve.h")).read()
    rows = re.findall(r"^\tX\((k2d_payload\w*), (\w+), ([01]), ([01]), ([01]), ([01])\)", src, re.M)
    assert len(rows) == 16 and len({r[0] for r in rows}) == 16
    for name, waves, lev, soft, car, fb in rows:
        assert name == "k2d_payload" + "_lev" * int(lev) + "_soft" * int(soft) + "_car" * int(car) + "_fb" * int(fb), name
        assert waves == ("K2D_WAVES" if name == "k2d_payload" else "4"), name
