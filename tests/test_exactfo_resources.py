"""What the compiler made of the K1 kernels with the rotation of VDL2GPU_F_EXACT_FO at their dump -- k1_fast<FMT, true>,
k1_pp<FMT, true>, k1_channelise<FMT, GLO, true> for all six formats: listed, no spills, no scratch -- and of the kernels a handle
without the flag runs: under their old names, with the registers and LDS profiles/r11_kernel_resources.txt recorded for them."""
import os

import pytest

from test_build_resources import resources  # noqa: F401  (the fixture: kernel_resources.txt as build_hip() wrote it)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FMTS = range(6)
FIGURES = ("VGPRs", "AGPRs", "TotalSGPRs", "LDS Size [bytes/block]", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]",
           "VGPRs Spill", "SGPRs Spill")


def _rot(fmt):
    return ([f"_Z7k1_fastILi{fmt}ELb1EEv8K1Params5K1Rot", f"_Z5k1_ppILi{fmt}ELb1EEv9K1PParams5K1Rot"]
            + [f"_Z13k1_channeliseILi{fmt}ELb{g}ELb1EEv8K1Params5K1Rot" for g in (0, 1)])


@pytest.mark.parametrize("fmt", FMTS)
def test_rotating_kernels_are_listed_and_use_no_scratch(resources, fmt):  # noqa: F811
    for k in _rot(fmt):
        r = resources[k]
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] == 0, k
    fast, pp = (resources[k] for k in _rot(fmt)[:2])
    assert fast["Occupancy [waves/SIMD]"] >= 4          # the rotating k1_fast is built for four wavefronts per SIMD (K1F_ROT_WAVES)
    assert pp["Occupancy [waves/SIMD]"] >= 6 and pp["LDS Size [bytes/block]"] == 50304
    assert fast["LDS Size [bytes/block]"] == 13060


def test_kernels_without_the_flag_are_what_they_were(resources):  # noqa: F811
    rec = {k: v for k, v in _recorded_fields().items() if k.startswith(("_Z7k1_fast", "_Z5k1_pp", "_Z13k1_channelise"))}
    assert len(rec) == 24
    for k, want in rec.items():
        got = resources[k]
        assert {f: got[f] for f in want} == want, k


def _recorded_fields():
    """name -> {figure: value} of the recorded file, whose lines are 'name field=value field=value ..' with spaces inside field names"""
    out = {}
    for ln in open(os.path.join(ROOT, "profiles", "r11_kernel_resources.txt")):
        if ln.startswith("#") or not ln.strip():
            continue
        name, rest = ln.rstrip("\n").split(" ", 1)
        vals = {}
        for f in FIGURES:
            i = rest.find(f + "=")
            while i > 0 and rest[i - 1] != " ":         # 'VGPRs=' also ends 'TotalSGPRs='? no, but 'VGPRs Spill' / 'VGPRs' share a head
                i = rest.find(f + "=", i + 1)
            if i >= 0:
                vals[f] = int(rest[i + len(f) + 1:].split(" ", 1)[0])
        out[name] = vals
    return out
