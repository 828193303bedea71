"""What the compiler made of the channeliser for VDL2GPU_FMT_CS8 (4) and VDL2GPU_FMT_S16R (5): k1_fast's counted waits rest on one
load instruction per sample and on five wavefronts per SIMD (K1F_WAVES_OF), neither of which a parity test notices."""
import os
import subprocess

import pytest

from test_build_resources import resources  # noqa: F401  (the fixture: kernel_resources.txt as build_hip() wrote it)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("fmt", [4, 5])
def test_k1_fast_registers(resources, fmt):  # noqa: F811
    r = resources[f"_Z7k1_fastILi{fmt}EEv8K1Params"]
    assert r["VGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] == 0
    assert r["VGPRs"] <= 96 and r["Occupancy [waves/SIMD]"] >= 5
    assert r["LDS Size [bytes/block]"] * 2 * 5 <= 160 * 1024           # two wavefronts per workgroup


@pytest.mark.parametrize("fmt", [4, 5])
def test_the_other_channelisers_are_listed_and_use_no_scratch(resources, fmt):  # noqa: F811
    for k in (f"_Z5k1_ppILi{fmt}EEv9K1PParams", f"_Z13k1_channeliseILi{fmt}EEv8K1Params"):
        assert k in resources, k
        assert resources[k]["VGPRs Spill"] == 0 and resources[k]["ScratchSize [bytes/lane]"] == 0, k
    assert resources[f"_Z5k1_ppILi{fmt}EEv9K1PParams"]["Occupancy [waves/SIMD]"] >= 6      # __launch_bounds__(K1P_THREADS, 6)


def _body(text, kern):
    start = next(i for i, ln in enumerate(text) if ln.startswith(kern + ":"))
    end = next(i for i in range(start, len(text)) if text[i].startswith(".Lfunc_end"))
    return [ln.strip() for ln in text[start:end]]


def test_k1_fast_issues_one_load_per_sample(tmp_path):
    """The ISA: cs8 and s16r issue exactly as many global loads as cu8 (6 per iteration and 6 in front of the loop for the samples,
    the rest the LO values), cs8 with cu8's 16-bit load, s16r with the sign-extending one -- no second load and no extra ALU
    operation between a load and its convert."""
    import __graft_entry__ as g
    asm = tmp_path / "vdl2gpu.s"
    flags = [f for f in g.HIPCC_FLAGS if f not in ("-shared", "-fPIC") and not f.startswith("-Wl,")]
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + flags + ["-S", "--cuda-device-only", "-w",
                           os.path.join(g.CSRC, "vdl2gpu.hip"), "-o", str(asm)])
    text = asm.read_text().splitlines()
    loads = {}
    for fmt in (0, 4, 5):
        body = _body(text, f"_Z7k1_fastILi{fmt}EEv8K1Params")
        loads[fmt] = [ln.split()[0] for ln in body if ln.startswith("global_load_")]
    assert len(loads[0]) > 0
    assert len(loads[4]) == len(loads[0]) and len(loads[5]) == len(loads[0])
    n16 = loads[0].count("global_load_ushort")
    assert n16 == 12                                                        # 2 x 3 in front of the loop, 2 x 3 inside it
    assert loads[4].count("global_load_ushort") == n16
    assert loads[5].count("global_load_sshort") == n16 and "global_load_ushort" not in loads[5]
    # s16r: the register is the sample as an int; converting it is one instruction per sample and nothing else
    body5 = _body(text, "_Z7k1_fastILi5EEv8K1Params")
    assert not [ln for ln in body5 if ln.startswith("v_bfe_i32") or "sdwa" in ln]
    assert sum(ln.startswith("v_cvt_f32_i32_e32") for ln in body5) >= 6
    body4 = _body(text, "_Z7k1_fastILi4EEv8K1Params")
    # cs8: each byte sign-extended by the convert itself (SDWA), as cs16's half-words are
    assert sum("v_cvt_f32_i32_sdwa" in ln and "sext(" in ln for ln in body4) == 12
