"""The development counters have one table (enum K2Dbg and enum K2aStage, csrc/vdl2gpu_types.h).  The tests and scripts take their slots
from vdlm2dec_amd/lib.py, which restates the table for Python: here the header is parsed and the two must be equal, name by name."""
import os
import re

from vdlm2dec_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TYPES = os.path.join(ROOT, "vdlm2dec_amd", "csrc", "vdl2gpu_types.h")


def _enum(name, prefix):
    """{enumerator without prefix: value} of `enum name { ... };`, counting on from the last `= number` like the compiler does"""
    src = open(TYPES).read()
    bodies = re.findall(r"^enum %s \{(.*?)\};" % name, src, re.M | re.S)
    assert len(bodies) == 1, name
    body = re.sub(r"/\*.*?\*/", "", bodies[0], flags=re.S)
    out, nxt = {}, 0
    for item in (x.strip() for x in body.split(",")):
        if not item:
            continue
        m = re.fullmatch(r"(\w+)(?:\s*=\s*(\d+))?", item)
        assert m and m.group(1).startswith(prefix), item
        nxt = int(m.group(2)) if m.group(2) else nxt
        out[m.group(1)[len(prefix):]] = nxt
        nxt += 1
    return out


def test_the_counter_slots_of_lib_are_the_header_s():
    want = _enum("K2Dbg", "K2_DBG_")
    assert len(set(want.values())) == len(want)
    assert lib.DBG == want
    src = open(TYPES).read()
    assert sorted(int(x) for x in re.findall(r"^#define VDL2_DBG_WORDS (\d+)", src, re.M)) == [lib.DBG_WORDS, lib.DBG_WORDS_TEST]
    assert max(v for k, v in want.items() if not k.startswith(("ESC_", "INV_", "CHK_"))) < lib.DBG_WORDS <= want["ESC_REG"]
    assert max(want.values()) < lib.DBG_WORDS_TEST


def test_the_stage_names_of_lib_are_the_header_s():
    want = _enum("K2aStage", "K2A_ST_")
    assert want.pop("SLOTS") == 16
    assert sorted(want.values()) == list(range(16))
    assert list(lib.DBG_STAGES) == [k.lower() for k, _ in sorted(want.items(), key=lambda kv: kv[1])]
    assert lib.DBG["REGION_STAGE0"] - lib.DBG["PROBE_STAGE0"] == 16 and lib.DBG["ESC_REG"] - lib.DBG["REGION_STAGE0"] == 16
