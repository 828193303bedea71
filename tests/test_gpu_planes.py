"""Crafted 84 kS/s planes (tests/plane_craft.py) through the whole HIP path, judged by the oracle: sync words whose fit error sits on the
detector's threshold in some timing classes and past it in others, header soft bits exactly on 0.5, header words the (25,20) trellis has
to correct -- some of them into ANOTHER length --, geometry edges, and payload phases on the slicer's decision boundary.

At 100 kS/s, SDRCLK 42, one channel at Fo = 0 and cf32 input with every sample written twice the channeliser is an exact identity
(each dump window is two equal inputs, the LO is 1 + 0j), so the plane the scan sees is the crafted one bit for bit -- asserted -- and
every family x decode path must give the oracle's records, stamps, carrier estimates, candidates and header soft bits.  Whether the
inputs really sit on the edges they aim at is asserted on the CPU, against the oracle alone: tests/test_plane_craft.py.

How a marginal trigger is reached (probe, region scan, verify and repair, serial redo) is the design's business: nothing here looks at
`repairs` or `serial_redos`."""
import numpy as np
import pytest

import plane_craft as PC
import test_gpu_rates as TR
from vdlm2dec_amd import lib

pytestmark = pytest.mark.gpu

# decode path -> (Receiver arguments, VDL2GPU_REPAIR_ROUNDS or None, channeliser: None = k1_pp takes the whole periods, "general" = k1_channelise alone)
PATHS = {
    "default": (dict(), None, None),                                     # probe + regions + verify
    "fullscan": (dict(full_scan=True), None, None),
    "serial": (dict(serial=True), None, "general"),
    "noregion-r0": (dict(flags=lib.F_TEST_NOREGION), "0", None),        # region scan dropped (test build): verify finds the triggers, K2f redoes
    "noregion-r2": (dict(flags=lib.F_TEST_NOREGION), "2", "general"),   # ... two repair rounds: the second payload pass
}
SCANNING = ("default", "fullscan")          # the paths whose candidate tables must hold every trigger the chain took
HEADS = ("header", "header_words")


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _f32(v):
    return int(np.float32(v).view(np.uint32))


def _rx(n, kw, **more):
    from vdlm2dec_amd.demod import Receiver, plan_channels
    kw = dict(kw, **more)
    flags = kw.pop("flags", 0) | kw.pop("more_flags", 0)
    return Receiver(PC.RATE, plan_channels(PC.FC, PC.FO), fmt="cf32", sdrclk=PC.SDRCLK, max_push=n, keep_dec=True, flags=flags, **kw)


def _check_cands(j, cands):
    """every trigger the oracle's chain took on a case's sync word is in the scan's table with the detector's own four numbers"""
    table = {}
    for nrel, _, p2, p, e, f in cands.view(np.uint32).reshape(-1, 6).tolist():
        table.setdefault((p2, p, e, f), []).append(np.int32(np.uint32(nrel)).item() if nrel >= 1 << 31 else nrel)
    offs, n = None, 0
    for c in j.plane.cases:
        t = j.sync_trigger(c)
        if t is None:
            continue
        hit = table.get((_f32(t["p2err"]), _f32(t["perr"]), _f32(t["err"]), _f32(t["pfr"])))
        assert hit, (c.label, c.align, t["dec_index"], t["perr"], t["err"])
        here = {nrel - t["dec_index"] for nrel in hit}     # (without a noise floor equal cases have equal numbers: several instants)
        offs = here if offs is None else offs & here
        n += 1
    assert n > 0 and len(offs) == 1, offs      # ... each at its own instant (the table counts from the start of the push's planes)


def _check_heads(j, heads):
    mine = heads[heads["sc"] == 0]
    n = 0
    for t in j.triggers:
        if len(t["head"]) < 25:
            continue
        cand = mine[mine["nstar"] == t["dec_index"]]
        hit = [e for e in cand if np.array_equal(_bits(e["soft"]), _bits(t["head"])) and _bits(e["perr"]) == _f32(t["perr"])
               and _bits(e["err"]) == _f32(t["err"]) and e["clk0"] == t["clk"]]
        assert hit, (t["dec_index"], len(cand))
        n += 1
    assert n >= len(j.plane.cases) // 2


def _check_soft(j, got):
    import soft_ref as R
    clk = {t["dec_index"]: t["clk"] for t in j.triggers if t["accepted"] == 1}
    pn = R.pn_bits()
    want = {b.trig_dec: R.soft_block(j.dec, b.nbrow, b.nlbyte, b.df, b.trig_dec, clk[b.trig_dec], pn) for b in j.blocks}
    assert len(got) == len(want) >= 100
    half = 0
    for b in got:
        hard, rel = want[b.trig_dec]
        assert hard.tobytes() == b.data, b.trig_dec          # the model is the oracle's slicer ...
        assert b.soft is not None and np.array_equal(b.soft, rel), b.trig_dec
        half += int((rel[0, :44] == 0).sum())
    assert half >= 100        # ... and bytes with a soft bit on the boundary itself (reliability 0) are among them


@pytest.mark.timeout(180)
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("name", PC.FAMILIES)
def test_crafted_planes_equal_the_oracle(built, oracle, monkeypatch, name, path):
    kw, rounds, k1 = PATHS[path]
    if rounds is None:
        monkeypatch.delenv("VDL2GPU_REPAIR_ROUNDS", raising=False)
    else:
        monkeypatch.setenv("VDL2GPU_REPAIR_ROUNDS", rounds)
    if k1 == "general":
        monkeypatch.setenv("VDL2GPU_NO_K1_FAST", "1")
    else:
        monkeypatch.delenv("VDL2GPU_NO_K1_FAST", raising=False)
    j = PC.judge(name)
    raw = j.plane.raw()
    n = raw.size // 2
    want = j.blocks
    frames = path == "default"
    soft = name == "slicer" and path == "default"
    with _rx(n, kw, frames=frames, soft_rs=soft, more_flags=lib.F_DEBUG_HEADS if name in HEADS else 0) as rx:
        rx.push(raw)            # one push: the debug taps hold the last push's planes, candidates and header soft bits
        g = rx.debug_dec(0, 0)
        assert len(g) == len(j.plane.plane) and np.array_equal(_bits(g), _bits(j.plane.plane))      # the identity, on the GPU
        k1n = rx.debug_k1()
        assert (k1n["k1_pp"] > 0) == (k1 is None) and k1n["k1_fast"] == 0, k1n
        got = rx.poll()
        TR._check_bursts(oracle, got, want, PC.SDRCLK, rx.poll_frames() if frames else None)
        if path in SCANNING:
            _check_cands(j, rx.debug_cands(0, 0))
        if name in HEADS:
            _check_heads(j, rx.debug_heads())
        if soft:
            _check_soft(j, got)
        st = rx.stats()
        assert st["bursts"] == len(want) and st["overflowed"] == 0
    for block in PC.cutting_blocks(j.plane):     # ... and cut into pushes, one of the cuts inside a sync word, one inside a header
        with _rx(block, kw) as rx:
            TR._check_bursts(oracle, rx.run(raw, block=block), want, PC.SDRCLK)
            rx.stats()
