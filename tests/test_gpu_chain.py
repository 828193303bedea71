"""Bursts that follow each other closely (tests/chain_craft.py) through the whole HIP path, judged by the oracle: followers triggered
while the detector still fits a partly stale ring, on both sides of VDL2_STEADY; trains longer than VDL2_CL_MAXB; bursts inside the time
a mis-sized header claims, which the scan lists and the chain must step over; stale sync words that fire again behind a burst.

The rig is the exact identity of tests/test_gpu_planes.py (asserted again here), so every family x decode path must give the oracle's
records, stamps and carrier estimates.  That the planes sit where they aim is asserted on the CPU (tests/test_chain_craft.py); that
the default path really took the code they aim at -- clusters of several bursts, clusters stopped at the limit -- is asserted here from
the cluster heads.  How the chain gets to the oracle's answer is the design's business: nothing looks at `repairs` or `serial_redos`."""
import types

import numpy as np
import pytest

import chain_craft as CC
import plane_craft as PC
import test_gpu_levels as TL
import test_gpu_rates as TR
from test_gpu_planes import PATHS, SCANNING, _bits, _rx
from vdlm2dec_amd import lib

pytestmark = pytest.mark.gpu


def _env(monkeypatch, path):
    kw, rounds, k1 = PATHS[path]
    if rounds is None:
        monkeypatch.delenv("VDL2GPU_REPAIR_ROUNDS", raising=False)
    else:
        monkeypatch.setenv("VDL2GPU_REPAIR_ROUNDS", rounds)
    if k1 == "general":
        monkeypatch.setenv("VDL2GPU_NO_K1_FAST", "1")
    else:
        monkeypatch.delenv("VDL2GPU_NO_K1_FAST", raising=False)
    return kw


def _heads(rx):
    """[(status, slots, bursts)] of the last push's clusters"""
    heads = [lib.cl_unpack(p) for p in rx.debug_clheads(0, 0)[:, 1]]
    return [(status, nslots, nburst) for status, _, nslots, _, _, nburst in heads]


def _check_heads(name, heads):
    steady = {b for st, _, b in heads if st == lib.CL_STEADY}
    print(f"\n{name}: cluster heads (status, slots, bursts) -> number: { {h: heads.count(h) for h in sorted(set(heads))} }")
    if name == "train":
        # a cluster that found its fourth burst before the detector was history-free again stopped at the limit and handed the
        # resolver its saved state (no cluster can end steady on four: the limit is looked at first) ...
        assert (lib.CL_NONSTEADY, CC.MAXB, CC.MAXB) in heads
        assert {2, 3} <= steady         # ... shorter trains, and the ends of long ones, are steady clusters of two and of three bursts
    if name == "claim":
        assert {1, 2} <= steady         # B taken inside A's cluster, and B met through the candidate table


def _check_listed(j, cands):
    """swallow: the scan lists the bursts inside the claimed time like any other (on clean planes their sync words are perfect)"""
    nrel = np.unique(cands.view(np.uint32).reshape(-1, 6)[:, 0].astype(np.int64))
    # the table counts from the start of the push's planes.  Every group's head is in it at one common offset; the groups look alike, so
    # a few other offsets fit as well (a head's instant on a burst inside the NEXT group): the first entry is the first head's
    heads = [j.sync_trigger(g[0])["dec_index"] for g in CC.groups_of(j.plane)]
    offs = set.intersection(*(set((nrel - t).tolist()) for t in heads))
    off = min(offs, key=lambda o: abs(o - (int(nrel[0]) - heads[0])))
    assert abs(off - (int(nrel[0]) - heads[0])) <= 8, (sorted(offs)[:8], int(nrel[0]), heads[0])
    nrel = nrel - off
    inside = [c for c in j.plane.cases if c.role.startswith("in")]
    assert len(inside) >= 20
    for c in inside:
        lo, hi = c.trig_window()
        assert np.searchsorted(nrel, hi) > np.searchsorted(nrel, lo), (c.label, c.role)


PART = 800_000      # input samples: a handle cuts a push longer than 8.4 s into parts and its debug taps hold the last part only, so the
#                     planes longer than that are handed over in pushes of their own, each one part, and the taps are read behind each


def _push_parts(rx, raw):
    """push the plane, one part at a time; behind each part yield what the taps hold of it"""
    n = raw.size // 2
    for s in range(0, n, PART):
        rx.push(raw[2 * s:2 * min(n, s + PART)])
        yield rx.debug_dec(0, 0)


@pytest.mark.timeout(180)
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("name", CC.FAMILIES)
def test_chain_planes_equal_the_oracle(built, oracle, monkeypatch, name, path):
    kw = _env(monkeypatch, path)
    j = CC.judge(name)
    raw = j.plane.raw()
    frames = path == "default"
    with _rx(min(raw.size // 2, PART), kw, frames=frames) as rx:
        dec, heads = [], []
        for g in _push_parts(rx, raw):
            dec.append(g)
            heads += _heads(rx) if path == "default" else []
        g = np.concatenate(dec)
        assert len(g) == len(j.plane.plane) and np.array_equal(_bits(g), _bits(j.plane.plane))      # the identity, on the GPU
        got = rx.poll()
        TR._check_bursts(oracle, got, j.blocks, PC.SDRCLK, rx.poll_frames() if frames else None)
        st = rx.stats()
        assert st["bursts"] == len(j.blocks) and st["overflowed"] == 0
        if path == "default":
            _check_heads(name, heads)
        if name == "swallow" and path in SCANNING:
            assert len(dec) == 1        # (one part: the table is the whole plane's)
            _check_listed(j, rx.debug_cands(0, 0))


@pytest.mark.timeout(180)
@pytest.mark.parametrize("path", ("default", "serial", "noregion-r2"))
@pytest.mark.parametrize("name", ("train", "claim"))
def test_pushes_cut_where_the_state_is_carried(built, oracle, monkeypatch, name, path):
    """a cut 1 .. 67 evaluations behind a burst (the ChanState crosses the push with `fresh` below VDL2_STEADY), a cut inside a
    follower's header (its cluster defers with bursts already counted) and a cut between a train's fourth and fifth burst"""
    kw = _env(monkeypatch, path)
    j = CC.judge(name)
    raw = j.plane.raw()
    for block in CC.cutting_blocks(j):
        assert block > 2 * CC.SERIAL_BELOW
        with _rx(block, kw) as rx:
            TR._check_bursts(oracle, rx.run(raw, block=block), j.blocks, PC.SDRCLK)
            st = rx.stats()
            assert st["bursts"] == len(j.blocks) and st["overflowed"] == 0


def _check_soft(j, got):
    """tests/soft_ref.py on the oracle's plane, as test_gpu_planes._check_soft has it (without the slicer family's own conditions)"""
    import soft_ref as R
    clk = {t["dec_index"]: t["clk"] for t in j.triggers if t["accepted"] == 1}
    pn = R.pn_bits()
    assert len(got) == len(j.blocks) >= 100
    want = {b.trig_dec: R.soft_block(j.dec, b.nbrow, b.nlbyte, b.df, b.trig_dec, clk[b.trig_dec], pn) for b in j.blocks}
    for b in got:
        hard, rel = want[b.trig_dec]
        assert hard.tobytes() == b.data, b.trig_dec
        assert b.soft is not None and np.array_equal(b.soft, rel), b.trig_dec


@pytest.mark.timeout(180)
@pytest.mark.parametrize("name", ("train", "collide"))
def test_levels_and_reliability_of_a_close_follower(built, oracle, monkeypatch, name):
    """a follower's noise window lies inside the burst before it: the definition (include/vdl2gpu.h) does not care, nor may the kernels"""
    kw = _env(monkeypatch, "default")
    j = CC.judge(name)
    raw = j.plane.raw()
    with _rx(min(raw.size // 2, PART), kw, levels=True, soft_rs=True) as rx:
        dec = np.concatenate(list(_push_parts(rx, raw)))
        assert np.array_equal(_bits(dec), _bits(j.dec))       # the planes the kernels measured on are the oracle's tap
        got = rx.poll()
        TR._check_bursts(oracle, got, j.blocks, PC.SDRCLK)
        ends = sorted(b.end_dec for b in j.blocks)
        close = [b for b in got if any(0 < b.trig_dec - e < 2 * CC.STEADY for e in ends)]
        assert len(close) >= 40         # followers met below VDL2_STEADY are among what is measured
        whole = types.SimpleNamespace(debug_dec=lambda stream, ch: dec)       # (levels_ref indexes the plane by the records' own stamps)
        TL._check_exact(whole, got, types.SimpleNamespace(rate=PC.RATE), "cf32")
        _check_soft(j, got)
