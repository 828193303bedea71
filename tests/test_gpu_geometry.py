"""The payload decode at every burst geometry, and the defer rule at a push's end frame by frame (tests/geom_craft.py), through the
whole HIP path, judged by the oracle.

burst_geom / burst_scatter replace the reference's byte-by-byte interleaver with divisions, burst_payload strides lanes over the ND + NF
bytes, burst_payload_soft and burst_payload_levels repeat the geometry, k4_frames takes a row's parity count from burst_geom for the soft row rule: `geom` has one
clean burst for nbrow 1 .. 8 x the last row's byte counts either side of every parity threshold, for the byte counts either side of the
lane strides, and one geometry in every timing class; `geom_frames` the same with a real frame in each and a flipped byte in the last
row.  `edge_cut` walks a burst's last symbol, header symbol 8 and trigger across the end of a push one frame at a time.

The rig is the exact identity of tests/test_gpu_planes.py (asserted on every part pushed).  That the planes sit where they aim is
asserted on the CPU (tests/test_geom_craft.py).  How the chain gets to the oracle's answer is the design's business: nothing looks at
`repairs` or `serial_redos`.

Every path takes the FULL sweep: on an MI355X a path's run over the 2.8 M frames of `geom` is 0.05 - 0.25 s, the three runs of
`geom_frames` together 1 s, an `edge_cut` plane (379 or 430 pushes, each polled) 0.1 - 0.8 s; building the planes and asking the
oracle is 2 s for `geom` and 3 s for `geom_frames`, once per process; the whole file 11 s."""
import types

import numpy as np
import pytest

import geom_craft as G
import plane_craft as PC
import test_gpu_levels as TL
import test_gpu_rates as TR
from test_gpu_chain import PART, _env, _push_parts
from test_gpu_planes import PATHS, _bits, _rx

pytestmark = pytest.mark.gpu


def _push_whole(rx, j, raw):
    """the plane in parts of PART input samples, the identity asserted behind each; returns the planes the kernels worked on"""
    dec, pos = [], 0
    for g in _push_parts(rx, raw):
        want = j.plane.plane[pos:pos + len(g)]
        assert len(g) == min(PART // 2, len(j.plane.plane) - pos) and np.array_equal(_bits(g), _bits(want)), pos
        dec.append(g)
        pos += len(g)
    assert pos == len(j.plane.plane) and len(dec) == -(-raw.size // 2 // PART)
    return np.concatenate(dec)


@pytest.mark.timeout(180)
@pytest.mark.parametrize("path", list(PATHS))
def test_every_geometry_equals_the_oracle(built, oracle, monkeypatch, path):
    """the full sweep on every path of PATHS: records, stamps and df bits"""
    kw = _env(monkeypatch, path)
    j = G.judge("geom")
    raw = j.plane.raw()
    with _rx(PART, kw) as rx:
        _push_whole(rx, j, raw)
        got = rx.poll()
        TR._check_bursts(oracle, got, j.blocks, PC.SDRCLK)
        assert {(b.nbrow, b.nlbyte) for b in got} >= set(G.geometries())
        st = rx.stats()
        assert st["bursts"] == len(j.blocks) and st["overflowed"] == 0


def _check_soft(name, got):
    maps = G.soft_maps(name)
    assert len(got) == len(maps) >= 100
    for b in got:
        hard, rel, taken = maps[b.trig_dec]
        assert hard.tobytes() == b.data, b.trig_dec              # the model is the oracle's slicer ...
        assert b.soft is not None and np.array_equal(b.soft, rel), (b.trig_dec, b.nbrow, b.nlbyte)
        assert (b.soft[~taken] == 255).all() and int(taken.sum()) == sum(G.takes(b.nbrow, b.nlbyte))     # ... bytes never taken are 255


@pytest.mark.timeout(180)
@pytest.mark.parametrize("levels,soft", [(True, False), (False, True), (True, True)], ids=["levels", "soft", "levels+soft"])
def test_every_geometry_with_levels_and_soft_maps(built, oracle, monkeypatch, levels, soft):
    """K2d's three other kernels: the levels and the reliability maps repeat the geometry"""
    kw = _env(monkeypatch, "default")
    j = G.judge("geom")
    raw = j.plane.raw()
    with _rx(PART, kw, levels=levels, soft_rs=soft) as rx:
        dec = _push_whole(rx, j, raw)
        got = rx.poll()
        TR._check_bursts(oracle, got, j.blocks, PC.SDRCLK)
        st = rx.stats()
        assert st["bursts"] == len(j.blocks) and st["overflowed"] == 0
    if soft:
        _check_soft("geom", got)
    else:
        assert all(b.soft is None for b in got)
    if levels:
        for b in got:       # from the record's own header by the reference's rules, not from the kernel's geometry
            assert b.level.nsym == G.nsym_of(b.nbrow, b.nlbyte) == (25 + 8 * sum(G.takes(b.nbrow, b.nlbyte)) + 2) // 3, (b.nbrow, b.nlbyte)
        wide = dec.astype(np.complex128)      # (levels_ref works in float64: converted once, not per burst)
        whole = types.SimpleNamespace(debug_dec=lambda stream, ch: wide)      # (... and indexes the plane by the records' own stamps)
        TL._check_exact(whole, got, types.SimpleNamespace(rate=PC.RATE), "cf32")
    else:
        assert all(b.level is None for b in got)


@pytest.mark.timeout(180)
def test_a_frame_in_every_geometry(built, oracle, monkeypatch):
    """k4_frames behind the payload decode: the last row's parity count, its erasures, and a byte to correct in it"""
    j = G.judge("geom_frames")
    raw = j.plane.raw()
    plain = None
    for path, soft in (("default", False), ("noregion-r0", False), ("default", True)):
        kw = _env(monkeypatch, path)
        with _rx(PART, kw, frames=True, soft_rs=soft) as rx:
            _push_whole(rx, j, raw)
            got = rx.poll()
            frames = rx.poll_frames()
            st = rx.stats()
        assert st["bursts"] == len(j.blocks) and st["overflowed"] == 0
        if not soft:
            TR._check_bursts(oracle, got, j.blocks, PC.SDRCLK, frames)         # the oracle's frames, every one
            assert len(frames) >= sum(c.nlbyte > 2 for c in j.plane.cases)
            plain = sorted(frames)
        else:
            TR._check_bursts(oracle, got, j.blocks, PC.SDRCLK)
            assert sorted(frames) == plain                                     # the soft row rule loses and adds nothing


@pytest.mark.timeout(180)
@pytest.mark.parametrize("path", ("default", "serial", "noregion-r2"))
@pytest.mark.parametrize("F", list(G.EDGE_SWEEPS))
def test_a_pushs_end_frame_by_frame(built, oracle, monkeypatch, F, path):
    """Receiver.run polls behind every push of F frames.  A burst whose last symbol is not there yet waits for the next push (the
    defer rule of mach_trigger: the header needs nsym0 + 64, the burst end_dec); one frame further and it may be delivered."""
    kw = _env(monkeypatch, path)
    j = G.judge(f"edge_cut:{F}")
    raw = j.plane.raw()
    polls = []
    with _rx(2 * F, kw) as rx:
        poll = rx.poll
        rx.poll = lambda *a, **k: polls.append(poll(*a, **k)) or polls[-1]
        got = rx.run(raw, block=2 * F)
        st = rx.stats()
    assert len(polls) == len(j.plane.plane) // F
    TR._check_bursts(oracle, got, j.blocks, PC.SDRCLK)           # equal to the oracle, every burst once
    assert st["bursts"] == len(j.blocks) and st["overflowed"] == 0 and st["deferrals"] > 0
    behind = {}
    for k, bursts in enumerate(polls):
        for b in bursts:
            assert (k + 1) * F > b.end_dec, (k, b.trig_dec, b.end_dec)       # never before the push that holds its last symbol's frame
            behind[b.trig_dec] = (k + 1) * F
    for n, stamp, _ in G.EDGE_SWEEPS[F]:
        rows = [(b, cut, d, behind[b.trig_dec]) for c, b, name, cut, d in G.edge_rows(j, F) if c.sweep == f"{n}/{stamp}"]
        late = [(d, (at - b.end_dec - 1) // F) for b, cut, d, at in rows]
        print(f"\nedge_cut:{F} {path} {n} bytes, {stamp}: pushes waited past the one that holds end_dec, by d: {sorted(late)}")
        if stamp != "end":
            continue
        # slack: frames from end_dec to the end of the push that holds it (1: it is that push's last frame)
        hold = [(b.end_dec // F + 1) * F for b, *_ in rows]
        at_once = sorted(h - b.end_dec for (b, _, _, at), h in zip(rows, hold) if at == h)
        waited = sorted(h - b.end_dec for (b, _, _, at), h in zip(rows, hold) if at > h)
        print(f"edge_cut:{F} {path} {n} bytes: delivered at once from a slack of {at_once[0] if at_once else None} frames; "
              f"waited at slacks {waited}")
        assert all(at in (cut, cut + F) for _, cut, _, at in rows)
        assert {at - cut for _, cut, _, at in rows} == {0, F}       # behind the push that ends at the sweep's cut, and behind the next
