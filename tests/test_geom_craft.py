"""The planes of tests/geom_craft.py against the oracle, on the CPU: the COVERAGE CONDITIONS that keep tests/test_gpu_geometry.py from
passing on inputs that miss what they aim at.  Held against the oracle's own triggers and blocks and the transmitter's rows
(synth.received_rows), never the GPU.

Run with -s for the byte counts, timing classes and cut distances each plane reaches (DESIGN.md section 2 quotes them)."""
import collections

import numpy as np
import pytest

import geom_craft as G
import plane_craft as PC
from vdlm2dec_amd import synth


@pytest.fixture(scope="module")
def J(oracle):
    return G.judge


def _accepted_headers():
    """(nbrow, nlbyte) of every length field a receiver accepts"""
    return sorted({(ln // synth.ROW_BITS + 1, (ln % synth.ROW_BITS + 7) // 8) for ln in range(8 * G.SHORTEST, 8 * synth.ROW_BITS)})


def test_the_byte_counts_are_the_reference_schedule():
    """takes() against the transmitter's own layout (synth.fec_layout / burst_bits), wherever the transmitter sends what the receiver takes"""
    for ln in range(8 * G.SHORTEST, 8 * synth.ROW_BITS):
        r, n = ln // synth.ROW_BITS + 1, (ln % synth.ROW_BITS + 7) // 8
        nd, nf = G.takes(r, n)
        assert PC.busy_symbols(ln) == PC.HEAD0 + G.nsym_of(r, n)
        if n and ln % 8 == 0:
            nbrow, nlbyte, rows_fec, nfec_last = synth.fec_layout(ln)
            assert (nbrow, nlbyte) == (r, n) and nd == ln // 8 == G.sent_bytes(r, n)
            assert nf == 6 * (rows_fec - 1) + (nfec_last if rows_fec == nbrow else 6)
    for r, n in ((1, 12), (1, 31), (2, 2), (2, 3), (3, 67), (8, 248)):
        assert len(synth.burst_bits(bytes(G.sent_bytes(r, n)))) == 25 + 8 * sum(G.takes(r, n))


@pytest.mark.parametrize("name", ("geom", "geom_frames"))
def test_the_plane_is_the_identity_and_settled(J, name):
    j = J(name)
    assert len(j.dec) == len(j.plane.plane) < 3_200_000
    assert np.array_equal(j.dec.view(np.uint32), j.plane.plane.view(np.uint32))
    assert np.isfinite(j.plane.plane.view(np.float32)).all()
    c0, c1 = j.plane.cases[0], j.plane.cases[1]
    gap = j.plane.plane[int(c0.t0) + (c0.nsym() + 5) * PC.SPS:int(c1.t0) - 5 * PC.SPS]
    assert len(gap) >= PC.GAP - 16 and not gap.view(np.uint32).any()           # exact zeros between the cases
    # one round of settle(): RESERVE holds every header that kept the receiver busy past its case, and nothing grew (a stale table fails here)
    assert {(name, c.label, c.align): c.reserve for c in j.plane.cases if c.reserve} == {k: v for k, v in G.RESERVE.items() if k[0] == name}
    assert len({b.trig_dec for b in j.blocks}) == len(j.blocks)


def test_geom_is_the_intended_geometry_with_the_transmitters_rows(J):
    j = J("geom")
    want = [(r, n) for r in G.NBROWS for n in G.NLBYTES if G.sent_bytes(r, n) >= G.SHORTEST]
    assert len(want) == 115
    got = collections.Counter()
    for c in j.plane.cases:
        b = G.block_of(j, c)
        assert b is not None and (b.nbrow, b.nlbyte) == (c.nbrow, c.nlbyte), (c.label, c.align, b)
        assert len(c.payload) == G.sent_bytes(c.nbrow, c.nlbyte) and (c.length_bits is None or c.nlbyte == 249)
        if c.nlbyte:            # (nlbyte 0: the receiver reads a whole last row the transmitter never sent)
            assert b.data == synth.received_rows(c.payload)[2], (c.label, c.align)
        assert b.end_dec - b.trig_dec == G.j0_of(j.sync_trigger(c)["clk"]) + PC.SPS * (G.nsym_of(b.nbrow, b.nlbyte) - 1)
        got[(c.nbrow, c.nlbyte)] += 1
    assert set(want) <= set(got) and [c.align for c in j.plane.cases[:16]] == list(PC.ALIGNS) * 2
    extra = [t for t in j.triggers if j.plane.case_of(t["dec_index"]) is None]
    print(f"\ngeom: {len(j.plane.cases)} cases of {len(got)} geometries, {len(j.triggers)} triggers, {len(j.blocks)} blocks, "
          f"{len(j.plane.plane)} plane samples; triggers behind a case: {[(t['accepted'], t['len_bits']) for t in extra]}")
    assert len(j.blocks) == len(j.plane.cases) + sum(t["accepted"] == 1 for t in extra)


def test_geom_reaches_every_residue_and_both_sides_of_every_lane_stride(J):
    j = J("geom")
    counts = {sum(G.takes(b.nbrow, b.nlbyte)) for b in j.blocks}
    assert {n % 3 for n in counts} == {0, 1, 2}                     # the last symbol carries 1, 2 and 3 bits: (25 + 8 n) % 3
    assert {(25 + 8 * n) % 3 for n in counts} == {0, 1, 2}
    assert max(counts) == 2039 and min(counts) <= 31
    possible = sorted({sum(G.takes(r, n)) for r, n in _accepted_headers()})
    near = {}
    for s in G.STRIDES:
        for v in (s - 1, s, s + 1):
            if v in possible:
                assert v in counts, v
            else:               # no header gives this count: the nearest one that exists on that side stands in
                side = [p for p in possible if p < v] if v < s else [p for p in possible if p > v]
                near[v] = max(side) if v < s else min(side)
                assert near[v] in counts, (v, near[v])
    print(f"\ngeom: byte counts near the strides {sorted(n for n in counts if any(abs(n - s) <= 3 for s in G.STRIDES))}; "
          f"counts no header gives -> the nearest that one does: {near}")
    assert near == {513: 515}
    # 255 needs a length that is no whole number of bytes: 1985 .. 1991 bits are one row of 249 bytes, and what is sent for 1992 bits
    # -- (2, 0), of which the receiver takes 504 -- is exactly that row and its six parity bytes
    assert len(synth.burst_bits(bytes(249))) == 25 + 8 * 255 and {(1, 249), (2, 0)} <= {(b.nbrow, b.nlbyte) for b in j.blocks}


def test_geom_meets_one_geometry_in_every_timing_class(J):
    j = J("geom")
    every = collections.Counter(G.j0_of(t["clk"]) for t in j.triggers if t["accepted"] == 1)
    one = collections.Counter(G.j0_of(j.sync_trigger(c)["clk"]) for c in j.plane.cases if (c.nbrow, c.nlbyte) == G.TIMING_GEOM)
    print(f"\ngeom: j0 of every accepted trigger {sorted(every.items())}, of the {G.TIMING_GEOM} cases {sorted(one.items())}")
    assert min(one) == min(every) and max(one) == max(every) and min(every) < max(every)


def test_geom_frames_one_frame_each_and_the_flipped_byte_corrected(J, oracle):
    j = J("geom_frames")
    assert [(c.nbrow, c.nlbyte) for c in j.plane.cases] == G.geometries(frames=True) and len(j.plane.cases) == 108 + 3
    n_frames = collections.Counter()
    shortened = 0
    for c in j.plane.cases:
        b = G.block_of(j, c)
        assert b is not None and (b.nbrow, b.nlbyte) == (c.nbrow, c.nlbyte), (c.label, c.align)
        assert len(c.payload) == G.sent_bytes(c.nbrow, c.nlbyte) and c.payload[0] == 0x7e
        clean = synth.received_rows(c.payload)
        frames = oracle.frames_of_block(b.nbrow, b.nlbyte, b.data)
        if c.nlbyte > 2:
            differ = [i for i, (x, y) in enumerate(zip(b.data, clean[2])) if x != y]
            assert differ == [255 * (c.nbrow - 1)] and b.data[differ[0]] ^ clean[2][differ[0]] == G.FLIP, (c.label, differ)    # the flip reached the slicer
            assert len(frames) == 1 and frames == oracle.frames_of_block(*clean), (c.label, len(frames))                          # ... and the row was corrected
            assert len(frames[0]) >= len(c.payload) - 8 - len(c.payload) // 40      # the longest frame that fits (flags, FCS, stuffed bits)
            shortened += G.takes(c.nbrow, c.nlbyte)[1] - 6 * (c.nbrow - 1) < 6
        else:
            assert b.data == clean[2] and frames == oracle.frames_of_block(*clean)
        n_frames[(c.nlbyte > 2, len(frames))] += 1
    print(f"\ngeom_frames: (nlbyte > 2, frames) -> cases {dict(n_frames)}; {shortened} corrected by a last row of 2 or 4 parity bytes")
    assert shortened >= 40


@pytest.mark.parametrize("F", list(G.EDGE_SWEEPS))
def test_edge_cut_copies_cover_every_distance_to_the_cut(J, F):
    j = J(f"edge_cut:{F}")
    assert len(j.plane.plane) % F == 0 and np.array_equal(j.dec.view(np.uint32), j.plane.plane.view(np.uint32))
    assert (F > G.SERIAL_BELOW) == (F == 5000)          # 5000 frames: the parallel path; 1376: straight to the serial machine
    rows = G.edge_rows(j, F)
    assert len(rows) == len(j.plane.cases) == len(j.blocks) == len(j.triggers)         # every copy taken, and nothing else
    seen = collections.defaultdict(set)
    for c, b, name, cut, d in rows:
        assert (b.nbrow, b.nlbyte) == synth.fec_layout(8 * len(c.payload))[:2] and b.data == synth.received_rows(c.payload)[2]
        st = G.stamps(b)
        assert st["trig"] < st["head"] - 64 <= st["trig"] + 8 and st[name] + d == cut and cut % F == 0 and abs(d) <= F // 2
        seen[c.sweep].add(d)
    for n, s, cover in G.EDGE_SWEEPS[F]:
        ds = seen[f"{n}/{s}"]
        print(f"\nedge_cut:{F} {n} bytes, {s}: d = {min(ds)} .. {max(ds)}")
        assert set(range(-cover, cover + 1)) <= ds, (n, s, sorted(ds))
    last_bits = {(25 + 8 * sum(G.takes(b.nbrow, b.nlbyte))) % 3 for _, b, *_ in rows}
    assert last_bits == ({0, 1, 2} if F == 5000 else {(25 + 8 * 2039) % 3})
