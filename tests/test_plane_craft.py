"""The crafted planes of tests/plane_craft.py against the oracle, on the CPU: the identity set-up, and the COVERAGE CONDITIONS that keep
tests/test_gpu_planes.py from passing on inputs that miss the edge they aim at.  The conditions are held against the oracle's own
triggers() -- fit errors, header soft bits and decoded lengths as the reference computes them --, never against the GPU.

Run with -s for the achieved perr / err / |v - 0.5| ranges per family (DESIGN.md section 2 quotes them).

What a sweep can and cannot show.  The oracle records the fit errors of the triggers its chain TOOK; a step that does not fire leaves no
number behind, only the fact: by the detector's rule (d8psk.c:292) the minimum of the fit error in the chain's class was then >= 4.  So
"across a flip the errors differ by at most 0.1" is held as: the firing neighbour of a step that does not fire has perr >= 3.9."""
import numpy as np
import pytest

import plane_craft as PC
from vdlm2dec_amd import synth


@pytest.fixture(scope="module")
def J(oracle):
    return PC.judge


@pytest.mark.parametrize("name", PC.FAMILIES)
def test_the_decimated_tap_is_the_crafted_plane(J, name):
    """100 kS/s, SDRCLK 42, Fo = 0, cf32, every plane sample twice: the channeliser is an exact identity"""
    j = J(name)
    assert len(j.dec) == len(j.plane.plane)
    assert np.array_equal(j.dec.view(np.uint32), j.plane.plane.view(np.uint32))
    assert np.isfinite(j.plane.plane.view(np.float32)).all()
    if name in ("notch", "lengths"):        # the variant with exact zeros between the cases
        c0, c1 = j.plane.cases[0], j.plane.cases[1]
        gap = j.plane.plane[int(c0.t0) + (c0.nsym() + 5) * PC.SPS:int(c1.t0) - 5 * PC.SPS]
        assert len(gap) >= PC.GAP - 16 and not gap.view(np.uint32).any()


def _fired(j):
    """[(case, trigger or None)]"""
    return [(c, j.sync_trigger(c)) for c in j.plane.cases]


def _flips(rows):
    """neighbouring steps of one sweep at one alignment of which one fires and the other does not: [(trigger of the one that fires)]"""
    by = {}
    for c, t in rows:
        by.setdefault((c.sweep, None if c.family == "plateau" else c.align), []).append((c.step, t))
    out = []
    for seq in by.values():
        seq.sort(key=lambda x: x[0])
        for (s0, t0), (s1, t1) in zip(seq, seq[1:]):
            if s1 == s0 + 1 and (t0 is None) != (t1 is None):
                out.append(t0 or t1)
    return out


@pytest.mark.parametrize("name", PC.SCAN_FAMILIES)
def test_scan_sweeps_cross_the_detector_threshold(J, name):
    j = J(name)
    rows = _fired(j)
    perr = np.array([t["perr"] for _, t in rows if t is not None])
    err = np.array([t["err"] for _, t in rows if t is not None])
    flips = _flips(rows)
    near = int(((perr >= 3.6) & (perr < 4.0)).sum())
    close = sorted((t["perr"] for t in flips), reverse=True)[:3]
    print(f"\n{name}: {len(rows)} cases, {len(perr)} fire, perr {perr.min():.3f} .. {perr.max():.3f}, err {err.min():.2f} .. {err.max():.2f}, "
          f"{near} triggers with perr in [3.6, 4), {len(flips)} flips, the three closest firing neighbours perr {[round(float(x), 3) for x in close]}")
    assert 0 < len(perr) < len(rows)            # some steps fire, others do not
    assert flips                                # ... next to each other
    assert near >= 3
    assert len(close) == 3 and close[-1] >= 3.9   # three flips whose other side, its minimum at >= 4, is within 0.1
    assert all(t["perr"] < 4.0 for _, t in rows if t is not None)
    if name == "plateau":
        flat = [t for _, t in rows if t is not None and abs(t["err"] - t["perr"]) < 0.1]
        print(f"plateau: {len(flat)} triggers with |err - perr| < 0.1, the closest {min(abs(t['err'] - t['perr']) for t in flat):.4f}")
        assert len(flat) >= 3
    if name == "notch":
        assert {c.param for c, _ in rows} >= {1.0, 1e-2, 1e-4, 1e-8, 0.0}
    if name == "cfo":
        pfr = np.array([t["pfr"] for _, t in rows if t is not None])
        print(f"cfo: pfr {pfr.min():.3f} .. {pfr.max():.3f} rad / symbol")
        assert pfr.min() < -2.0 and pfr.max() > 0.5         # the slope of the fit far from 0, both signs (2 pi f / 10500 less the 0.35 the outlier adds)


def test_deep_steps_fire_in_some_classes_only(J):
    j = J("deep")
    rows = _fired(j)
    steps = {}
    for c, t in rows:
        steps.setdefault(c.step, []).append(t)
    marginal = [s for s, ts in steps.items() if any(t is not None and t["perr"] < 4.0 for t in ts) and any(t is None for t in ts)]
    silent = [s for s, ts in steps.items() if all(t is None for t in ts)]
    print(f"\ndeep: {len(steps)} steps, {len(marginal)} fire at some alignments only, {len(silent)} at none (perturbations up to "
          f"{max(c.param for c, _ in rows if c.sweep == 'outlier_mid'):.2f} rad on one symbol, {max(c.param for c, _ in rows if c.sweep == 'zigzag'):.2f} zigzag)")
    assert len(marginal) >= 3
    assert len(silent) >= 6                 # ... and the sweep goes on far past the threshold (fit error of the minimum beyond 7.5)


def test_edge_cases_sit_on_the_margins_to_the_last_bit(J):
    """What a wrong margin in the sparse stages would need to show: a minimum of the fit error a few 1e-7 below the detector's 4 (the fourth
    screen works from an estimate and a margin), and two neighbouring evaluations whose fit errors differ by one ulp or not at all (the
    fifth screen orders estimates, again with a margin) -- far inside what the estimates can resolve."""
    j = J("edge")
    rows = _fired(j)
    zz = [t for c, t in rows if c.sweep == "zz"]
    pl = [t for c, t in rows if c.sweep == "pl"]
    near4 = sorted(4.0 - float(t["perr"]) for t in zz if t is not None)
    up = sorted(float(t["err"]) - float(t["perr"]) for t in pl if t is not None)
    down = sorted(abs(float(t["perr"]) - float(t["p2err"])) for t in pl if t is not None)
    print(f"\nedge: 4 - perr {[f'{x:.1e}' for x in near4]}, {sum(t is None for t in zz)} past 4; err - perr from {up[0]:.1e}: {[f'{x:.1e}' for x in up[:4]]}; "
          f"|perr - p2err| from {down[0]:.1e}: {[f'{x:.1e}' for x in down[:4]]}")
    assert all(t is not None for t in pl)
    assert sum(t is None for t in zz) >= 2                       # just past 4: no trigger
    assert 0 < near4[0] < 1e-6 and near4[4] < 1e-6 and near4[8] < 1e-3      # just below: triggers, five of them within 5e-7
    assert 0 < up[0] < 1e-6 and up[1] < 1e-4 and up[2] < 1e-3    # err = perr + 1 ulp: the strict > of d8psk.c:292 holds, and fires
    assert down[0] == 0.0 and down[1] < 1e-4 and down[2] < 1e-3  # perr == p2err: not "a later step of a run" (perr > p2err is strict too)


HEADER_BIT = 14     # the soft bit the `header` sweep moves: third tribit of symbol 25


def test_header_sweep_puts_a_soft_bit_on_the_boundary(J):
    """The issue asked for soft bits with 1e-3 < |v - 0.5| < 2e-3 and with 0 < |v - 0.5| < 1e-3.  NO INPUT GIVES THOSE: a soft bit is an entry
    of one of the three 257-entry Grey tables or one minus it (d8psk.c:71-83), and the entries are exactly 0.5 at the decision boundaries
    and at least 0.047 away from it everywhere else -- asserted below over all 771 entries.  So the header gate's band |v - 0.5| < 1e-3 holds
    v == 0.5 and nothing else, and that value IS reachable: the sweep lands on it, on its two neighbours 0.5 -+ 0.0471, and beyond."""
    import soft_ref as R
    g = R.GREY.astype(np.float64)
    both = np.concatenate([g.ravel(), (1.0 - g).astype(np.float32).astype(np.float64).ravel()])
    d = np.abs(both - 0.5)
    assert (d == 0).sum() >= 9 and d[d > 0].min() > 0.047       # nothing in (0, 2e-3): the gate's band is the boundary itself
    step = float(d[d > 0].min())
    j = J("header")
    sweep = [(c, t) for c, t in _fired(j) if c.sweep != "tie"]
    v = np.array([t["head"][HEADER_BIT] for c, t in sweep if t is not None and len(t["head"]) == 25], np.float64) - 0.5
    print(f"\nheader: {len(v)} triggers, soft bit {HEADER_BIT}: {int((v == 0).sum())} exactly 0.5, {int((v < 0).sum())} below "
          f"(closest {v[v < 0].max():+.4f}), {int((v > 0).sum())} above (closest {v[v > 0].min():+.4f})")
    assert len(v) == len(sweep)
    assert (v == 0).sum() >= 8
    assert (v < 0).any() and (v > 0).any()
    assert np.isclose(v[v < 0].max(), -step) and np.isclose(v[v > 0].min(), step)      # the nearest values there are, both sides
    others = np.array([np.delete(t["head"], HEADER_BIT) for _, t in sweep], np.float64)
    assert (np.abs(others[:, 3:] - 0.5) > 0.3).all()          # ... and no other bit anywhere near: ONE bit crosses


def test_header_ties_are_broken_against_the_hard_decisions(J):
    """Three soft bits exactly 0.5 on the places of a weight-3 codeword: the hard decisions form a codeword (the shortcut's first condition
    holds), yet the reference's trellis, which keeps the survivor it met first, decodes ANOTHER word.  Only the gate |v - 0.5| < 1e-3 keeps
    the shortcut away from these; with the gate at 0 the GPU would return the hard word's length."""
    j = J("header")
    pinned = []
    for c, t in _fired(j):
        if c.sweep != "tie" or t is None or len(t["head"]) < 25:
            continue
        h = t["head"]
        hard = [int(x > 0.5) for x in h]
        syn = 0
        for n in range(25):
            syn ^= synth.HEADER_H[n] if hard[n] else 0
        hard_len = sum(hard[3 + i] << i for i in range(17))
        if int((h == 0.5).sum()) == 3 and syn == 0 and t["len_bits"] != hard_len:
            pinned.append((c.label, c.align, hard_len, t["len_bits"], t["accepted"]))
    print(f"\nheader ties: {pinned}")
    assert len(pinned) >= 2 and len({x[0] for x in pinned}) == 2


def test_header_words_reach_the_trellis_and_other_lengths(J):
    j = J("header_words")
    rows = _fired(j)
    assert all(t is not None and len(t["head"]) == 25 for _, t in rows)        # every case is met by an idle detector
    acc = [t["accepted"] for _, t in rows]
    other = [(c.label, c.align, t["len_bits"]) for c, t in rows if t["accepted"] == 1 and t["len_bits"] != PC.LEN12]
    hard = lambda t: [int(v > 0.5) for v in t["head"]]        # noqa: E731
    cw = synth.header_bits(PC.LEN12)
    words = {c.label: hard(t) for c, t in rows}
    print(f"\nheader_words: {len(rows)} cases, {acc.count(1)} accepted, {acc.count(0)} refused, {len(other)} accepted with another length: "
          f"{sorted({x[2] for x in other})}")
    assert acc.count(1) > 0 and acc.count(0) > 0 and other
    assert words["codeword"] == cw                              # the shortcut's case: a codeword, every bit far from 0.5
    for n in range(3, 25):                                      # (the receiver zeroes the first three soft bits)
        assert words[f"flip{n}"] == PC._flip(cw, n), n          # the hard word IS the flipped one: syndrome != 0, the trellis runs
    for c, t in rows:                                           # the layout reserved what each header made the receiver take
        if t["accepted"] == 1:
            assert PC.busy_symbols(t["len_bits"]) <= c.busy_sym(), (c.label, c.align, t["len_bits"])


def test_lengths_are_the_intended_geometry(J):
    j = J("lengths")
    blocks = {b.trig_dec: b for b in j.blocks}
    want = {lab: geo for lab, _, _, _, geo in PC.LENGTHS}
    seen = {}
    for c, t in _fired(j):
        assert t is not None, (c.label, c.align)
        if want[c.label] is None:
            assert t["accepted"] == 0 and t["dec_index"] not in blocks, c.label
        else:
            b = blocks[t["dec_index"]]
            assert t["accepted"] == 1 and (b.nbrow, b.nlbyte) == want[c.label], (c.label, c.align, b.nbrow, b.nlbyte)
            if want[c.label][1]:        # (a multiple of 1992 bits: the receiver reads a whole last row the transmitter never sent)
                assert b.data == synth.received_rows(c.payload)[2], (c.label, c.align)
        seen[c.label] = seen.get(c.label, 0) + 1
    print(f"\nlengths: {seen}")
    assert set(seen) == set(want)


def test_slicer_sweep_changes_the_bytes_and_returns(J):
    j = J("slicer")
    blocks = {b.trig_dec: b for b in j.blocks}
    sent = synth.received_rows(PC.P40)[2]
    steps = {}
    for c, t in _fired(j):
        assert t is not None and t["accepted"] == 1 and t["len_bits"] == 320, (c.label, c.align)
        steps.setdefault(c.step, []).append(blocks[t["dec_index"]].data)
    last = max(steps)
    diff = {s: sum(sum(a != b for a, b in zip(d, sent)) for d in ds) for s, ds in steps.items()}
    print(f"\nslicer: bytes that differ from the sent ones per step (eight alignments together): {[diff[s] for s in sorted(diff)]}")
    assert all(d == sent for d in steps[0]) and all(d == sent for d in steps[last])
    assert any(v > 0 for v in diff.values())
    assert len({d for ds in steps.values() for d in ds}) >= 4       # several different outcomes along the sweep, not one flip


@pytest.mark.parametrize("name", PC.FAMILIES)
def test_block_cuts_fall_inside_a_sync_word_and_a_header(name):
    pl = PC.family(name)
    a, b = PC.cutting_blocks(pl)
    assert b % 2 == 1 and a > 2 * 4096 * 100 // 84 and 2 * len(pl.plane) > b > 2 * 4096 * 100 // 84     # pushes long enough for the parallel path
