"""Crafted planes in which bursts follow each other CLOSELY: what tests/plane_craft.py keeps apart on purpose (CPU only: numpy).

After a burst the detector keeps the 68 phases it held at the trigger, so for its next 68 evaluations it fits a ring that is partly
stale.  The resolver gives that state a constant (VDL2_STEADY, 68: from there K2b and K2c trust the scan's candidate records), a
limit (VDL2_CL_MAXB, 4 bursts per cluster) and two defer cases; nothing placed GAP apart ever meets them.  Here cases form GROUPS:
inside a group each case is placed against the last symbol of the case before it -- the one it SENT or the one its header CLAIMS --
by a signed offset in plane samples, and only the groups are GAP or more apart.  The rig is plane_craft's exact identity (100 kS/s,
SDRCLK 42, Fo 0, cf32, every plane sample written twice), so the oracle judges every plane.

    count(j, t)     (trigger's dec_index - the previous block's end_dec) / 2, in the oracle's own stamps: the evaluations the
                    detector has made since the receiver went back to idle; below 68 the trigger was fitted on a partly stale ring
    family(name)    `claim`, `collide`, `train`, `swallow`, `stale` (below)

Bursts inside a group carry no tail symbols; the last burst of a group keeps plane_craft's two.  Everything is deterministic; what
had to be found with the oracle is in the tables beside each family, and tests/test_chain_craft.py fails when a table is stale."""
from __future__ import annotations

import dataclasses
import math
from typing import Dict, List, Optional

import numpy as np

import plane_craft as PC
from plane_craft import ALIGNS, FRAC, GAP, HEAD0, NOISE, SPS, payload_bytes
from vdlm2dec_amd import synth

FAMILIES = ("claim", "collide", "train", "swallow", "stale")
STEADY = 68                 # VDL2_STEADY (csrc/vdl2gpu_types.h): evaluations after which the detector has forgotten the last burst
MAXB = 4                    # VDL2_CL_MAXB: bursts a cluster takes before the resolver goes on from its saved state


@dataclasses.dataclass
class Link(PC.Case):
    """a case of a group.  The head of a group has anchor "" and is placed like a case of plane_craft; every other case has its
    symbol 0 at (symbol 0 of case `ref` of the group) + 8 * (that case's last symbol + 1) + offset"""
    group: int = 0
    role: str = ""              # what the case is in its group ("A", "B", "f3": third burst of a train, "in1", "across", "behind")
    anchor: str = ""            # "sent": the last symbol the case before it transmitted; "claim": the last one its header claims
    offset: float = 0.0         # plane samples
    ref: int = -1               # which earlier case of the group the anchor is (index into the group; -1: the one before)
    tail: int = 0               # tail symbols (plane_craft.TAIL for the last burst of a group)

    def symbols(self) -> np.ndarray:
        a = super().symbols()[:-PC.TAIL]
        if self.tail:
            t = np.full(self.tail, 4.0 * a[PC.SYNC0 + PC.SYNC_N - 1] / abs(a[PC.SYNC0 + PC.SYNC_N - 1]) * np.exp(1j * np.pi))
            a = np.concatenate([a, t])
        return a

    def sent(self) -> int:
        """symbols transmitted without the tail = the last transmitted symbol's index + 1"""
        return super().nsym() - PC.TAIL

    def nsym(self) -> int:
        return self.sent() + self.tail

    def claimed(self) -> int:
        """the last symbol the header claims, + 1 (0: a receiver refuses the header)"""
        return PC.busy_symbols(self.acts_on())


def place(groups: List[List[Link]], reserve: Optional[Dict[int, int]] = None) -> int:
    """set every case's t0; reserve: group -> plane samples the oracle has shown the receiver to stay busy behind the group's last
    transmitted or claimed symbol (a stale sync word whose header it accepted, with whatever length came out).  Returns the
    length of the plane."""
    pos = 512
    for gi, g in enumerate(groups):
        for k, c in enumerate(g):
            c.group = gi
            if k == 0:
                assert c.anchor == ""
                c.t0 = float((pos + 4 * SPS + 7) // 8 * 8 + c.align) + (FRAC[c.align] if c.frac is None else c.frac) + c.dt
            else:
                a = g[c.ref if c.ref >= 0 else k - 1]
                n = a.sent() if c.anchor == "sent" else a.claimed()
                assert c.anchor in ("sent", "claim") and n > 0
                c.t0 = a.t0 + SPS * n + c.offset
        pos = group_end(g) + (reserve or {}).get(gi, 0) + GAP
    return pos + 512


def group_end(g: List[Link]) -> int:
    """the plane sample behind everything the group's cases send or claim"""
    return int(math.ceil(max(c.t0 + (max(c.nsym(), c.claimed()) + 4) * SPS for c in g)))


def layout(name: str, groups: List[List[Link]], noise: float = NOISE, seed: int = 0, reserve: Optional[Dict[int, int]] = None) -> PC.Plane:
    """the groups one after the other on a floor drawn per group (seed, step of the group's head): a group sees the same floor wherever
    the groups before it put it, and whichever other groups are there"""
    n = place(groups, reserve)
    acc = np.zeros(n, np.complex128)
    for g in groups:
        for c in g:
            PC.render(acc, c)
    cut = [0] + [int(g[0].t0) - 4 * SPS - GAP // 2 for g in groups[1:]] + [n]
    for i in range(len(groups)):
        rng = np.random.default_rng([seed, groups[i][0].step])
        m = cut[i + 1] - cut[i]
        acc[cut[i]:cut[i + 1]] += noise * (rng.standard_normal(2 * m).view(np.complex128))
    return PC.Plane(name, acc.astype(np.complex64), [c for g in groups for c in g])


# ------------------------------------------------------------------------------------------------------------- the families
P12, P14 = PC.P12, payload_bytes(14)
CLAIM_BITS = 320                                    # A sends P12 and claims 40 bytes
CLAIM_SWEEP = [-60.0 + 0.25 * i for i in range(288)]    # B's symbol 0 against A's claimed last symbol + 1, plane samples
SHORT_BITS, SHORT_SENT = 96, 40                     # ... and the other half: A sends 40 bytes and claims 12
SHORT_SWEEP = [0.25 * i for i in range(32)]         # B's symbol 0 against A's transmitted last symbol + 1
COLLIDE_SWEEP = [-56.0 + 0.25 * i for i in range(320)]
TRAIN_LENGTHS = (2, 3, 4, 5, 6, 7, 9)
TRAIN_OVERLAPS = (46.0, 44.0, 40.0, 36.5)           # plane samples a follower's symbol 0 lies in front of the last symbol + 1 of the burst before
#                                                     it: the oracle takes the followers at counts of 61 .. 67; at 44 and 40 it takes every train whole, at 46 and
#                                                     36.5 the stale word fires behind some bursts and breaks their trains (tests/test_chain_craft.py prints which)
TRAIN_NEXT = (5, 44.0, -30.0)                       # the train of this length and overlap is followed by one more burst at this offset: count 68 .. 72
ROWS2, ROWS8 = synth.ROW_BITS + 160, 7 * synth.ROW_BITS + 160     # swallow: length fields of two rows and of eight


def _al(i: int) -> int:
    """the alignment of step i of a sweep in quarter samples: the four fractions of the sweep meet each of the eight alignments"""
    return (i + i // 4) % 8


def _pair(name, i, sweep, a_kw, anchor, off, b_payload=P14):
    a = Link(family=name, step=i, align=_al(i), label=f"{sweep}:{off:+.2f}", sweep=sweep, param=off, role="A", **a_kw)
    b = Link(family=name, step=i, label=a.label, sweep=sweep, param=off, role="B", payload=b_payload, anchor=anchor, offset=off, tail=PC.TAIL)
    return [a, b]


def _train(name, i, n, overlap, align, next_off=None):
    g = []
    for k in range(n):
        last = k == n - 1 and next_off is None
        g.append(Link(family=name, step=i, align=align, label=f"train{n}/{overlap}", sweep=f"train{n}", param=overlap, role=f"f{k}",
                      payload=payload_bytes(12 + k, seed=i), anchor="sent" if k else "", offset=-overlap if k else 0.0,
                      tail=PC.TAIL if last else 0))
    if next_off is not None:
        g.append(Link(family=name, step=i, label=g[0].label, sweep="next", param=next_off, role="next", payload=payload_bytes(12 + n, seed=i),
                      anchor="sent", offset=next_off, tail=PC.TAIL))
    return g


# swallow: (claimed length field, alignment, offset of the burst across the claimed end).  A sends P12; `in1` .. `in3` follow its
# transmitted end and each other 24 .. 120 samples apart, wholly inside the claimed time; `across` is a step of the `claim` sweep;
# `behind` follows what `across` sent (lost or not, its samples are there) by SWALLOW_BEHIND samples.
SWALLOW = [(ROWS2, a, off) for a, off in zip(ALIGNS, (-44.0, -7.75, -30.5, -12.25, -50.0, -3.0, -21.5, -9.0))] + \
          [(ROWS8, 1, -40.25), (ROWS8, 6, -8.5)]
SWALLOW_IN = (120.0, 24.0, 57.25)
SWALLOW_BEHIND = 40.0


def _swallow(name, i, bits, align, off):
    lab = f"rows{bits // synth.ROW_BITS + 1}:{off:+.2f}"
    kw = dict(family=name, step=i, label=lab, sweep=lab.split(":")[0], param=off)
    g = [Link(align=align, role="A", payload=P12, length_bits=bits, **kw)]
    nin = 2 + i % 2
    for k in range(nin):
        g.append(Link(role=f"in{k + 1}", payload=payload_bytes(12 + k, seed=40 + i), anchor="sent", offset=SWALLOW_IN[k], **kw))
    g.append(Link(role="across", payload=P14, anchor="claim", ref=0, offset=off, **kw))
    g.append(Link(role="behind", payload=payload_bytes(13, seed=60 + i), anchor="sent", offset=SWALLOW_BEHIND, tail=PC.TAIL, **kw))
    return g


# stale: bursts without a tail behind which the OLD sync word fires again: the detector does not touch its ring of 68 phases during
# a burst, so each of its first three evaluations afterwards fits the old word with one new phase.  Every group is A = payload_bytes(n,
# seed) and a real burst B whose symbol 0 lies STALE_FOLLOW[k % 3] samples behind A's last symbol + 1, k = 40 (n - 12) + seed (B's ramp
# is part of what the three evaluations see, so B is in place during the search).  Which instants the detector evaluates behind A
# depends on the class it met A in, and that is left by the group before: a group found alone does not behave the same elsewhere.
# So the family IS the search, n = 12 .. 15, seed = 0 .. 39 IN THIS ORDER, and the tables hold what the oracle found in it
# (stale_found(); tests/test_chain_craft.py asserts that it still finds exactly this):
#   STALE_REJECTED   (n, seed): a trigger at a count of 3 or less whose header the receiver refuses, and B is then taken, met by a
#                    detector that has a refused header AND a burst behind it
#   STALE_ACCEPTED   (n, seed, length the stale header decoded to): ... accepts, with whatever length came out; B lies inside the time
#                    it claims and must be lost.  (The search found some; were this list empty, it would have found none.)
# In the other groups nothing fires behind A, and B simply follows it at a count of 97 .. 113.
STALE_REJECTED: List[tuple] = [(12, 11), (12, 12), (12, 15), (12, 18), (13, 3), (13, 11), (13, 26), (14, 7), (14, 12), (14, 20), (14, 36), (14, 39), (15, 7), (15, 10),
                                (15, 31), (15, 35), (15, 36), (15, 39)]
STALE_ACCEPTED: List[tuple] = [(12, 19, 15578), (12, 22, 15578), (13, 39, 15578), (14, 23, 15578), (15, 28, 15578)]
STALE_FOLLOW = (24.0, 40.0, 56.0)
STALE_NS, STALE_SEEDS = range(12, 16), range(40)


def _stale_group(n, s):
    k = 40 * (n - 12) + s
    kw = dict(family="stale", step=k, label=f"{n}/{s}", sweep="search", param=float(n))
    return [Link(align=k % 8, role="A", payload=payload_bytes(n, seed=s), **kw),
            Link(role="B", payload=P14, anchor="sent", offset=STALE_FOLLOW[k % 3], tail=PC.TAIL, **kw)]


def stale_found(j: PC.Judged):
    """(rejected, accepted) as the tables hold them"""
    rej, acc = [], []
    for a, b in groups_of(j.plane):
        n, s = (int(v) for v in a.label.split("/"))
        blk = block_of(j, a)
        st = [t for t in j.triggers if blk is not None and 0 < t["dec_index"] - blk.end_dec <= 6]
        if st and st[0]["accepted"] == 1:
            acc.append((n, s, int(st[0]["len_bits"])))
        elif st and block_of(j, b) is not None:
            rej.append((n, s))
    return rej, acc


def family_groups(name: str) -> List[List[Link]]:
    if name == "claim":
        g = [_pair(name, i, "long", dict(payload=P12, length_bits=CLAIM_BITS), "claim", off) for i, off in enumerate(CLAIM_SWEEP)]
        g += [_pair(name, len(CLAIM_SWEEP) + i, "short", dict(payload=payload_bytes(SHORT_SENT), length_bits=SHORT_BITS), "sent", off)
              for i, off in enumerate(SHORT_SWEEP)]
        return g
    if name == "collide":
        return [_pair(name, i, "collide", dict(payload=P12), "sent", off) for i, off in enumerate(COLLIDE_SWEEP)]
    if name == "train":
        g, i = [], 0
        for n in TRAIN_LENGTHS:
            for ov in TRAIN_OVERLAPS:
                g.append(_train(name, i, n, ov, i % 8, TRAIN_NEXT[2] if (n, ov) == TRAIN_NEXT[:2] else None))
                i += 1
        return g
    if name == "swallow":
        return [_swallow(name, i, *row) for i, row in enumerate(SWALLOW)]
    if name == "stale":
        return [_stale_group(n, s) for n in STALE_NS for s in STALE_SEEDS]
    raise KeyError(name)


# family -> {group: plane samples}, from settle(): stale sync words whose header the oracle accepted, and the length that came out
RESERVE: Dict[str, Dict[int, int]] = {
    "claim": {42: 5280, 54: 22400, 105: 35768, 137: 42632, 141: 20872, 161: 4816, 163: 4816, 165: 4816, 167: 4816, 233: 18496},
    "collide": {148: 4816},
    "stale": {19: 42008, 22: 42008, 79: 42008, 103: 42008, 148: 42008},         # the groups of STALE_ACCEPTED: eight rows each
}

_cache: Dict[str, PC.Plane] = {}
_judged: Dict[str, PC.Judged] = {}


def family(name: str) -> PC.Plane:
    """the family's plane (built once per process; treat it as read-only)"""
    if name not in _cache:
        _cache[name] = layout(name, family_groups(name), NOISE, 100 + FAMILIES.index(name), RESERVE.get(name, {}))
    return _cache[name]


def run_oracle(pl: PC.Plane) -> PC.Judged:
    from oracle import oracle as O
    ch = O.OracleChannel(PC.RATE, PC.FO[0], PC.FC + PC.FO[0], tap_dec=True, sdrclk=PC.SDRCLK)
    ch.feed(pl.raw(), "cf32")
    j = PC.Judged(pl, ch.dec(), ch.triggers(), ch.blocks())
    ch.close()
    return j


def unsettled(j: PC.Judged) -> Dict[int, int]:
    """group -> the reserve it needs: every header the oracle accepted, a case's or a stale word's, keeps the receiver busy for the length
    that came out, and the next group must find the detector history-free.  Empty when RESERVE holds what it must."""
    gs = groups_of(j.plane)
    starts = [int(g[0].t0) - 4 * SPS for g in gs]
    out: Dict[int, int] = {}
    for t in j.triggers:
        if t["accepted"] != 1:
            continue
        gi = max(0, int(np.searchsorted(starts, t["dec_index"], side="right")) - 1)
        busy_to = t["dec_index"] + SPS * (PC.busy_symbols(t["len_bits"]) - HEAD0 + 2)       # (the trigger lies half a symbol in front of symbol 21)
        nxt = starts[gi + 1] if gi + 1 < len(gs) else len(j.plane.plane) - 512 + 4 * SPS
        if busy_to + GAP > nxt + 4 * SPS:
            out[gi] = max(out.get(gi, 0), (busy_to - group_end(gs[gi]) + 7) // 8 * 8)
    return out


def settle(name: str, rounds: int = 40) -> Dict[int, int]:
    """how RESERVE[name] is found: lay out, ask the oracle, grow the reservations until nothing changes"""
    groups, res = family_groups(name), dict(RESERVE.get(name, {}))
    for _ in range(rounds):
        j = run_oracle(layout(name, groups, NOISE, 100 + FAMILIES.index(name), res))
        more = {g: v for g, v in unsettled(j).items() if v > res.get(g, 0)}
        if not more:
            return res
        res.update(more)
    raise AssertionError(f"{name}: the layout does not settle")


def judge(name: str) -> PC.Judged:
    """the family's plane through the oracle (once per process; read-only)"""
    if name not in _judged:
        _judged[name] = run_oracle(family(name))
    return _judged[name]


def count(j: PC.Judged, t) -> Optional[float]:
    """(the trigger's dec_index - the previous block's end_dec) / 2; None in front of the first block"""
    ends = [b.end_dec for b in j.blocks if b.end_dec < t["dec_index"]]
    return (t["dec_index"] - max(ends)) / 2.0 if ends else None


def met_in(j: PC.Judged, t) -> Optional[int]:
    """the FIR sub-phase the detector idled in when it met the trigger: the one the trigger before it left (clk mod 4)"""
    prev = [x for x in j.triggers if x["dec_index"] < t["dec_index"]]
    return prev[-1]["clk"] % 4 if prev else None


def groups_of(pl: PC.Plane) -> List[List[Link]]:
    out: List[List[Link]] = []
    for c in pl.cases:
        if c.group == len(out):
            out.append([])
        out[c.group].append(c)
    return out


def block_of(j: PC.Judged, c: Link):
    """the block the oracle made of the case (its chain took a trigger on the case's sync word and accepted the header), or None"""
    t = j.sync_trigger(c)
    if t is None or t["accepted"] != 1:
        return None
    return next((b for b in j.blocks if b.trig_dec == t["dec_index"]), None)


SERIAL_BELOW = 4096         # VDL2_SERIAL_BELOW: pushes of at most this many 84 kS/s frames go to the serial machine directly


def cut_windows(j: PC.Judged) -> Dict[str, List[tuple]]:
    """where a push cut makes the resolver carry its state: open intervals of plane samples, by kind
        "fresh"   behind a burst, 1 .. 67 evaluations after its end, in front of a follower the oracle then takes at a count below 68
        "header"  between such a follower's trigger and the last symbol of its header
        "fifth"   between the end of a train's fourth burst and the trigger of its fifth (trains the oracle takes whole)"""
    out: Dict[str, List[tuple]] = {"fresh": [], "header": [], "fifth": []}
    ends = sorted(b.end_dec for b in j.blocks)
    for g in groups_of(j.plane):
        blks = [block_of(j, c) for c in g]
        for k in range(1, len(g)):
            if blks[k] is None:
                continue
            trig = blks[k].trig_dec
            c = count(j, j.sync_trigger(g[k]))
            if not 1 <= c < STEADY:
                continue
            end = max(e for e in ends if e < trig)
            out["fresh"].append((end + 2, trig))
            out["header"].append((trig, trig + 8 * SPS))
            if g[k].role == "f4" and all(blks[:5]):
                out["fifth"].append((end + 2, trig))
    if not out["fifth"]:
        del out["fifth"]
    return {k: sorted(v) for k, v in out.items()}


def cutting_blocks(j: PC.Judged) -> List[int]:
    """odd block sizes in input samples for Receiver.run, every one longer than 2 * VDL2_SERIAL_BELOW so that the parallel path runs,
    which between them put a cut into a window of every kind of cut_windows(); one size where one does it"""
    win = cut_windows(j)
    n_in = 2 * len(j.plane.plane)
    first: Dict[str, int] = {}
    for blk in range(2 * SERIAL_BELOW + 1, 60001, 2):
        p = np.arange(blk, n_in, blk) / 2.0
        hit = set()
        for kind, w in win.items():
            lo, hi = np.array([x[0] for x in w], np.float64), np.array([x[1] for x in w], np.float64)
            i = np.searchsorted(lo, p, side="left") - 1         # the last window that starts in front of the cut
            if ((i >= 0) & (p > lo[np.maximum(i, 0)]) & (p < hi[np.maximum(i, 0)])).any():
                hit.add(kind)
                first.setdefault(kind, blk)
        if hit == set(win):
            return [blk]
    assert set(first) == set(win), f"no block size cuts {set(win) - set(first)}"
    return sorted(set(first.values()))
