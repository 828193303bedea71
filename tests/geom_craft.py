"""Crafted planes for the payload decode: one clean burst at every burst geometry the receiver's byte schedule distinguishes, and
copies of one burst whose last symbol, header and trigger are walked frame by frame across the end of a push (CPU only: numpy).

The rig is plane_craft's exact identity (100 kS/s, SDRCLK 42, Fo 0, cf32, every plane sample written twice), so the oracle judges
every plane; tests/test_geom_craft.py asserts against the oracle alone that the planes sit where they aim.

    takes(nbrow, nlbyte)    (ND, NF): the data and parity bytes the receiver takes for a header, by the reference's rules
    plane(name) / judge(name)
        "geom"          nbrow 1 .. 8 x the last row's byte counts either side of every parity threshold, the bytes of each payload
                        random, exact zeros between the cases; then the byte counts either side of the lane strides, then one
                        geometry at every alignment and quarter sample (the timing classes: j0 of burst_timing)
        "geom_frames"   the same geometries with nlbyte != 0, each payload one real frame and flag fill, one byte of the last row
                        flipped on the air wherever the reference decodes that row
        "edge_cut:F"    copies of one burst placed against the multiples of F frames (EDGE_SWEEPS)

A header of nbrow rows with nlbyte 0 is sent for a payload of (nbrow - 1) * 249 bytes; the receiver then reads a whole last row
the transmitter never sent (plane_craft.busy_symbols reserves it), out of the tail symbols and the zeros behind them."""
from __future__ import annotations

import dataclasses
from typing import Dict, List, Optional, Tuple

import numpy as np

import plane_craft as PC
from plane_craft import GAP, SPS, payload_bytes
from vdlm2dec_amd import synth

NBROWS = tuple(range(1, 9))
NLBYTES = (0, 1, 2, 3, 4, 29, 30, 31, 32, 66, 67, 68, 69, 247, 248)       # either side of 2|3, 30|31, 67|68, and both ends of a row
SHORTEST = 12               # bytes: a header that announces less is refused
STRIDES = (64, 256, 512)    # K2B_NT, K2_NT and twice that: lanes stride over the ND + NF bytes by the first two
# ND + NF on and either side of each stride.  The sweep itself gives 254, 256, 257, 509, 511, 512 and 515; these add 63, 64, 65 and 255.
# 255 is one row of 249 bytes, which only a length of 1985 .. 1991 BITS announces (a whole 249 bytes are two rows, the second empty):
# the case sends 249 bytes under a header of 1991 bits.  513 is no receiver's byte count at all (test_geom_craft goes through every
# accepted header): behind (3, 2) = 512 comes (3, 3) = 515, which gains two parity bytes with its row.
STRIDE_CASES = ((1, 59), (1, 60), (1, 61), (1, 249))
# one geometry at every alignment and at two quarter-sample fractions each: between them the detector meets it with every clk0 it
# shows anywhere in the plane (test_geom_craft holds that both the smallest and the largest j0 are among these)
TIMING_GEOM = (2, 30)
TIMING_FRACS = (0.0, 0.5)


def takes(nbrow: int, nlbyte: int) -> Tuple[int, int]:
    """(ND, NF) for an accepted header: data bytes are taken column by column over nbrow rows, the last row holding nlbyte of them
    (a whole row where nlbyte is 0); parity bytes the same way over the rows that have any: every full row has 6, the last row
    none up to 2 data bytes, 2 up to 30, 4 up to 67, else 6"""
    nd = (nbrow - 1) * 249 + (nlbyte if nlbyte else 249)
    last = 0 if nlbyte <= 2 else (2 if nlbyte <= 30 else (4 if nlbyte <= 67 else 6))
    return nd, 6 * (nbrow - 1) + last


def nsym_of(nbrow: int, nlbyte: int) -> int:
    """symbols from the header's first to the last one the receiver takes: 25 header bits and 8 (ND + NF) more, three to a symbol"""
    nd, nf = takes(nbrow, nlbyte)
    return (25 + 8 * (nd + nf) + 2) // 3


def sent_bytes(nbrow: int, nlbyte: int) -> int:
    return (nbrow - 1) * 249 + nlbyte


@dataclasses.dataclass
class GCase(PC.Case):
    nbrow: int = 0
    nlbyte: int = 0
    corrupt: Optional[Dict[tuple, int]] = None      # (row, column) -> xor mask on the air (synth.burst_bits)

    def bits(self) -> np.ndarray:
        b = super().bits()
        if self.corrupt:
            b[25:] = synth.burst_bits(self.payload, self.corrupt)[25:]
        return b


def geometries(frames: bool = False) -> List[Tuple[int, int]]:
    """(nbrow, nlbyte) of the cases of `geom`; frames: of `geom_frames` (without the rows no transmitter fills)"""
    out = [(r, n) for r in NBROWS for n in NLBYTES if sent_bytes(r, n) >= SHORTEST and (n or not frames)]
    return out + [g for g in STRIDE_CASES if g[1] < 249 or not frames]


def frame_payload(n: int, seed: int) -> bytes:
    """one real frame, the longest whose flags, stuffed bits and FCS fit into n bytes, then flag fill to exactly n"""
    rng = np.random.default_rng(5000 + seed)
    info = bytes(rng.integers(0, 256, max(0, n - 13), dtype=np.uint8).tolist())
    while True:
        p = synth.hdlc_payload(synth.avlc_frame(info))
        if len(p) <= n:
            return p + b"\x7e" * (n - len(p))
        assert info, n
        info = info[:-1]


FLIP = 0x5a                 # geom_frames: xor mask on the last row's first byte


def _cases(name: str) -> List[GCase]:
    out = []
    for i, (r, n) in enumerate(geometries(name == "geom_frames")):
        nb = sent_bytes(r, n)
        kw = dict(family=name, step=i, align=i % 8, label=f"{r}x{n}", sweep=f"rows{r}", param=float(nb), nbrow=r, nlbyte=n,
                  length_bits=8 * nb - 1 if n == 249 else None)
        if name == "geom":
            out.append(GCase(payload=payload_bytes(nb, seed=i), **kw))
        else:
            out.append(GCase(payload=frame_payload(nb, i), corrupt={(r - 1, 0): FLIP} if n > 2 else None, **kw))
    if name == "geom":
        r, n = TIMING_GEOM
        for k, f in enumerate(TIMING_FRACS):
            for a in PC.ALIGNS:
                if f == PC.FRAC[a]:
                    continue        # (the sweep's own case at this alignment has that fraction)
                out.append(GCase(family=name, step=len(out), align=a, frac=f, label=f"{r}x{n}@{a}+{f}", sweep="timing", param=a + f,
                                 payload=payload_bytes(sent_bytes(r, n), seed=900 + 8 * k + a), nbrow=r, nlbyte=n))
    return out


# (plane, label, alignment) -> symbols the oracle has shown the receiver to stay busy for, from a settled run (plane_craft.RESERVE's
# role; settle() finds them again in a few rounds where this is stale or empty)
RESERVE: Dict[tuple, int] = {("geom", "2x0", 2): 6560, ("geom", "5x0", 7): 8600, ("geom", "6x0", 6): 9280, ("geom", "8x0", 4): 10640,
                            ("geom_frames", "2x248", 7): 2437}

_planes: Dict[str, PC.Plane] = {}
_judged: Dict[str, PC.Judged] = {}


def plane(name: str) -> PC.Plane:
    """built once per process; treat it as read-only"""
    if name not in _planes:
        if name.startswith("edge_cut:"):
            _planes[name] = edge_plane(int(name.split(":")[1]))
        else:
            cases = _cases(name)
            for c in cases:
                c.reserve = RESERVE.get((name, c.label, c.align), 0)
            _planes[name] = PC.settle(name, cases, 0.0, 0)
    return _planes[name]


def run_oracle(pl: PC.Plane) -> PC.Judged:
    from oracle import oracle as O
    ch = O.OracleChannel(PC.RATE, PC.FO[0], PC.FC + PC.FO[0], tap_dec=True, sdrclk=PC.SDRCLK)
    ch.feed(pl.raw(), "cf32")
    j = PC.Judged(pl, ch.dec(), ch.triggers(), ch.blocks())
    ch.close()
    return j


def judge(name: str) -> PC.Judged:
    """the plane through the oracle (once per process; read-only)"""
    if name not in _judged:
        _judged[name] = run_oracle(plane(name))
    return _judged[name]


def block_of(j: PC.Judged, c: PC.Case):
    """the block the oracle made of the case, or None"""
    t = j.sync_trigger(c)
    if t is None or t["accepted"] != 1:
        return None
    return next((b for b in j.blocks if b.trig_dec == t["dec_index"]), None)


def j0_of(clk0: int) -> int:
    """frames from the trigger to the first symbol the receiver takes (the reference advances its clock by 4 a frame until it passes 32)"""
    return max(1, (32 - clk0 + 3) // 4)


_soft: Dict[str, dict] = {}


def soft_maps(name: str) -> dict:
    """trig_dec -> (hard bytes, reliability map, mask of the bytes the receiver takes) of every block of the plane, the first two by
    tests/soft_ref.py on the oracle's tap (once per process)"""
    if name not in _soft:
        import soft_ref as R
        j = judge(name)
        clk = {t["dec_index"]: t["clk"] for t in j.triggers if t["accepted"] == 1}
        pn = R.pn_bits()
        out = {}
        for b in j.blocks:
            hard, rel = R.soft_block(j.dec, b.nbrow, b.nlbyte, b.df, b.trig_dec, clk[b.trig_dec], pn)
            nd, nf = takes(b.nbrow, b.nlbyte)
            taken = np.zeros((R.ROWS, R.ROWLEN), bool)
            for r in range(b.nbrow):        # data: whole rows and nlbyte of the last (a whole one at 0); parity: what is left of nf row by row
                last = r == b.nbrow - 1
                taken[r, :(b.nlbyte or 249) if last else 249] = True
                taken[r, 249:249 + (nf - 6 * (b.nbrow - 1) if last else 6)] = True
            assert int(taken.sum()) == nd + nf
            out[b.trig_dec] = (hard, rel, taken)
        _soft[name] = out
    return _soft[name]


# ------------------------------------------------------------------------------------------------------- a push's end
# A push of 2 F input samples is F frames of the plane, so with Receiver.run(raw, block=2 * F) the pushes end at the multiples of F.
# Every copy aims one of its stamps at a cut:
#   "end"    end_dec: the last symbol the receiver takes
#   "head"   nsym0 + 64: header symbol 8, the last one the header decode needs (nsym0 = end_dec - 8 (nsym - 1))
#   "trig"   trig_dec
# d = (the cut nearest to the stamp) - stamp: with d >= 1 the stamp's frame is d frames inside the push that ends at the cut, with
# d <= 0 it is the (1 - d)-th frame of the next push.  The detector evaluates every second frame and which ones depends on the burst
# before, so where a stamp lands is the oracle's to say: the copies aim at more values of d than must be covered.
SERIAL_BELOW = 4096         # VDL2_SERIAL_BELOW: pushes of at most this many frames go to the serial machine directly
LONGEST = sent_bytes(8, 248)
D_SHORT, D_LONG = 12, 4     # |d| that must be covered, every integer
AIM_SHORT, AIM_LONG = 14, 6  # |d| aimed at
# (payload bytes, stamp, |d| to cover) per F
EDGE_SWEEPS = {
    5000: [(n, s, D_SHORT) for n in (12, 13, 14) for s in ("end", "head", "trig")] + [(LONGEST, "end", D_LONG)],
    1376: [(LONGEST, "end", D_LONG)],       # the live path's 32768 samples at 2 MS/s
}
# stamp - t0 of a copy at a whole-sample t0, as the oracle shows them on these planes: the trigger 170 or 171 frames behind symbol 0's
# centre, the first symbol taken j0 = 5 .. 7 frames behind the trigger.  (Where a burst before leaves the detector in another class
# these move by a frame or two: AIM is wider than what must be covered, and test_geom_craft holds the coverage.)
TRIG_AT, NSYM0_AT = 171, 177


def _aim(n: int, stamp: str) -> int:
    """stamp - t0, about"""
    if stamp == "trig":
        return TRIG_AT
    if stamp == "head":
        return NSYM0_AT + 64
    return NSYM0_AT - (n == LONGEST) + SPS * (nsym_of(*synth.fec_layout(8 * n)[:2]) - 1)


def edge_plane(F: int) -> PC.Plane:
    cases: List[PC.Case] = []
    pos = 512
    for n, stamp, cover in EDGE_SWEEPS[F]:
        aim = AIM_SHORT if cover == D_SHORT else AIM_LONG
        pay = payload_bytes(n, seed=3)
        for d in range(-aim, aim + 1):
            c = PC.Case(family="edge_cut", step=len(cases), label=f"{n}/{stamp}:{d:+d}", sweep=f"{n}/{stamp}", param=float(d), payload=pay)
            off = _aim(n, stamp) + d
            cut = -(-(pos + 4 * SPS + off) // F) * F        # the first cut the copy can reach
            c.t0 = float(cut - off)
            pos = int(c.t0) + (c.busy_sym() + 4) * SPS + GAP
            cases.append(c)
    acc = np.zeros(-(-(pos + 512) // F) * F, np.complex128)
    for c in cases:
        PC.render(acc, c)
    return PC.Plane(f"edge_cut:{F}", acc.astype(np.complex64), cases)


def stamps(b) -> Dict[str, int]:
    """the three stamps of an oracle block (or a record: the same fields)"""
    nsym0 = b.end_dec - SPS * (nsym_of(b.nbrow, b.nlbyte) - 1)
    return {"end": b.end_dec, "head": nsym0 + 64, "trig": b.trig_dec}


def cut_of(stamp: int, F: int) -> Tuple[int, int]:
    """(the cut nearest to the stamp, d)"""
    cut = (stamp + F // 2) // F * F
    return cut, cut - stamp


def edge_rows(j: PC.Judged, F: int):
    """[(case, block, stamp name, cut, d)] of every copy the oracle made a block of"""
    out = []
    for c in j.plane.cases:
        b = block_of(j, c)
        if b is not None:
            name = c.sweep.split("/")[1]
            out.append((c, b, name) + cut_of(stamps(b)[name], F))
    return out
