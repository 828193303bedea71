"""Crafted 84 kS/s planes handed to the sync scan and the demodulator through the public ABI (CPU only: numpy, no GPU import).

At 100 kS/s with SDRCLK 42, one channel at Fo = 0 and cf32 input the channeliser is an exact identity once every plane sample
is written twice: each dump window of the integrate-and-dump is then exactly two inputs, the LO table is 1 + 0j, x + x is exact
and / 2 is exact (`wrap`).  So a test can hand the scan, the header decode and the slicers ANY plane it likes and let the oracle
judge what comes out.  (200 kS/s with SDRCLK 42 behaves the same; SDRCLK 63 with samples written three times is not exact.)

    wrap(plane)        complex64 plane -> raw cf32 at RATE / SDRCLK / FO
    Case               one burst at plane rate: per-symbol phase offsets and amplitudes, timing in fractions of a plane sample,
                       carrier offset, the header's 25 transmitted bits or its length field replaced
    layout(cases, ..)  many cases in one plane, far enough apart that the detector is history-free again before each
    family(name)       the deterministic sweeps below, every step at eight alignments (t0 shifted by 0 .. 7 plane samples)

Symbols of a burst (synth.burst_increments): 0 .. 3 ramp, 4 .. 20 the seventeen symbols of the sync word, 21 .. 29 the header
(25 bits and the first two of the payload; the receiver zeroes the first three soft bits, so symbol 21 carries nothing), then
the payload.  Bit q of the on-air stream behind the sync word is tribit q % 3 of symbol 21 + q // 3.
"""
from __future__ import annotations

import dataclasses
import math
from typing import Dict, List, Optional, Sequence

import numpy as np

from vdlm2dec_amd import synth

RATE = 100_000
SDRCLK = 42
FO = (0,)
FC = 136_975_000
PLANE_RATE = 84_000.0
SPS = 8                     # plane samples per symbol
AMP = 32.0
NOISE = 0.004               # sigma per component of the low floor (-78 dB below a burst)
SYNC0, SYNC_N, HEAD0, PAY0 = 4, 17, 21, 30
ALIGNS = tuple(range(8))
TAIL = 2
FRAC = (0.0, 0.25, 0.5, 0.75, 0.75, 0.25, 0.0, 0.5)   # ... and by this fraction of one on top: between bursts the detector idles in the FIR
#                             sub-phase the previous burst's timing left it in, so whole-sample shifts alone would keep the chain in one
#                             sub-phase for ever; with these every burst is met from a sub-phase 0, 1, 2 or 3 quarter samples off its own
GAP = 344                   # plane samples between a burst's last pulse and the next burst's first: the 68 evaluations (136 samples)
#                             the detector still sees pre-burst phases in, a sync word (136) and slack
TRIG_LO, TRIG_HI = 150, 200  # the detector fires this far behind symbol 0's centre (sync word's last symbol + filter delay + one step)

FAMILIES = ("outlier", "zigzag", "bend", "cfo", "notch", "plateau", "deep", "header", "header_words", "lengths", "slicer", "edge")
SCAN_FAMILIES = FAMILIES[:6]        # the ones whose sweep must cross the detector threshold


def wrap(plane: np.ndarray) -> np.ndarray:
    """complex64 plane -> interleaved cf32 at 100 kS/s, every plane sample written twice"""
    p = np.ascontiguousarray(plane, np.complex64)
    return np.repeat(p, 2).view(np.float32).copy()


def payload_bytes(n: int, seed: int = 1) -> bytes:
    return bytes(np.random.default_rng(1000 + 7 * n + seed).integers(0, 256, n, dtype=np.uint8).tolist())


def busy_symbols(length_bits: int) -> int:
    """symbols from symbol 0 to the last one a receiver takes for a header of this length (0: it refuses the header)"""
    ln = length_bits
    nbrow, nlbyte = ln // synth.ROW_BITS + 1, (ln % synth.ROW_BITS + 7) // 8
    if ln < 96 or nbrow > 8:
        return 0
    nd = (nbrow - 1) * 249 + (nlbyte if nlbyte else 249)
    nf = 6 * (nbrow - 1) + (0 if nlbyte <= 2 else (2 if nlbyte <= 30 else (4 if nlbyte <= 67 else 6)))
    return HEAD0 + (25 + 8 * (nd + nf) + 2) // 3


@dataclasses.dataclass
class Case:
    family: str
    step: int                               # index along the family's sweep
    align: int = 0                          # t0 shifted by so many whole plane samples
    label: str = ""
    sweep: str = ""                         # which of the family's sweeps the step belongs to (neighbouring steps of one sweep are neighbours)
    payload: bytes = b""
    phase: Optional[np.ndarray] = None      # radians added to symbol k's phase, k < len(phase); the last value holds from there on
    amp: Optional[Dict[int, float]] = None  # symbol index -> amplitude factor
    dt: float = 0.0                         # t0 shifted by a fraction of a plane sample
    frac: Optional[float] = None            # the alignment's own fraction (None: FRAC[align])
    cfo: float = 0.0                        # Hz
    head25: Optional[Sequence[int]] = None  # the header's 25 transmitted bits before scrambling
    length_bits: Optional[int] = None       # ... or its length field (parity computed)
    busy_bits: int = 0                      # the payload length the receiver will act on when that is not the transmitted one
    param: float = 0.0                      # the swept parameter, for reports
    reserve: int = 0                        # symbols (from symbol 0) the oracle has shown the receiver to stay busy for (settle)
    t0: float = 0.0                         # plane sample of symbol 0's pulse centre (layout)

    def bits(self) -> np.ndarray:
        b = synth.burst_bits(self.payload).copy()
        hb = None
        if self.length_bits is not None:
            hb = synth.header_bits(self.length_bits)
        if self.head25 is not None:
            hb = list(self.head25)
        if hb is not None:
            b[:25] = np.array(hb, np.uint8) ^ synth.pn_sequence(25)
        return b

    def symbols(self) -> np.ndarray:
        inc = synth.burst_increments(self.bits())
        ph = np.cumsum(inc) * (np.pi / 4.0)
        n = len(ph)
        if self.phase is not None:
            off = np.asarray(self.phase, np.float64)
            ph = ph + (off[:n] if len(off) >= n else np.concatenate([off, np.full(n - len(off), off[-1])]))
        # Two more symbols behind the last one the receiver takes, half a turn away from the sync word's last symbol.  The detector
        # does not touch its ring of 68 phases during a burst, so its first three evaluations afterwards fit the OLD sync word with one
        # new phase each; left to chance that phase fits in every third case, the stale word fires, a random header is decoded and the
        # receiver is busy through the cases that follow.  (The oracle and the GPU agree on such a trigger; it just is not the case.)
        ph = np.concatenate([ph, np.full(TAIL, ph[SYNC0 + SYNC_N - 1] + np.pi)])
        a = np.exp(1j * ph)
        a[-TAIL:] *= 4.0            # (louder than the payload: between two symbol centres the phase is then the tail's, not half way)
        for k, f in (self.amp or {}).items():
            a[k] *= f
        return a

    def nsym(self) -> int:
        return len(synth.burst_increments(synth.burst_bits(self.payload))) + TAIL

    def busy_sym(self) -> int:
        """symbols the receiver may stay busy for, counted from symbol 0: the transmitted burst, what the header it is expected to
        decode asks for, and what the oracle has shown it to take (settle)"""
        return max(self.nsym(), busy_symbols(self.acts_on()), self.reserve)

    def acts_on(self) -> int:
        """the length in bits the layout assumes the receiver decodes"""
        return self.busy_bits or (self.length_bits if self.length_bits is not None else 8 * len(self.payload))

    def trig_window(self):
        t = int(math.floor(self.t0))
        return t + TRIG_LO, t + TRIG_HI


def render(acc: np.ndarray, c: Case) -> None:
    """add the burst into acc (complex128, plane rate); symbol k's pulse centre at plane sample c.t0 + 8 k"""
    a = c.symbols()
    n = len(a)
    lo = max(0, int(math.floor(c.t0 - 4 * SPS)))
    hi = min(len(acc), int(math.ceil(c.t0 + (n - 1 + 4) * SPS)) + 1)
    t = np.arange(lo, hi, dtype=np.float64)
    u = (t - c.t0) / SPS
    kc = np.floor(u).astype(np.int64)
    s = np.zeros(len(t), np.complex128)
    for j in range(-4, 6):
        k = kc + j
        ok = (k >= 0) & (k < n)
        s += np.where(ok, a[np.clip(k, 0, n - 1)] * synth.rc_pulse(u - k), 0.0)
    if c.cfo:
        s *= np.exp(2j * np.pi * c.cfo * (t - c.t0) / PLANE_RATE)
    acc[lo:hi] += AMP * s


@dataclasses.dataclass
class Plane:
    name: str
    plane: np.ndarray           # complex64
    cases: List[Case]

    def raw(self) -> np.ndarray:
        return wrap(self.plane)

    def case_of(self, dec_index: int) -> Optional[Case]:
        for c in self.cases:
            lo, hi = c.trig_window()
            if lo <= dec_index < hi:
                return c
        return None


def layout(name: str, cases: List[Case], noise: float = NOISE, seed: int = 0) -> Plane:
    """the cases one after the other; noise = 0: exact zeros between them.  The floor is drawn per case (seed, index of the case), from
    half a gap in front of it: a case sees the same floor wherever the cases before it put it."""
    pos = 512
    for c in cases:
        c.t0 = float((pos + 4 * SPS + 7) // 8 * 8 + c.align) + (FRAC[c.align] if c.frac is None else c.frac) + c.dt
        pos = int(math.ceil(c.t0)) + (c.busy_sym() + 4) * SPS + GAP
    n = pos + 512
    acc = np.zeros(n, np.complex128)
    for c in cases:
        render(acc, c)
    if noise > 0:
        cut = [0] + [int(c.t0) - 4 * SPS - GAP // 2 for c in cases[1:]] + [n]
        for i in range(len(cases)):
            rng = np.random.default_rng([seed, i])
            m = cut[i + 1] - cut[i]
            acc[cut[i]:cut[i + 1]] += noise * (rng.standard_normal(2 * m).view(np.complex128))
    return Plane(name, acc.astype(np.complex64), cases)


def settle(name: str, cases: List[Case], noise: float, seed: int, rounds: int = 40) -> Plane:
    """layout(), then ask the oracle what each case's header made the receiver do: a header that decodes to another length than the
    one sent keeps the receiver busy for THAT long, and the cases behind it must wait for it (header_words: which codeword a flipped
    header lands on depends on soft bits a few hundredths apart, and on the class the detector met the burst in).  A case's
    reservation only ever grows, so this ends; RESERVE below holds where it ended, which makes it one round."""
    from oracle import oracle as O
    for c in cases:
        c.reserve = max(c.reserve, RESERVE.get((name, c.label, c.align), 0))
    for _ in range(rounds):
        pl = layout(name, cases, noise, seed)
        ch = O.OracleChannel(RATE, FO[0], FC + FO[0], sdrclk=SDRCLK)
        ch.feed(pl.raw(), "cf32")
        changed = False
        for t in ch.triggers():
            c = pl.case_of(t["dec_index"])
            need = busy_symbols(t["len_bits"]) if t["accepted"] == 1 else 0
            if c is None and need:      # a trigger behind a case (the stale sync word again, where a tail did not help) whose header was accepted
                c = max((x for x in pl.cases if x.t0 <= t["dec_index"]), key=lambda x: x.t0, default=None)
                need += int(t["dec_index"] - c.t0) // SPS - HEAD0 + 4 if c is not None else 0
            if c is not None and need > c.busy_sym():
                c.reserve, changed = need, True
        ch.close()
        if not changed:
            return pl
    raise AssertionError(f"{name}: the layout does not settle")


RESERVE: Dict[tuple, int] = {      # (family, label, alignment) -> symbols, from a settled run
    ("outlier", "outlier_last:2.2229", 5): 1032,
    ("header", "tie67", 0): 3107,
    ("header_words", "flip4", 3): 758, ("header_words", "flip4", 5): 758, ("header_words", "flip4", 6): 75,
    ("header_words", "flip6", 0): 72, ("header_words", "flip6", 1): 72, ("header_words", "flip6", 2): 72, ("header_words", "flip6", 3): 75, ("header_words", "flip6", 4): 75, ("header_words", "flip6", 5): 72, ("header_words", "flip6", 6): 72, ("header_words", "flip6", 7): 72,
    ("header_words", "flip9", 5): 2851,
    ("header_words", "flip12", 0): 947, ("header_words", "flip12", 5): 947,
    ("header_words", "flip15", 0): 1816, ("header_words", "flip15", 5): 2168,
    ("header_words", "flip21", 0): 70, ("header_words", "flip21", 1): 70, ("header_words", "flip21", 3): 70, ("header_words", "flip21", 4): 70, ("header_words", "flip21", 6): 70, ("header_words", "flip21", 7): 70,
    ("header_words", "flip20+21", 0): 766, ("header_words", "flip20+21", 3): 766, ("header_words", "flip20+21", 5): 766, ("header_words", "flip20+21", 6): 766,
    ("header_words", "other_len", 0): 950, ("header_words", "other_len", 3): 950, ("header_words", "other_len", 5): 950, ("header_words", "other_len", 6): 950,
    ("lengths", "row", 2): 6560, ("lengths", "row", 7): 6560,
}


# ------------------------------------------------------------------------------------------------------------- the families
P12 = payload_bytes(12)
P40 = payload_bytes(40)
LEN12 = 96


def _sync_phase(offsets: Dict[int, float], ramp_from: Optional[int] = None, slope: float = 0.0) -> np.ndarray:
    """per-symbol phase for symbols 0 .. 20 (0 from 21 on unless a ramp runs on): sync symbol l is symbol 4 + l"""
    ph = np.zeros(PAY0 + 400)
    for l, v in offsets.items():
        ph[SYNC0 + l] += v
    if ramp_from is not None:
        k = np.arange(len(ph))
        ph += np.where(k > SYNC0 + ramp_from, slope * (k - SYNC0 - ramp_from), 0.0)
        return ph
    return ph[:PAY0]


def _aligned(family: str, steps) -> List[Case]:
    """every step at the eight alignments; steps: [(label, param, dict of Case fields)]"""
    out = []
    for i, (label, param, kw) in enumerate(steps):
        for a in ALIGNS:
            out.append(Case(**{"family": family, "step": i, "align": a, "label": label, "sweep": label.split(":")[0], "param": param, "payload": P12, **kw}))
    return out


def _steps(kind: str, values) -> list:
    out = []
    for v in values:
        if kind.startswith("outlier"):
            l = {"outlier_first": 0, "outlier_mid": 8, "outlier_last": 16}[kind]
            out.append((f"{kind}:{v:.4f}", v, dict(phase=_sync_phase({l: v}))))
        elif kind == "zigzag":
            out.append((f"zigzag:{v:.4f}", v, dict(phase=_sync_phase({l: (v if l % 2 else -v) for l in range(SYNC_N)}))))
        elif kind == "bend":
            out.append((f"bend:{v:.4f}", v, dict(phase=_sync_phase({}, ramp_from=8, slope=v))))
        elif kind == "cfo":
            out.append((f"cfo:{v:.1f}", v, dict(cfo=float(v), phase=_sync_phase(CFO_BASE))))
        elif kind == "notch":
            out.append((f"notch:{v:.3g}", v, dict(amp={SYNC0 + 8: float(v)}, phase=_sync_phase({l: (ZZ if l % 2 else -ZZ) for l in range(SYNC_N)}))))
    return out


def _lin(a, b, n):
    return [float(x) for x in np.linspace(a, b, n)]


# The sweeps.  Each list is centred on where the ORACLE's detector stops firing for that shape (found once with the oracle; the
# coverage conditions of tests/test_plane_craft.py hold them there: a sweep that drifted off the threshold fails on the CPU).
ZZ = 0.479                 # zigzag amplitude that leaves the minimum of the fit error at 3.85 .. 3.95
SWEEPS = {
    "outlier": [("outlier_first", _lin(2.22, 2.42, 8)), ("outlier_mid", _lin(2.02, 2.19, 8)), ("outlier_last", _lin(2.12, 2.30, 8))],
    "zigzag": [("zigzag", _lin(0.45, 0.495, 16))],
    "bend": [("bend", _lin(0.345, 0.405, 16))],
    # a carrier offset alone never stops the detector (the fit takes the slope out; the oracle fires up to +-5250 Hz, where the phase
    # step per symbol passes pi): the sweep rides on an outlier on the sync word's last symbol that puts the minimum at 3.85
    "cfo": [("cfo", [0.0, 600.0, -600.0, 1200.0, -1200.0, 1800.0, -1800.0] + _lin(1900.0, 2500.0, 6) + _lin(-3000.0, -4800.0, 9))],
    # ... and a notch in ONE symbol moves the minimum by 0.2 at most: it rides on a zigzag of ZZ
    "notch": [("notch", [1.0, 0.8, 0.6, 0.4, 0.3, 0.2, 0.15, 0.1, 0.07, 0.05, 0.03, 0.025, 0.02, 0.015, 1e-2, 1e-4, 1e-8, 0.0])],
    "deep": [("outlier_mid", _lin(2.06, 2.18, 5) + _lin(2.30, 2.90, 5)), ("zigzag", _lin(0.474, 0.490, 5) + _lin(0.52, 0.66, 5))],
}
CFO_BASE = {16: 2.21}
PLATEAU_OUTLIER = (2.04, 2.12)  # on the sync word's middle symbol: the minimum of the fit error sits at the detector's 4
HEADER_SYM, HEADER_SWEEP = 25, _lin(np.pi / 8 - 0.045, np.pi / 8 + 0.045, 24)
# (found by trying, for payloads of 12 .. 120 bytes, every weight-3 codeword of the (25,20) code whose places 3 .. 24 lie in three
# different symbols, with steps of +-0.392 rad (pi / 8: the middle of the 0.0245 rad wide table bin on the boundary) from those symbols on,
# one burst alone on exact zeros, and keeping what the oracle reports as: three soft bits exactly 0.5, syndrome of the hard word 0,
# decoded length != the hard word's length)
HEADER_TIES = [(65, (3, 10, 19), (1, 1, 1), ALIGNS), (67, (3, 11, 16), (1, -1, 1), (0, 5))]   # payload bytes, header bits, signs, alignments
SLICER_SWEEP = [0.0, np.pi / 8 - 0.03, np.pi / 8 - 0.012, float(np.float32(np.pi / 8)), np.pi / 8 + 0.012, np.pi / 8 + 0.03, np.pi / 8 + 0.06]
OTHER_LEN = 104             # header_words: a header that decodes to this length over a payload of LEN12 bits
LENGTHS = [     # (label, payload bytes or None, header length field or None, alignments, (nbrow, nlbyte) or None when rejected)
    ("shortest", 12, None, ALIGNS, (1, 12)),
    ("too_short", 12, 88, ALIGNS, None),
    ("too_long", 12, 8 * synth.ROW_BITS, ALIGNS, None),
    ("row-1", 248, None, (0, 3, 5, 6), (1, 248)),
    ("row", 249, None, (1, 2, 4, 7), (2, 0)),
    ("row+1", 250, None, (0, 3, 5, 6), (2, 1)),
    ("rows8_1byte", 7 * 249 + 1, None, (3,), (8, 1)),
    ("rows8_full", 7 * 249 + 248, None, (6,), (8, 248)),
]


# `edge`: the two margins of the sparse stages taken to the last bit, on exact zeros between the cases (nothing random anywhere).
# Every value was found by bisection with the oracle IN THIS ORDER, each case behind the ones before it (the class the detector meets a
# burst in is left by the burst before): "zz" a zigzag whose minimum is 4 less 5e-7, 2e-5, 2e-4, 2e-3, 2e-2 (fires) and just past 4
# (does not) -- what the fourth screen's margin of 0.25 over an estimate good to 0.02 must keep; "pl" the timing at which two
# neighbouring evaluations have the SAME fit error: err = perr + 1 ulp, perr = p2err bit for bit, then 4e-5, 4e-4, 4e-3 apart either
# way -- what the fifth screen's ordering margin of 0.1 must keep.  To find them again after a change to the builder: for case i, with
# cases 0 .. i-1 in place, bisect the zigzag amplitude between a value that fires and one that does not; bisect the timing between two
# values 1/32 sample apart whose triggers are two samples apart; then move off by the listed amounts (tests/test_plane_craft.py
# asserts what came out, so a stale table fails on the CPU).
EDGE = [("zz", 0.48397556875082504), ("zz", 0.4874051671167625), ("zz", 0.48740716711676246), ("zz", 0.4873961671167625),
        ("zz", 0.4873061671167625), ("zz", 0.4875061671167625), ("zz", 0.4864061671167625), ("pl", 1.5420286122802906),
        ("pl", 0.5420286122798927), ("pl", 1.5419986122798643), ("pl", 0.5420586122798643), ("pl", 1.5417286122798644),
        ("pl", 0.5423286122798643), ("pl", 1.5390286122798644), ("pl", 0.5450286122798643),
        # ... and the threshold zigzags again, (value, alignment, fraction): each is met in the sub-phase the one before it left, so that
        # the region scan and the verify pass (limit 4) see them, not only the probe's own class (limit 7): 4 less 2e-7 .. 5e-7 and 1.6e-4
        ("zz", 0.48191555193603997, 1, 0.25), ("zz", 0.48438751963474486, 2, 0.5), ("zz", 0.4843977142502282, 3, 0.75),
        ("zz", 0.48397380079034513, 5, 0.25), ("zz", 0.4876383418650924, 6, 0.5), ("zz", 0.4819072423867736, 7, 0.75),
        ("zz", 0.4873961671167625, 4, 0.0), ("zz", 0.4876483418650924, 0, 0.5)]


def _flip(bits, *pos):
    b = list(bits)
    for p in pos:
        b[p] ^= 1
    return b


def family_cases(name: str) -> List[Case]:
    if name in SWEEPS:
        steps = []
        for kind, vals in SWEEPS[name]:
            steps += _steps(kind, vals)
        return _aligned(name, steps)
    if name == "plateau":
        # the detector idles in the class the PREVIOUS burst's timing left it in, so what is swept is the timing of each case against
        # the one before it: t_j - t_(j-1) = (j mod 32) / 16 plane samples, every sixteenth of the two samples between evaluations;
        # two mild outliers: with the first the minimum between two evaluations still fires (err = perr + a little), with the second not
        out, t = [], 0.0
        for j in range(128):
            t = (t + (j % 32) / 16.0) % 8.0
            d = PLATEAU_OUTLIER[(j // 32) % 2]
            out.append(Case(family=name, step=j, align=int(t), dt=t - int(t), frac=0.0, label=f"t:{t:.4f}/{d}", sweep=f"plateau{j // 32}", param=t, payload=P12, phase=_sync_phase({8: d})))
        return out
    if name == "header":
        steps = []
        for v in HEADER_SWEEP:      # a phase step from symbol HEADER_SYM on: ONE differential phase moves, one soft bit crosses 0.5
            ph = np.zeros(HEADER_SYM + 1)
            ph[HEADER_SYM] = v
            steps.append((f"head:{v:.5f}", v, dict(phase=ph)))
        out = _aligned(name, steps)
        # Ties.  One soft bit on 0.5 cannot tie two codewords (they differ in three places at least); THREE can, where the three places
        # are a codeword of weight 3.  Then the metrics of two words are equal to the last bit (a factor 0.5 is exact in a double), the
        # reference's trellis keeps whichever survivor it met first, and the hard decisions -- all three 0 -- are a codeword too: the
        # only input on which the shortcut's gate |v - 0.5| < 1e-3 decides anything.  Found by search with the oracle: a payload
        # length and three phase steps of pi / 8 for which the trellis keeps the OTHER word (tests/test_plane_craft.py holds that).
        for i, (nbytes, places, signs, aligns) in enumerate(HEADER_TIES):
            ph = np.zeros(PAY0 + 1)
            for q, sg in zip(places, signs):
                ph[HEAD0 + q // 3:] += sg * 0.392
            for a in aligns:
                out.append(Case(family=name, step=len(steps) + i, align=a, label=f"tie{nbytes}", sweep="tie", param=float(nbytes),
                                payload=payload_bytes(nbytes), phase=ph))
        return out
    if name == "header_words":
        cw = synth.header_bits(LEN12)
        words = [("codeword", cw)] + [(f"flip{n}", _flip(cw, n)) for n in range(25)]
        # A clean symbol's soft bits are 0.002 .. 0.05 from their ends, so flipping a confident bit can cost the decoder more than
        # flipping two doubtful ones elsewhere: several single flips land on ANOTHER codeword, i.e. another length, and on which one
        # depends on the class the detector met the burst in.  The words that can keep the receiver busy for thousands of symbols
        # are placed at fewer alignments (settle() finds out how long; RESERVE holds it).
        words += [("flip20+21", _flip(cw, 20, 21)), ("flip5+17", _flip(cw, 5, 17)), ("other_len", _flip(synth.header_bits(OTHER_LEN), 12))]
        few = {"flip9": (0, 5), "flip12": (0, 5), "flip15": (0, 5), "flip4": (0, 3, 5, 6), "flip20+21": (0, 3, 5, 6), "other_len": (0, 3, 5, 6)}
        return [Case(family=name, step=i, align=a, label=lab, param=float(i), payload=P12, head25=w)
                for i, (lab, w) in enumerate(words) for a in few.get(lab, ALIGNS)]
    if name == "lengths":
        out = []
        for i, (lab, nbytes, field, aligns, _) in enumerate(LENGTHS):
            for a in aligns:
                out.append(Case(family=name, step=i, align=a, label=lab, param=float(nbytes), payload=payload_bytes(nbytes, seed=i), length_bits=field))
        return out
    if name == "edge":
        out = []
        for i, (kind, v, *where) in enumerate(EDGE):
            if kind == "zz":
                a, f = where or (0, 0.0)
                out.append(Case(family=name, step=i, align=a, frac=f, label=f"zz{i}", sweep="zz", param=v, payload=P12,
                                phase=_sync_phase({l: (v if l % 2 else -v) for l in range(SYNC_N)})))
            else:
                out.append(Case(family=name, step=i, align=int(v), frac=0.0, dt=v - int(v), label=f"pl{i}", sweep="pl", param=v, payload=P12,
                                phase=_sync_phase({8: 2.04})))
        return out
    if name == "slicer":
        steps = []
        for v in SLICER_SWEEP + [-x for x in reversed(SLICER_SWEEP)]:
            ph = np.zeros(PAY0 + 200)
            ph[PAY0 + 1::2] = v
            steps.append((f"slice:{v:+.6f}", v, dict(phase=ph, payload=P40)))
        return _aligned(name, steps)
    raise KeyError(name)


_cache: Dict[str, Plane] = {}


def family(name: str) -> Plane:
    """the family's plane (built once per process; treat it as read-only)"""
    if name not in _cache:
        zeros = name in ("notch", "lengths", "edge")        # the variant with exact zeros between the cases
        _cache[name] = settle(name, family_cases(name), 0.0 if zeros else NOISE, FAMILIES.index(name) + 1)
    return _cache[name]


@dataclasses.dataclass
class Judged:
    plane: Plane
    dec: np.ndarray             # the oracle's 84 kS/s tap
    triggers: list              # OracleChannel.triggers()
    blocks: list                # OracleChannel.blocks()

    def sync_trigger(self, c: Case):
        """the trigger the oracle's chain took on the case's sync word, or None"""
        lo, hi = c.trig_window()
        for t in self.triggers:
            if lo <= t["dec_index"] < hi:
                return t
        return None


_judged: Dict[str, Judged] = {}


def judge(name: str) -> Judged:
    """the family's plane through the oracle (once per process; read-only)"""
    if name not in _judged:
        from oracle import oracle as O
        pl = family(name)
        ch = O.OracleChannel(RATE, FO[0], FC + FO[0], tap_dec=True, sdrclk=SDRCLK)
        ch.feed(pl.raw(), "cf32")
        _judged[name] = Judged(pl, ch.dec(), ch.triggers(), ch.blocks())
        ch.close()
    return _judged[name]


def cutting_blocks(pl: Plane):
    """two block sizes in input samples for Receiver.run, each long enough for the parallel path: an ordinary one and an odd one one of
    whose cuts falls inside a sync word and another inside a header; for a plane too short for that, an odd one for each"""
    n_in = 2 * len(pl.plane)
    sync = head = None
    for blk in range(9801, 60001, 2):
        in_sync = in_head = False
        for cut in range(blk, n_in, blk):
            p = cut / 2.0
            for c in pl.cases:
                if c.t0 + SYNC0 * SPS + 8 < p < c.t0 + (SYNC0 + SYNC_N - 1) * SPS - 8:
                    in_sync = True
                if c.t0 + (HEAD0 + 1) * SPS < p < c.t0 + (PAY0 - 1) * SPS:
                    in_head = True
        if in_sync and in_head:
            return 32768, blk
        sync = sync or (blk if in_sync else None)
        head = head or (blk if in_head else None)
    if sync and head:
        return sync, head
    raise AssertionError("no block size cuts a sync word and a header")
