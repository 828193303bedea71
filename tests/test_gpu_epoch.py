"""The same stream, late: handles of the test build created with a stream epoch T0 (VDL2GPU_TEST_EPOCH, include/vdl2gpu.h) must hand
out what the oracle gives for the stream from sample 0 with every instant moved by exactly T0 input samples / D0 = 21 T0 / SDRCLK
frames and nothing else changed, bit for bit -- with T0 chosen so that the stream crosses 2^31 or 2^32 input samples (in31, in32),
2^31 or 2^32 decimated frames (dec31, dec32), or lies behind 2^40 input samples (big40).  The reference is the oracle (and, where the
oracle cannot judge -- rates off the 25 kHz grid, VDL2GPU_F_EXACT_FO -- the numpy models the existing tests pin to it), never a
second handle at epoch 0.

Every case asserts on the CPU, from the oracle's stamps, that its first burst begins 2600 frames or more behind the stream's start,
that bursts are decoded on both sides of its boundary and that one is in flight across it (trigger before, last symbol behind), and on
the GPU which channeliser kernel ran (vdl2gpu_debug_k1).  tests/epoch_rule.py is the rule for T0, tests/test_epoch_cpu.py holds the
host's arithmetic at the same magnitudes without a GPU."""
import dataclasses
import types

import numpy as np
import pytest

import chain_craft as CC
import epoch_rule as E
import exactfo_model as X
import levels_ref as LR
import offgrid_model as M
import plane_craft as PC
import scenarios as S
import soft_ref as SR
import test_gpu_levels as TL
import test_gpu_offgrid_rates as G
import test_gpu_rates as TR
from test_gpu_planes import PATHS
from vdlm2dec_amd import lib, synth

pytestmark = pytest.mark.gpu

FIRST = 2600                # frames in front of the first burst: every noise block of every level lies inside the pushed stream
RAMP = 200                  # a burst begins less than this many frames in front of its trigger (21 symbols and the filter's delay)
MARGIN = 4000               # input samples: a burst that ends this close to a cut may come out with either push
PER = X.PER


@dataclasses.dataclass
class Ref:
    """a stream and what the yardstick makes of it from sample 0"""
    rate: int
    clk: int
    fmt: str
    fos: tuple
    raw: np.ndarray
    blocks: list            # oracle Blocks of every channel
    dec: dict               # channel -> 84 kS/s plane
    trig: dict              # channel -> OracleChannel.triggers() (oracle-judged streams only)
    sdrclk: int = 0         # what the handle is given (0: the default)

    @property
    def n(self):
        return self.raw.size // PER[self.fmt]


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _f32(v):
    return int(np.float32(v).view(np.uint32))


def _oracle_ref(O, raw, fmt, rate, fos, ofmt=None):
    blocks, dec, trig = [], {}, {}
    for c, fo in enumerate(fos):
        ch = O.OracleChannel(rate, fo, S.FC + fo, chn=c, tap_dec=True)
        ch.feed(raw, ofmt or fmt)
        blocks += ch.blocks()
        dec[c], trig[c] = ch.dec(), ch.triggers()
        ch.close()
    raw.setflags(write=False)
    return Ref(rate, rate // 4000, fmt, tuple(fos), raw, blocks, dec, trig)


def _model_ref(O, raw, fmt, rate, fos, planes):
    blocks = [b for c, (p, fo) in enumerate(zip(planes, fos)) for b in M.demod_blocks(O, p, S.FC + fo, chn=c)]
    raw.setflags(write=False)
    return Ref(rate, rate // 4000, fmt, tuple(fos), raw, blocks, dict(enumerate(planes)), {})


_refs = {}


def _cached(key, make):
    if key not in _refs:
        _refs[key] = make()
    return _refs[key]


# six bursts on two channels, the third a long one (what is in flight), overlapping in time across the channels
TWO_PLAN = [(0.035, 40), (0.052, 120), (0.080, 250), (0.150, 31), (0.165, 66), (0.190, 17)]
TWO_FO = (-50_000, 250_000)


def _two(O, fmt="cs16", seed=31, plan=TWO_PLAN):
    def make():
        spec = S.placed(2_000_000, TWO_FO, seed, plan, q=8000, nsamples=432_000)
        return _oracle_ref(O, synth.synth_stream(spec, fmt), fmt, 2_000_000, TWO_FO)
    return _cached(("two", fmt, seed), make)


def _crafted(name):
    """a crafted plane of the identity rig (tests/plane_craft.py, tests/chain_craft.py) behind 8 * 336 frames of zeros, judged anew"""
    def make():
        src = (PC if name in PC.FAMILIES else CC).family(name)
        plane = np.concatenate([np.zeros(8 * 336, np.complex64), src.plane])
        j = CC.run_oracle(PC.Plane(name, plane, src.cases))
        assert np.array_equal(_bits(j.dec), _bits(plane))
        raw = PC.wrap(plane)
        raw.setflags(write=False)
        return Ref(PC.RATE, PC.SDRCLK, "cf32", PC.FO, raw, j.blocks, {0: j.dec}, {0: j.triggers}, sdrclk=PC.SDRCLK)
    return _cached(("crafted", name), make)


# ------------------------------------------------------------------------------------------------------------ the epoch of a case
def _epoch(ref, bnd, quirk=False, pure_shift=False, q=None):
    """(the burst in flight, T0): the longest burst that is neither the first nor the last to trigger, and the largest admissible T0
    that puts the boundary behind its trigger -- asserted to cross it with that burst in flight"""
    q = q or E.quantum(ref.rate, ref.sdrclk, quirk, pure_shift)
    by_time = sorted(ref.blocks, key=lambda b: b.trig_dec)
    assert len(by_time) >= 3 and by_time[0].trig_dec - RAMP >= FIRST, by_time[0].trig_dec
    blk = max(by_time[1:-1], key=lambda b: b.end_dec - b.trig_dec)
    t0 = E.epoch_for(E.BOUNDARIES[bnd], blk.trig_dec, ref.clk, q)
    assert t0 > 0 and t0 % q == 0 and E.admissible(t0, ref.rate, ref.sdrclk, quirk)
    _assert_crossing(ref, bnd, t0, blk)
    return blk, t0


def _assert_crossing(ref, bnd, t0, blk=None):
    """from the yardstick's stamps: at epoch t0 bursts end before the boundary and trigger behind it, and one (blk, if given) is in
    flight across it; big40: everything lies behind 2^40"""
    before, across, after = E.crossing(E.BOUNDARIES[bnd], t0, ref.clk, ref.blocks)
    if bnd == "big40":
        assert t0 >= 1 << 40 and not before and not across and len(after) == len(ref.blocks) >= 3
        return
    assert before and after and across and (blk is None or blk in across), (bnd, t0, len(before), len(across), len(after))
    axis, value = E.BOUNDARIES[bnd]
    lo = t0 if axis == "in" else E.d0(t0, ref.clk)
    assert lo < value < lo + (ref.n if axis == "in" else 21 * ref.n // ref.clk)      # the boundary lies inside the pushed stream


def _env(monkeypatch, t0, general=False, rounds=None, ticket0=None):
    monkeypatch.setenv("VDL2GPU_TEST_EPOCH", str(t0))
    for name, v in (("VDL2GPU_NO_K1_FAST", "1" if general else None), ("VDL2GPU_REPAIR_ROUNDS", rounds),
                    ("VDL2GPU_TEST_TICKET0", None if ticket0 is None else str(ticket0))):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, v)


def _rx(ref, max_push, fos=None, **kw):
    from vdlm2dec_amd.demod import Receiver, plan_channels
    fos = ref.fos if fos is None else fos
    plan = [plan_channels(S.FC, f) for f in fos] if isinstance(fos[0], tuple) else plan_channels(S.FC, fos)
    return Receiver(ref.rate, plan, fmt=ref.fmt, sdrclk=ref.sdrclk, max_push=max_push, keep_dec=True, testhooks=True, **kw)


# ------------------------------------------------------------------------------------------------------------------- the cuttings
def _ragged(ref, blk):
    """five pushes or more of odd sizes: a cut in the middle of the burst in flight (it is deferred), a push shorter than
    VDL2_SERIAL_BELOW frames behind it, and the last cut 600 frames in front of the last trigger (the last push holds a whole burst)"""
    s = lambda m: E.dec_to_sample(m, ref.clk)       # noqa: E731
    mid = s((blk.trig_dec + blk.end_dec) // 2) | 1
    short = (CC.SERIAL_BELOW * ref.clk // 21 // 2) | 1
    last = s(max(b.trig_dec for b in ref.blocks) - 600) | 1
    cuts = [mid // 2 | 1, mid, mid + short]
    if last > cuts[-1] + short:
        cuts += [(cuts[-1] + last) // 2 | 1, last]
    sizes = np.diff([0] + cuts + [ref.n]).tolist()
    assert len(sizes) >= 4 and min(sizes) > 0 and sum(sizes) == ref.n
    assert 21 * short // ref.clk < CC.SERIAL_BELOW and sizes[2] == short
    return sizes


def _whole(ref, unit, parts):
    """pushes of whole units (superperiods, hand-off blocks), in the proportions `parts`"""
    u = ref.n // unit
    assert u * unit == ref.n
    k = [max(3, u * p // sum(parts)) for p in parts[:-1]]
    k.append(u - sum(k))
    assert k[-1] >= 3
    return [x * unit for x in k]


def _pushed(rx, ref, sizes, every=True, streams=None):
    """push the stream in parts; the planes put together from the parts' (every: read behind each push, which waits for it) or
    the last push's alone, and every record in hand-out order"""
    raws = [ref.raw] if streams is None else streams
    per = PER[ref.fmt]
    nch = len(ref.dec)
    parts, got, pos = {(s, c): [] for s in range(len(raws)) for c in range(nch)}, [], 0
    for i, k in enumerate(sizes):
        a = np.stack([r[per * pos:per * (pos + k)] for r in raws]) if len(raws) > 1 else raws[0][per * pos:per * (pos + k)]
        rx.push(a)
        if every or i == len(sizes) - 1:
            for key in parts:
                parts[key].append(rx.debug_dec(*key))
        got += rx.poll_ready()
        pos += k
    got += rx.poll()
    return {key: np.concatenate(p) for key, p in parts.items()}, got


# -------------------------------------------------------------------------------------------------------------------- the checks
def _fields(b, t0, d0):
    return (b.chn, b.nbrow, b.nlbyte, _f32(b.df), _f32(b.ppm), b.trig_dec - d0, b.end_dec - d0, b.trig_sample - t0, b.end_sample - t0,
            b.data)


def _check_records(ref, got, t0, sizes, stream=0):
    """records of one stream: channel, rows, df and ppm bits, the four stamps moved by exactly D0 / T0, all 2040 bytes; hand-out order"""
    d0, s = E.d0(t0, ref.clk), lambda m: E.dec_to_sample(m, ref.clk)      # noqa: E731
    key = lambda f: (f[6], f[0])      # noqa: E731
    mine = [b for b in got if b.stream == stream]
    want = sorted(((w.chn, w.nbrow, w.nlbyte, _f32(w.df), _f32(w.ppm), w.trig_dec, w.end_dec, s(w.trig_dec), s(w.end_dec), w.data)
                   for w in ref.blocks), key=key)
    fields = [_fields(b, t0, d0) for b in mine]
    assert sorted(fields, key=key) == want
    assert all(len(b.data) == 8 * 255 for b in mine)
    last = {}
    for f in fields:        # per channel in time order, always
        assert last.get(f[0], -1) < f[6]
        last[f[0]] = f[6]
    cuts = np.cumsum(sizes)[:-1]
    if all(abs(w[8] - c) > MARGIN for w in want for c in cuts):
        assert fields == want       # (end_sample, stream, chn): no burst ends where either of two pushes could complete it
    return mine


def _check_planes(ref, planes, what, stream=0, last=None):
    """the planes of every push put together are the yardstick's; last = J of the last push: only that push's were read"""
    for c, d in ref.dec.items():
        g = planes[(stream, c)]
        d = d if last is None else d[len(d) - last:]
        assert len(g) == len(d) and np.array_equal(_bits(g), _bits(d)), (what, stream, c)


def _poll_frames(rx, cap=4096):
    """(stream, chn, trig_dec, end_dec, hdata) of every frame, in hand-out order"""
    buf = (lib.FrameT * cap)()
    n = rx._check(rx.L.vdl2gpu_poll_frames(rx.h, buf, cap))
    assert n < cap
    return [(buf[i].stream, buf[i].chn, buf[i].trig_dec, buf[i].end_dec, bytes(buf[i].data[:buf[i].len])) for i in range(n)]


def _check_frames(O, ref, frames, t0, stream=0, some=True):
    """frames of one stream and their stamps, per channel in time order; some: the stream has CRC-clean frames (the crafted planes' payloads
    are random bytes: their frame list is the oracle's, empty or not)"""
    d0 = E.d0(t0, ref.clk)
    want = [(stream, b.chn, b.trig_dec, b.end_dec, f) for b in sorted(ref.blocks, key=lambda b: (b.end_dec, b.chn))
            for f in O.frames_of_block(b.nbrow, b.nlbyte, b.data)]
    mine = [(s, c, t - d0, e - d0, f) for s, c, t, e, f in frames if s == stream]
    assert sorted(mine) == sorted(want) and (len(want) >= 1 or not some)
    last = {}
    for s, c, t, e, f in mine:
        assert last.get(c, -1) <= e
        last[c] = e


def _check_levels_and_soft(ref, mine, t0, levels=True):
    """levels against tests/levels_ref.py and reliability maps against tests/soft_ref.py, both on the oracle's planes, with the
    records' stamps moved back by D0 (test_gpu_levels._check_exact indexes the plane by them)"""
    d0 = E.d0(t0, ref.clk)
    back = [dataclasses.replace(b, trig_dec=b.trig_dec - d0, end_dec=b.end_dec - d0) for b in mine]
    if levels:
        back = [dataclasses.replace(b, level=dataclasses.replace(b.level, sym_first_dec=b.level.sym_first_dec - d0)) for b in back]
        assert all(b.level.noise_blocks == LR.NEVAL // LR.BLOCK for b in back)      # (FIRST: no block is clipped by the stream's start)
        whole = types.SimpleNamespace(debug_dec=lambda stream, ch: ref.dec[ch])
        TL._check_exact(whole, back, types.SimpleNamespace(rate=ref.rate), ref.fmt)
    pn = SR.pn_bits()
    clk = {(c, t["dec_index"]): t["clk"] for c, tr in ref.trig.items() for t in tr if t["accepted"] == 1}
    for b in back:
        hard, rel = SR.soft_block(ref.dec[b.chn], b.nbrow, b.nlbyte, b.df, b.trig_dec, clk[(b.chn, b.trig_dec)], pn)
        assert hard.tobytes() == b.data and b.soft is not None and np.array_equal(b.soft, rel), (b.chn, b.trig_dec)


def _check_heads(ref, heads, t0, from_dec, stream=0):
    """every trigger of the oracle's chain in the last push (from frame from_dec on) has an entry with its instant moved by D0, its 25
    soft bits and the detector's four floats as bits"""
    d0, n = E.d0(t0, ref.clk), 0
    for c, trigs in ref.trig.items():
        mine = heads[heads["sc"] == stream * 8 + c]
        for t in trigs:
            if len(t["head"]) < 25 or t["dec_index"] < from_dec + 16:
                continue
            cand = mine[mine["nstar"] - d0 == t["dec_index"]]
            hit = [e for e in cand if np.array_equal(_bits(e["soft"]), _bits(t["head"])) and e["clk0"] == t["clk"]
                   and [_f32(e[k]) for k in ("p2err", "perr", "err", "pfr")] == [_f32(t[k]) for k in ("p2err", "perr", "err", "pfr")]]
            assert hit, (c, t["dec_index"], len(cand))
            n += 1
    assert n >= 1


def _check_stats(rx, ref, t0, nbursts=None):
    st = rx.stats()
    assert st["samples_in"] == t0 + ref.n and st["dec_samples"] == E.d0(t0, ref.clk) + 21 * ref.n // ref.clk
    assert st["bursts"] == (len(ref.blocks) if nbursts is None else nbursts) and st["overflowed"] == 0 and st["frames_dropped"] == 0
    return st


def _check_k1(rx, want):
    """which channeliser kernels ran: {kernel: True (some launches), False (none) or an exact count}"""
    k = rx.debug_k1()
    for name, v in want.items():
        assert (k[name] > 0) == v if isinstance(v, bool) else k[name] == v, (name, v, k)


# ============================================================================================ a. the demodulator's paths, 2 MS/s cs16
FEATURES = {"default": ("frames", "levels", "soft"), "fullscan": ("frames", "heads"), "serial": ("frames",),
            "noregion-r0": ("levels", "soft"), "noregion-r2": ("frames", "levels", "soft", "heads")}


def _demod_case(O, monkeypatch, ref, path, bnd, k1_fast_name):
    kw, rounds, k1 = PATHS[path]
    blk, t0 = _epoch(ref, bnd)
    _env(monkeypatch, t0, general=k1 == "general", rounds=rounds)
    sizes = _ragged(ref, blk)
    feat = FEATURES[path]
    kw = dict(kw, flags=kw.get("flags", 0) | (lib.F_DEBUG_HEADS if "heads" in feat else 0))
    identity = ref.fmt == "cf32"
    levels = "levels" in feat and not identity      # (the crafted planes have exact zeros between their bursts: no noise level in dB)
    with _rx(ref, max(sizes), frames="frames" in feat, levels=levels, soft_rs="soft" in feat, **kw) as rx:
        # (the planes of every push are read only in the identity rig: reading them waits for the push, and the pushes of the
        # 2 MS/s stream are to overlap as they do in service)
        planes, got = _pushed(rx, ref, sizes, every=identity)
        last_from = 21 * (ref.n - sizes[-1]) // ref.clk
        _check_planes(ref, planes, path, last=None if identity else 21 * ref.n // ref.clk - last_from)
        mine = _check_records(ref, got, t0, sizes)
        if "frames" in feat:
            _check_frames(O, ref, _poll_frames(rx), t0, some=not identity)
        if "soft" in feat:
            _check_levels_and_soft(ref, mine, t0, levels)
        if "heads" in feat:
            _check_heads(ref, rx.debug_heads(), t0, last_from)
        _check_stats(rx, ref, t0)
        if k1 == "general":
            _check_k1(rx, {"k1_fast": False, "k1_pp": False, "general_lds": True, "general_global": False})
        else:
            _check_k1(rx, {k1_fast_name: True, "general_global": False})


@pytest.mark.timeout(120)
@pytest.mark.parametrize("bnd", ("in31", "in32", "dec31", "dec32"))
@pytest.mark.parametrize("path", list(PATHS))
def test_demodulator_paths_across_a_boundary(built, oracle, monkeypatch, path, bnd):
    """k3's carry and rebase, a deferred burst, a serial push and the repair rounds' windows at a dec_base beside 2^31 / 2^32, on both
    axes: the K2Params a push is given, ChanState.pos, the (int)(n - dec_base) narrowings, dec_to_sample on the way out"""
    _demod_case(oracle, monkeypatch, _two(oracle), path, bnd, "k1_fast")


@pytest.mark.timeout(120)
@pytest.mark.parametrize("bnd", ("dec31", "big40"))
@pytest.mark.parametrize("path", ("default", "noregion-r2"))
@pytest.mark.parametrize("name", ("edge", "train"))
def test_crafted_planes_late(built, oracle, monkeypatch, name, path, bnd):
    """geometry edges and trains of close followers through the identity rig: debug_dec == the crafted plane, bit for bit, at every push"""
    _demod_case(oracle, monkeypatch, _crafted(name), path, bnd, "k1_pp")


# ================================================================================================================ b. k1_fast, late
@pytest.mark.timeout(120)
@pytest.mark.parametrize("general", (False, True), ids=("k1_fast", "general"))
@pytest.mark.parametrize("bnd", ("in31", "in32", "big40"))
@pytest.mark.parametrize("fmt", ("cu8", "cs16"))
def test_k1_fast_whole_superperiods(built, oracle, monkeypatch, fmt, bnd, general):
    """pushes of whole superperiods: k1_fast takes all of each (no general launch at either end); the same epoch through the general
    kernel alone"""
    ref = _two(oracle, fmt)
    _, t0 = _epoch(ref, bnd)
    _env(monkeypatch, t0, general=general)
    sizes = _whole(ref, 8000, (13, 5, 21, 13))
    with _rx(ref, max(sizes)) as rx:
        planes, got = _pushed(rx, ref, sizes)
        _check_planes(ref, planes, (fmt, bnd, general))
        _check_records(ref, got, t0, sizes)
        _check_stats(rx, ref, t0)
        _check_k1(rx, {"k1_fast": 0, "k1_pp": 0, "general_lds": len(sizes), "general_global": 0} if general else
                  {"k1_fast": len(sizes), "k1_pp": 0, "general_lds": 0, "general_global": 0})


@pytest.mark.timeout(120)
def test_rtl_quirk_late(built, oracle, monkeypatch):
    """VDL2GPU_F_RTL_QUIRK: T0 a multiple of 4 096 000 (whole superperiods and whole 32768-sample blocks); the quirk keeps a handle on
    the general kernel, whatever the push"""
    def make():
        spec = S.placed(2_000_000, TWO_FO, 41, [(0.035, 40), (0.300, 66), (0.575, 250), (0.600, 120), (0.670, 31)], q=32768)
        return _oracle_ref(oracle, synth.synth_stream(spec, "cu8"), "cu8", 2_000_000, TWO_FO, ofmt="cu8_quirk")
    ref = _cached("quirk", make)
    _, t0 = _epoch(ref, "in31", quirk=True)
    assert t0 % 4_096_000 == 0
    _env(monkeypatch, t0)
    sizes = _whole(ref, 32768, (10, 7, 15, 11))
    with _rx(ref, max(sizes), rtl_quirk=True) as rx:
        planes, got = _pushed(rx, ref, sizes)
        _check_planes(ref, planes, "quirk")
        _check_records(ref, got, t0, sizes)
        _check_stats(rx, ref, t0)
        _check_k1(rx, {"k1_fast": 0, "k1_pp": 0, "general_lds": len(sizes), "general_global": 0})


# ================================================================================== c. k1_fast across a wrap of its work counters
TICKET0 = (1 << 32) - 3
K1F_CHUNK = 8               # superperiods per ticket (vdl2gpu_k1.h)
WRAP_SP = (320, 192, 192)   # superperiods per push
WRAP_PLAN = [(0.035, 40), (0.600, 120), (1.200, 250), (1.900, 66), (2.700, 31)]


def _wrap_ref(O, seed=51, plan=WRAP_PLAN):
    def make():
        spec = S.placed(2_000_000, TWO_FO, seed, plan, q=8000, nsamples=sum(WRAP_SP) * 8000)
        return _oracle_ref(O, synth.synth_stream(spec, "cs16"), "cs16", 2_000_000, TWO_FO)
    return _cached(("wrap", seed), make)


def _wrap_sizes(ref, nfam):
    """Three pushes of whole superperiods, k1_fast taking all of each.  A family (role x XCD x) of a launch over n superperiods has
    (n - x + 7) >> 3 of them, in tickets of K1F_CHUNK, and makes one request to its counter per ticket: request k gets the answer
    tbase + k and is handed ticket nfam + (int)(answer - tbase).  With the counters begun at 2^32 - 3 the first launch must make more
    than three requests in every family -- the fourth gets the answer 0, numerically BELOW its base -- and must not end on 0 again, so
    that the later launches start from a small wrapped base on both sides.  With one workgroup per family (nfam = 1) every ticket but
    the first comes from an answer, and the one from the answer 0 must still have work."""
    sizes = [k * 8000 for k in WRAP_SP]
    assert sum(sizes) == ref.n
    tickets = [[-(-((k - x + 7) >> 3) // K1F_CHUNK) for x in range(8)] for k in WRAP_SP]
    assert all(t >= 3 for ts in tickets for t in ts)                                    # every push: three tickets or more in every family
    below = (1 << 32) - TICKET0                                                         # the request that gets the answer 0
    assert all(t > below and (TICKET0 + t) % (1 << 32) != 0 for t in tickets[0])
    if nfam == 1:
        assert all(nfam + below < t for t in tickets[0])
    return sizes


def _wrap_env(monkeypatch, t0, nfam):
    _env(monkeypatch, t0, ticket0=TICKET0)
    if nfam:
        monkeypatch.setenv("VDL2GPU_K1F_NFAM", str(nfam))
    else:
        monkeypatch.delenv("VDL2GPU_K1F_NFAM", raising=False)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("nfam", (0, 1), ids=("nfam-default", "nfam-1"))
@pytest.mark.parametrize("bnd", (None, "in32"), ids=("epoch0", "in32"))
def test_k1_fast_counters_wrap(built, oracle, monkeypatch, bnd, nfam):
    """nfam-default: as many workgroups per family as the handle chooses; nfam-1: one, which takes every ticket behind its first from
    the counter's answers (VDL2GPU_K1F_NFAM, a knob of the product)"""
    ref = _wrap_ref(oracle)
    t0 = 0 if bnd is None else _epoch(ref, bnd)[1]
    _wrap_env(monkeypatch, t0, nfam)
    sizes = _wrap_sizes(ref, nfam)
    with _rx(ref, max(sizes)) as rx:
        planes, got = _pushed(rx, ref, sizes)
        _check_planes(ref, planes, ("wrap", bnd, nfam))
        _check_records(ref, got, t0, sizes)
        _check_stats(rx, ref, t0)
        _check_k1(rx, {"k1_fast": 3, "k1_pp": 0, "general_lds": 0, "general_global": 0})


@pytest.mark.timeout(120)
def test_k1_fast_counters_wrap_two_streams(built, oracle, monkeypatch):
    """the host's idea of the counters is kept per stream: two streams with their own bursts, one workgroup per family"""
    refs = [_wrap_ref(oracle), _wrap_ref(oracle, 52, [(0.040, 66), (0.800, 250), (1.500, 40), (2.200, 120), (2.720, 17)])]
    assert refs[0].n == refs[1].n
    _wrap_env(monkeypatch, 0, 1)
    sizes = _wrap_sizes(refs[0], 1)
    with _rx(refs[0], max(sizes), fos=(TWO_FO, TWO_FO)) as rx:
        planes, got = _pushed(rx, refs[0], sizes, streams=[r.raw for r in refs])
        for s, ref in enumerate(refs):
            _check_planes(ref, planes, "wrap, two streams", stream=s)
            _check_records(ref, got, 0, sizes, stream=s)
        _check_stats(rx, refs[0], 0, nbursts=sum(len(r.blocks) for r in refs))
        _check_k1(rx, {"k1_fast": 3, "k1_pp": 0, "general_lds": 0, "general_global": 0})


# ==================================================================================== d. k1_pp and the general channeliser, late
def _eight(O, rate, fmt, fo):
    def make():
        spec = S.eight_channels(rate=rate, fo=fo, dur=0.12, t0=0.035)
        return _oracle_ref(O, synth.synth_stream(spec, fmt), fmt, rate, fo)
    return _cached(("eight", rate, fmt), make)


def _offgrid(O):
    """15.36 MS/s: the LO table (3072 entries) does not fit LDS beside the windows, the general kernel reads it from global memory at
    no0 = total_in % 3072; judged by tests/offgrid_model.py (the oracle's own table is no whole period off the 25 kHz grid)"""
    def make():
        rate, fmt = 15_360_000, "cs16"
        fos = G.fos_of(rate, fmt, 2)
        spec = S.placed(rate, fos, 61, [(0.035, 17), (0.046, 120), (0.056, 66), (0.095, 28)], q=4 * 3840)
        raw = synth.synth_stream(spec, fmt)
        return _model_ref(O, raw, fmt, rate, fos, [M.channelise(raw, fmt, rate, fo) for fo in fos])
    return _cached("offgrid", make)


D_CASES = [("10000k-cs16", "in31"), ("10000k-cs16", "in32"), ("5000k-f32", "in32"), ("15360k-cs16", "in32")]


@pytest.mark.timeout(180)
@pytest.mark.parametrize("row,bnd", D_CASES, ids=[f"{r}-{b}" for r, b in D_CASES])
def test_k1_pp_and_general_late(built, oracle, monkeypatch, row, bnd):
    """ragged pushes: the carried partial window (c0, nf0) and the table offset no0 come from a total_in beside 2^31 / 2^32"""
    if row == "10000k-cs16":
        ref = _eight(oracle, 10_000_000, "cs16", S.FO8_10MS)
    elif row == "5000k-f32":
        ref = _eight(oracle, 5_000_000, "f32", S.FO8_AIR_5MS)
    else:
        ref = _offgrid(oracle)
        assert not G._table_in_lds(ref.rate) and E.lo_len(ref.rate) == 3072
    _, t0 = _epoch(ref, bnd)
    _env(monkeypatch, t0)
    sizes = TR._ragged(4 * ref.clk, ref.n, np.random.default_rng(ref.rate // 1000))
    assert len(sizes) >= 4 and any(k % (4 * ref.clk) for k in sizes[:-1])
    with _rx(ref, max(sizes)) as rx:
        planes, got = _pushed(rx, ref, sizes)
        _check_planes(ref, planes, (row, bnd))
        _check_records(ref, got, t0, sizes)
        _check_stats(rx, ref, t0)
        lds = row != "15360k-cs16"
        _check_k1(rx, {"k1_pp": True, "k1_fast": 0, "general_lds": lds, "general_global": not lds})


# ================================================================================================================== e. exact Fo, late
# the rows of tests/exactfo_model.py that run k1_fast, k1_pp and the general kernel (here: alone) with a residual: rate, format,
# offsets, the kernel
E_ROWS = {"2000k": (2_000_000, "cs16", (-295_900, 12_500), "k1_fast"), "2048k": (2_048_000, "cu8", (-195_900, 312_500), "k1_pp"),
          "15360k": (15_360_000, "cs16", (4_100,), "general_global")}
E_SHORT = [(0.035, 17), (0.050, 120), (0.095, 28), (0.112, 40)]        # (no two overlap: one row has a single channel)
E_LONG = [(0.035, 40), (0.700, 28), (1.472, 120), (1.480, 66), (1.530, 40)]      # a burst over sample 2^32 mod 4 000 000 = 2 967 296
E_CASES = [("2000k", "in32", True), ("2000k", "in32", False), ("2000k", "big40", False), ("2048k", "in32", False), ("15360k", "in32", False)]


def _exact_input(row, long):
    def make():
        rate, fmt, fos, _ = E_ROWS[row]
        spec = S.placed(rate, fos, 71, E_LONG if long else E_SHORT, q=16 * (rate // 4000))
        raw = synth.synth_stream(spec, fmt)
        raw.setflags(write=False)
        return raw
    return _cached(("exact raw", row, long), make)


def _exact_ref(O, row, long, first):
    """the model's planes (tests/exactfo_model.py) for the stream whose first sample is sample `first`, and the oracle's demodulator
    over them"""
    def make():
        rate, fmt, fos, _ = E_ROWS[row]
        raw = _exact_input(row, long)
        return _model_ref(O, raw, fmt, rate, fos, [X.channelise(raw, fmt, rate, fo, first=first) for fo in fos])
    return _cached(("exact", row, long, first), make)


@pytest.mark.timeout(180)
@pytest.mark.parametrize("row,bnd,pure", E_CASES, ids=[f"{r}-{b}-{'shift' if p else 'abs'}" for r, b, p in E_CASES])
def test_exact_fo_late(built, oracle, monkeypatch, row, bnd, pure):
    """the residual oscillator's per-push base (K1Rot.sq0, i0 from done / 21 * SDRCLK) at a qin beside 2^32 and 2^40.  pure: T0 a multiple
    of 2 SDRINRATE, where the oscillator begins anew -- the expectation is the model from sample 0, moved; otherwise the model with
    absolute sample indices, which is NOT the model from sample 0 (asserted)"""
    rate, fmt, fos, kernel = E_ROWS[row]
    zero = _exact_ref(oracle, row, pure, 0)
    _, t0 = _epoch(zero, bnd, pure_shift=pure)
    assert (t0 % (2 * rate) == 0) == pure
    ref = zero if pure else _exact_ref(oracle, row, False, t0)
    fd = X.split(fos[0])[1]
    assert fd != 0 and np.array_equal(X.indices(64 * zero.clk, rate, fd, first=t0), X.indices(64 * zero.clk, rate, fd)) == pure
    if not pure:
        assert not np.array_equal(_bits(ref.dec[0]), _bits(zero.dec[0]))
        assert sorted(ref.blocks, key=lambda b: b.trig_dec)[0].trig_dec - RAMP >= FIRST
        _assert_crossing(ref, bnd, t0)      # ... and the model's records at that epoch cross the boundary as well
    _env(monkeypatch, t0, general=kernel == "general_global")
    per = 16 * ref.clk
    cuts = [7 * per + 123, 7 * per + 124, 16 * per + 124, 21 * per]
    if bnd != "big40":      # a push begins behind the boundary: its base is worked out from a total_in past 2^32
        cuts.append((1 << 32) - t0 + 2 * per + 7)
    cuts = sorted(set(cuts))
    assert 0 < cuts[0] and cuts[-1] < ref.n
    sizes = np.diff([0] + cuts + [ref.n]).tolist()
    with _rx(ref, max(sizes), exact_fo=True) as rx:
        planes, got = _pushed(rx, ref, sizes)
        _check_planes(ref, planes, (row, bnd, pure))
        _check_records(ref, got, t0, sizes)
        _check_stats(rx, ref, t0)
        if kernel == "general_global":
            _check_k1(rx, {"k1_fast": 0, "k1_pp": 0, "general_lds": 0, "general_global": True})
        else:
            _check_k1(rx, {kernel: True, "general_global": 0})


# ========================================================================================== f. the ingest ring and two streams
@pytest.mark.timeout(120)
def test_ingest_ring_two_streams_late(built, oracle, monkeypatch):
    """the 2 MS/s stream of the demodulator paths and another with its own bursts, written in place into the page-locked ring, with
    frames, levels and reliability maps, across 2^32 input samples"""
    refs = [_two(oracle), _two(oracle, seed=32, plan=[(0.036, 66), (0.060, 250), (0.135, 17), (0.150, 120), (0.192, 17)])]
    n = refs[0].n
    assert refs[1].n == n
    blk, t0 = _epoch(refs[0], "in32")
    before, _, after = E.crossing(E.BOUNDARIES["in32"], t0, 500, refs[1].blocks)
    assert before and after
    _env(monkeypatch, t0)
    slot = 50_001
    sizes = [min(slot, n - s) for s in range(0, n, slot)]
    with _rx(refs[0], slot, fos=(TWO_FO, TWO_FO), frames=True, levels=True, soft_rs=True) as rx:
        rx.ring_init(slot, nslots=3)
        got, pos = [], 0
        for k in sizes:
            buf = rx.ring_acquire()
            for s, r in enumerate(refs):
                buf[s, :4 * k] = r.raw[2 * pos:2 * (pos + k)].view(np.uint8)
            rx.ring_commit(k)
            got += rx.poll_ready()
            pos += k
        got += rx.poll()
        frames = _poll_frames(rx)
        for s, ref in enumerate(refs):
            mine = _check_records(ref, got, t0, sizes, stream=s)
            _check_frames(oracle, ref, frames, t0, stream=s)
            _check_levels_and_soft(ref, mine, t0)
        _check_stats(rx, refs[0], t0, nbursts=sum(len(r.blocks) for r in refs))
        _check_k1(rx, {"k1_fast": True, "k1_pp": 0, "general_global": 0})
