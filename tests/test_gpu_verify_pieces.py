"""The verify pass hands its workgroups PIECES of the stretches the chain idled through (k2a_verify: pieces aligned at a stretch's own
start, shared out in equal chunks over whatever grid the launch has).  Region scan dropped (test build, F_TEST_NOREGION), so every
burst is an event only the verify pass can find: a piece that is skipped, cut short or scanned in the wrong class loses a burst.
2 MS/s cs16, 1 << 21 samples, three channels; the oracle's bursts are computed once per stream."""
import ctypes as C
import functools

import numpy as np
import pytest

import scenarios as S
from vdlm2dec_amd import lib, synth

pytestmark = pytest.mark.gpu

N = 1 << 21
TILE = 2048         # samples of a full piece: K2A_TS evaluation instants of one parity
SLOT = lib.DBG["VERIFY_INSTANTS"]   # debug counter: evaluation instants of every piece the verify passes scanned


def _keys(bursts):
    return sorted((b.chn, b.nbrow, b.nlbyte, bytes(b.data)) for b in bursts)


GAP = 0.131         # seconds between two burst starts of a channel in the sparse stream: more than the longest push its cases use (250 001 samples)


@functools.lru_cache(maxsize=None)
def _scenario(sparse=False):
    """Two streams from one random_scenario.  The rich one as it comes (14 bursts a second and channel).  The sparse one keeps a
    burst only if it starts more than GAP after the last one kept on its channel: with the region scan dropped a burst leaves the chain in
    a class nothing is listed in, so the SECOND burst that starts in a channel-push is an event the repair round's own verify pass
    finds -- one local repair round cannot carry such a push (two rounds, or the serial redo, do), whatever the verify pass's
    decomposition.  With at most one burst start per channel-push it must."""
    spec = synth.random_scenario(2_000_000, S.FO8[:3], N, seed=1010, bursts_per_s=14.0, info_max=120)
    if sparse:
        kept, last = [], {}
        for b in sorted(spec.bursts, key=lambda b: b.t0):
            if b.t0 - last.get(b.chan, -1.0) > GAP:
                kept.append(b)
                last[b.chan] = b.t0
        spec.bursts = kept
    raw = synth.synth_stream(spec, "cs16")
    raw.setflags(write=False)
    return spec, raw


@pytest.fixture(scope="module")
def want(oracle):
    """the oracle's bursts of the rich and of the sparse stream, computed once"""
    out = {}
    for sparse in (False, True):
        spec, raw = _scenario(sparse)
        out[sparse] = sorted(b.key() for b in oracle.run_oracle(raw, "cs16", spec.rate, spec.fo, S.FC))
    assert len(out[False]) >= 25 and len(out[True]) >= 12
    return out


def _run(block, sparse=False):
    from vdlm2dec_amd import lib as _lib
    from vdlm2dec_amd.demod import Receiver, plan_channels
    spec, raw = _scenario(sparse)
    with Receiver(spec.rate, plan_channels(S.FC, spec.fo), fmt="cs16", max_push=block, flags=_lib.F_TEST_NOREGION, testhooks=True) as rx:
        got = rx.run(raw, block=block)
        st = rx.stats()
    return got, st


def _check(block, want, rounds=1):
    """both streams in pushes of `block` samples: the oracle's bursts; on the sparse one, where a repair round is scheduled, every
    channel-push with a burst goes through it and none is left to the serial redo"""
    assert block / 2_000_000 < GAP
    got, st = _run(block)
    assert _keys(got) == want[False]
    got, st = _run(block, sparse=True)
    assert _keys(got) == want[True]
    if rounds >= 1:
        assert st["serial_redos"] == 0, (st["serial_redos"], st["repairs"])
        assert st["repairs"] >= len(want[True]) // 2, st["repairs"]      # (a burst in seven of the eight classes is an event)


def _segs(rx, ch):
    buf = np.zeros((4096, 4), np.int32)
    n = rx.L.vdl2gpu_debug_segs(rx.h, 0, ch, buf.ctypes.data_as(C.c_void_p), 4096)
    assert n >= 0
    return buf[:n]


def _instants(segs):
    return sum((int(hi) - int(lo) + 1) // 2 for lo, hi, _, _ in segs if hi > lo)


@pytest.mark.parametrize("block", [65536, 65537, 250001, 4099] + [TILE * 31 + d for d in (-2, -1, 0, 1, 2)])
def test_piece_edges_push_lengths(built, want, block):
    """Pushes of 65 536 and 65 537 samples (the second: an odd time base on every other push), 250 001, a push shorter than one tile,
    and pushes a sample or two either side of a whole number of tiles: where stretches begin and end moves against the pieces'
    length, every burst is found all the same and the local repair carries every channel (no serial redo)."""
    _check(block, want)


@pytest.mark.parametrize("hooks", [{"VDL2GPU_TEST_ITEM_GRID": "1"}, {"VDL2GPU_TEST_ITEM_GRID": "3"}, {"VDL2GPU_VERIFY2_WG": "1"},
                                   {"VDL2GPU_VERIFY2_WG": "64"}, {"VDL2GPU_REPAIR_ROUNDS": "0"}, {"VDL2GPU_REPAIR_ROUNDS": "1"},
                                   {"VDL2GPU_REPAIR_ROUNDS": "2"}], ids=lambda h: "-".join(f"{k[8:].lower()}{v}" for k, v in h.items()))
def test_any_grid_covers_the_part(built, want, monkeypatch, hooks):
    """One and three workgroups per channel (test build: one workgroup walks every chunk, in batches), the repair round's pass with 1
    and 64 workgroups, and 0, 1, 2 repair rounds: the oracle's bursts whatever the grid."""
    for k, v in hooks.items():
        monkeypatch.setenv(k, v)
    _check(250_001, want, rounds=int(hooks.get("VDL2GPU_REPAIR_ROUNDS", "1")))


@pytest.mark.parametrize("noregion", [True, False], ids=["noregion", "regions"])
@pytest.mark.parametrize("grid", [None, "1", "3"])
def test_every_instant_of_every_stretch_is_scanned_once(built, want, monkeypatch, grid, noregion):
    """With the debug counters on, one push and no repair round (the stretches vdl2gpu_debug_segs returns are then the ones the
    push's only verify pass was given): the evaluation instants of the pieces scanned are sum_k ceil((hi_k - lo_k) / 2), no more
    and no fewer.  Region scan dropped: one stretch per channel, the whole push (172 pieces); with it: a stretch per burst."""
    from vdlm2dec_amd import lib as _lib
    from vdlm2dec_amd.demod import Receiver, plan_channels
    monkeypatch.setenv("VDL2GPU_DEBUG_COUNTERS", "1")
    monkeypatch.setenv("VDL2GPU_REPAIR_ROUNDS", "0")
    if grid:
        monkeypatch.setenv("VDL2GPU_TEST_ITEM_GRID", grid)
    spec, raw = _scenario()
    with Receiver(spec.rate, plan_channels(S.FC, spec.fo), fmt="cs16", max_push=N, flags=_lib.F_TEST_NOREGION if noregion else 0, testhooks=True) as rx:
        rx.push(raw)
        got = rx.poll()
        rx.sync()
        scanned = rx.debug_counters(n=32, reset=False)[SLOT]
        segs = [_segs(rx, ch) for ch in range(len(spec.fo))]
    assert _keys(got) == want[False]
    total = sum(_instants(g) for g in segs)
    print("stretches", [len(g) for g in segs], "instants", total, "scanned", scanned)
    assert sum(len(g) for g in segs) >= (3 if noregion else 20) and total > 64 * 1024
    assert scanned == total, (scanned, total, [len(g) for g in segs])


@functools.lru_cache(maxsize=None)
def _dense():
    """one channel of short bursts back to back, 4.2 s in ONE push: more than 256 stretches in a channel-push"""
    spec = synth.random_scenario(2_000_000, S.FO8[:1], 4 << 21, seed=2020, bursts_per_s=2000.0, info_max=3, amp_range=(20.0, 60.0))
    raw = synth.synth_stream(spec, "cs16")
    raw.setflags(write=False)
    return spec, raw


@pytest.mark.parametrize("rounds,grid", [(0, None), (0, "1"), (1, None)])
def test_more_stretches_than_a_block_scan_takes_at_once(built, oracle, monkeypatch, rounds, grid):
    """More than K2A_THREADS = 256 stretches in one channel-push: the prefix of the pieces runs in chunks with a carried base.
    This case keeps the region scan: without it the chain finds no burst on its own and idles through the push in ONE stretch
    (and a local repair takes 256 new events at most).  Without a repair round the list the verify pass was given is still there
    to be counted, and its instants to be compared with what was scanned.  With ONE workgroup (test build) its share is every
    piece: more than K2A_VITEMS = 64, worked off in batches, each with the chunked prefix afresh."""
    from vdlm2dec_amd.demod import Receiver, plan_channels
    monkeypatch.setenv("VDL2GPU_DEBUG_COUNTERS", "1")
    monkeypatch.setenv("VDL2GPU_REPAIR_ROUNDS", str(rounds))
    if grid:
        monkeypatch.setenv("VDL2GPU_TEST_ITEM_GRID", grid)
    spec, raw = _dense()
    w = sorted(b.key() for b in oracle.run_oracle(raw, "cs16", spec.rate, spec.fo, S.FC))
    assert len(w) > 256
    with Receiver(spec.rate, plan_channels(S.FC, spec.fo), fmt="cs16", max_push=4 << 21, testhooks=True) as rx:
        rx.push(raw)
        got = rx.poll()
        rx.sync()
        st = rx.stats()
        scanned = rx.debug_counters(n=32, reset=False)[SLOT]
        segs = _segs(rx, 0)
    assert _keys(got) == w
    print("stretches", len(segs), "instants", _instants(segs), "scanned", scanned, "serial_redos", st["serial_redos"], "repairs", st["repairs"])
    if rounds == 0:
        assert len(segs) > 256, len(segs)
        assert scanned == _instants(segs), (scanned, len(segs))
    else:
        assert st["serial_redos"] == 0, st
