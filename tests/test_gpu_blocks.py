"""Block path on the GPU: vdl2gpu_decode_blocks == the reference's blk_thread
(vdlm2.c:84-161, rs.c, crc.c) as restated by the oracle, frame for frame, byte for byte."""
import json
import glob
import os

import numpy as np
import pytest

import scenarios as S
from vdlm2dec_amd import synth

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _rx():
    from vdlm2dec_amd.demod import Receiver, plan_channels
    return Receiver(2_000_000, plan_channels(S.FC, [-50000]), fmt="cu8", max_push=4096)


def _want(oracle, blocks):
    out = []
    for i, (nbrow, nlbyte, data) in enumerate(blocks):
        out += [(i, f) for f in oracle.frames_of_block(nbrow, nlbyte, data)]
    return out


def test_golden_blocks_give_the_reference_frames(built, oracle):
    """msgblk_t records of the real reference (tests/golden) -> the frames its own out() received."""
    blocks, frames = [], []
    for path in sorted(glob.glob(os.path.join(HERE, "golden", "*.json"))):
        meta = json.load(open(path))
        for c in meta["channels"]:
            for b in c["blocks"]:
                blocks.append((b["nbrow"], b["nlbyte"], bytes.fromhex(b["data"])))
            frames += c["frames"]
    with _rx() as rx:
        got = rx.decode_blocks(blocks)
    assert [f.hex() for _, f in got] == frames and len(frames) >= 20
    assert got == _want(oracle, blocks)


def _tx_block(rng, info_len, nerr_rows=()):
    """One transmitted burst as the demodulator would hand it over, optionally with byte errors."""
    info = bytes(rng.integers(0, 256, info_len, dtype=np.uint8).tolist())
    nbrow, nlbyte, data = synth.received_rows(synth.hdlc_payload(synth.avlc_frame(info)))
    data = bytearray(data)
    for r, nerr in nerr_rows:
        if r < nbrow:
            span = 249 if r < nbrow - 1 else max(nerr, nlbyte)
            for pos in rng.choice(span, size=nerr, replace=False):
                data[r * 255 + int(pos)] ^= int(rng.integers(1, 256))
    return nbrow, nlbyte, bytes(data)


def test_corrected_uncorrectable_and_random_rows(built, oracle):
    """Frames of bursts whose rows are clean, carry 1..3 byte errors in their data bytes (corrected: the frame arrives), 4 and more
    (no frame on either side, whatever rs() left in the row), over burst lengths in the three FEC-shortening regimes, and of
    records of pure noise and of one repeated byte (no frame either).  What this observes is frames: a row rs() cannot repair, or
    miscorrects, is compared row by row in test_gpu_rs.py, not here."""
    rng = np.random.default_rng(77)
    blocks = []
    for n in (1, 2, 3, 10, 28, 31, 60, 66, 70, 120, 247, 250, 400, 497, 900, 1500, 1900):
        blocks.append(_tx_block(rng, n))
        for nerr in (1, 2, 3, 4, 5, 7):
            blocks.append(_tx_block(rng, n, [(0, nerr)]))
            blocks.append(_tx_block(rng, n, [(r, nerr) for r in range(8)]))
    for _ in range(200):
        nbrow = int(rng.integers(1, 9))
        blocks.append((nbrow, int(rng.integers(0, 250)), bytes(rng.integers(0, 256, 8 * 255, dtype=np.uint8).tolist())))
    for fill in (0x00, 0xff, 0x7e, 0x3f, 0xfc):       # degenerate streams: all stuffing / all flags
        blocks.append((8, 249, bytes([fill]) * (8 * 255)))
    want = _want(oracle, blocks)
    with _rx() as rx:
        got = rx.decode_blocks(blocks)
    assert got == want
    assert len(want) >= 80


def test_decoded_stream_to_frames_end_to_end(built, oracle):
    """IQ -> bursts (demodulator kernels) -> frames (block kernel), all on the GPU, against
    IQ -> oracle demodulator -> oracle block path."""
    from vdlm2dec_amd.demod import Receiver, plan_channels
    spec = S.eight_channels(seed=340)
    raw = synth.synth_stream(spec, "cs16")
    ob = sorted(oracle.run_oracle(raw, "cs16", spec.rate, spec.fo, S.FC), key=lambda b: (b.chn, b.end_dec))
    want = [(b.chn, f) for b in ob for f in oracle.frames_of_block(b.nbrow, b.nlbyte, b.data)]
    with Receiver(spec.rate, plan_channels(S.FC, spec.fo), fmt="cs16", max_push=1 << 21) as rx:
        bursts = sorted(rx.run(raw), key=lambda b: (b.chn, b.end_dec))
        got = [(bursts[i].chn, f) for i, f in rx.decode_blocks(bursts)]
    assert got == want and len(want) >= 8


def test_block_path_in_the_pipeline(built, oracle):
    """frames=True: the block kernel runs on every push's records in device memory; frames arrive
    through vdl2gpu_poll_frames, the bursts are still there for vdl2gpu_poll."""
    from vdlm2dec_amd.demod import Receiver, plan_channels
    spec = S.eight_channels(seed=341)
    raw = synth.synth_stream(spec, "cs16")
    ob = sorted(oracle.run_oracle(raw, "cs16", spec.rate, spec.fo, S.FC), key=lambda b: (b.end_dec, b.chn))
    want = [(0, b.chn, f) for b in ob for f in oracle.frames_of_block(b.nbrow, b.nlbyte, b.data)]
    with Receiver(spec.rate, plan_channels(S.FC, spec.fo), fmt="cs16", max_push=1 << 19, frames=True) as rx:
        bursts, frames = [], []
        per = 4
        for s0 in range(0, spec.nsamples, 1 << 19):
            rx.push(raw[2 * s0:2 * (s0 + (1 << 19))])
            frames += rx.poll_frames()
            bursts += rx.poll()
    assert sorted(frames) == sorted(want) and len(want) >= 8
    assert sorted((b.chn, b.nbrow, b.nlbyte, b.data) for b in bursts) == sorted(b.key() for b in ob)


def _compact_scenario():
    """One channel whose bursts reach every way a frame leaves the block kernel in the pipeline: a first frame of 199 and of 200
    bytes (with its 56-byte head, exactly the record's 256-byte slot) and of 201 (the arena), frames of about 1000 and 1900 bytes,
    two bursts of three nested frames (the second and third of a burst always go to the arena), ordinary short bursts between."""
    import blocks_craft as K
    rng = np.random.default_rng(2024)

    def body(n):
        return bytes(v if v != 0x7e else 0x7d for v in rng.integers(0, 256, n).tolist())

    payloads = [K.frame(body(195)), None, K.frame(body(196)), K.nested(3, rng, first=20, more=30), K.frame(body(197)), None,
                K.frame(body(1000)), None, K.nested(3, rng, first=150, more=120), K.frame(body(1900)), None]
    bursts, t = [], 0.002
    for i, p in enumerate(payloads):
        b = synth.Burst(chan=0, t0=t, info=body(int(rng.integers(5, 60))), amp=40.0, cfo=float(rng.uniform(-200, 200)), raw_payload=p)
        bursts.append(b)
        t += b.duration() + 0.002
    ns = (int((t + 0.004) * 2_000_000) + 32767) // 32768 * 32768
    return synth.StreamSpec(rate=2_000_000, fo=[-50000], nsamples=ns, bursts=bursts, seed=12)


def test_compact_slots_and_arena_in_the_pipeline(built, oracle):
    from vdlm2dec_amd.demod import Receiver, plan_channels
    spec = _compact_scenario()
    assert spec.nsamples < 4_000_000
    raw = synth.synth_stream(spec, "cs16")
    ob = oracle.run_oracle(raw, "cs16", spec.rate, spec.fo, S.FC)
    per = [oracle.frames_of_block(b.nbrow, b.nlbyte, b.data, cap=1 << 16) for b in ob]
    want = sorted((0, b.chn, f) for b, fs in zip(ob, per) for f in fs)
    assert sorted(len(fs) for fs in per) == [1] * 9 + [3, 3]
    lens = [len(fs[0]) for fs in per]
    assert {199, 200, 201} <= set(lens) and any(990 < n < 1100 for n in lens) and max(lens) > 1850
    step = -(-spec.nsamples // 3)
    with Receiver(spec.rate, plan_channels(S.FC, spec.fo), fmt="cs16", max_push=step, frames=True) as rx:
        bursts, frames = [], []
        for s0 in range(0, spec.nsamples, step):
            rx.push(raw[2 * s0:2 * (s0 + step)])
            frames += rx.poll_frames()
            bursts += rx.poll()
    assert sorted(frames) == want and len(want) == 15
    assert sorted((b.chn, b.nbrow, b.nlbyte, b.data) for b in bursts) == sorted(b.key() for b in ob)


def test_frames_of_channels_redone_serially(built, oracle):
    """The payload gather runs ahead of the verify pass; when that pass fails a channel, the serial redo
    makes the channel's records again and the ones made ahead are void.  The block kernel must skip
    them on the device (the records themselves are filtered on the host): every frame exactly once."""
    from vdlm2dec_amd import lib
    from vdlm2dec_amd.demod import Receiver, plan_channels
    spec = synth.random_scenario(2_000_000, S.FO8[:3], 1 << 21, seed=92, bursts_per_s=10.0, info_max=100)
    raw = synth.synth_stream(spec, "cs16")
    ob = oracle.run_oracle(raw, "cs16", spec.rate, spec.fo, S.FC)
    want = sorted((0, b.chn, f) for b in ob for f in oracle.frames_of_block(b.nbrow, b.nlbyte, b.data))
    with Receiver(spec.rate, plan_channels(S.FC, spec.fo), fmt="cs16", max_push=1 << 20, frames=True,
                  flags=lib.F_TEST_NOREGION) as rx:
        bursts, frames = [], []
        for s0 in range(0, spec.nsamples, 600_000):
            rx.push(raw[2 * s0:2 * (s0 + 600_000)])
            frames += rx.poll_frames()
            bursts += rx.poll()
        st = rx.stats()
    assert st["serial_redos"] > 0
    assert sorted(frames) == want and len(want) >= 10
    assert sorted((b.chn, b.nbrow, b.nlbyte, b.data) for b in bursts) == sorted(b.key() for b in ob)


def test_frames_of_channels_repaired_behind_the_payload_decode(built, oracle, monkeypatch):
    """The same handicap with repair rounds scheduled from the first push: the payload decode has run ahead on the first
    pass's selection when a round re-resolves a channel; those records (and the frames K4 would make of them) are void,
    the repaired selection is decoded behind the rounds -- bursts and frames must be the oracle's, none twice."""
    from vdlm2dec_amd import lib
    from vdlm2dec_amd.demod import Receiver, plan_channels
    monkeypatch.setenv("VDL2GPU_REPAIR_ROUNDS", "3")
    monkeypatch.setenv("VDL2GPU_DEBUG_COUNTERS", "1")
    spec = synth.random_scenario(2_000_000, S.FO8[:3], 1 << 21, seed=96, bursts_per_s=10.0, info_max=100)
    raw = synth.synth_stream(spec, "cs16")
    ob = oracle.run_oracle(raw, "cs16", spec.rate, spec.fo, S.FC)
    want = sorted((0, b.chn, f) for b in ob for f in oracle.frames_of_block(b.nbrow, b.nlbyte, b.data))
    with Receiver(spec.rate, plan_channels(S.FC, spec.fo), fmt="cs16", max_push=1 << 20, frames=True,
                  flags=lib.F_TEST_NOREGION) as rx:
        bursts, frames = [], []
        for s0 in range(0, spec.nsamples, 600_000):
            rx.push(raw[2 * s0:2 * (s0 + 600_000)])
            frames += rx.poll_frames()
            bursts += rx.poll()
        repaired = rx.debug_counters(32, reset=False)[lib.DBG["REPAIRED"]]      # channel-pushes that went through a repair round
    assert repaired > 0
    assert sorted(frames) == want and len(want) >= 10
    assert sorted((b.chn, b.nbrow, b.nlbyte, b.data) for b in bursts) == sorted(b.key() for b in ob)
