"""VDL2GPU_F_RAW_FLAGS on the GPU: crafted burst records through vdl2gpu_decode_blocks_ex with VDL2GPU_BLK_ALL_FRAMES | VDL2GPU_BLK_RAW_FLAGS
against the CPU model (tests/rawflags_ref.py) and against what the transmitter put into the burst (tests/rawflags_cases.py), the report's
counts, the modes that were there before, the row rules in front of it, and the pipeline and the drop-in with the flag and without it."""
import ctypes as C

import numpy as np
import pytest

import allframes_cases as Cs
import allframes_ref as A
import blockrep_ref as BR
import blocks_craft as K
import rawflags_cases as RC
import rawflags_ref as R
import scenarios as S
from test_gpu_allframes import RATE, _by_block, _ex, _poll_frames, _poll_records, rx  # noqa: F401  (rx: the fixture, any handle serves)

pytestmark = pytest.mark.gpu

RAW = 5         # VDL2GPU_BLK_ALL_FRAMES | VDL2GPU_BLK_RAW_FLAGS
ALL = 1
FRONT = ("row_roots", "row_how", "row_changed", "bytes_changed", "rows_failed", "rows_rescued", "stuffed", "nbytes", "flag_at", "status")


def _counts(r):
    return dict(cand=r.cand, too_short=r.too_short, bad_fcs=r.bad_fcs, frames=r.frames)


@pytest.fixture(scope="module")
def crafted(rx):  # noqa: F811
    """every crafted case in one call: (names, blocks, sent, frames per block, dropped, reports)"""
    from vdlm2dec_amd import lib
    assert lib.BLK_ALL_FRAMES | lib.BLK_RAW_FLAGS == RAW
    cs = RC.cases()
    blocks = [c[1] for c in cs]
    frames, dropped, reps = _ex(rx, blocks, RAW)
    return [c[0] for c in cs], blocks, [c[2] for c in cs], _by_block(frames, len(blocks)), dropped, reps


def test_crafted_bursts_against_model_and_transmitter(crafted):
    """a data byte 0x7e in the middle of a frame, as its first byte (behind the first flag: m1; behind a later flag), as its last body
    byte, as either FCS byte, runs of them, heavy stuffing around them, the dropped zero on the raw stream's boundaries, the byte on the
    mark words' and the scan's boundaries, per = 1, eight rows, 150 frames, a bad FCS: frames, dropped and counts are the model's, the
    frames the transmitter's, and everything in front of cand is the block path's without the mode"""
    names, blocks, sent, got, dropped, reps = crafted
    assert {"mid", "first-of-first", "first-of-later", "last-of-body", "fcs-low", "fcs-high", "run6", "ff7e", "bf7e", "info7e", "nested",
            "drop-bit7", "drop-bit0", "drop-row-last", "drop-row-first", "drop-span-last", "drop-span-first", "mark31", "mark32",
            "span-first", "span-last", "tiny", "full8", "many13", "badfcs"} <= set(names)
    for name, blk, s, g, r in zip(names, blocks, sent, got, reps):
        model, cnt = R.model(*blk)
        assert model == s, name
        assert g == s[:R.NCAND], name
        assert _counts(r) == cnt and r.cand == r.too_short + r.bad_fcs + r.frames, name
        ref = BR.model(*blk)
        for f in FRONT:
            assert getattr(r, f) == getattr(ref, f), (name, f)
    assert dropped == sum(max(0, len(s) - R.NCAND) for s in sent) == 138
    by = dict(zip(names, zip(got, reps)))
    assert by["many13"][1].frames == 150 and len(by["many13"][0]) == 12
    assert by["badfcs"][1].bad_fcs == 1 and len(by["badfcs"][0]) == 2          # counted once, and seq skips it (_by_block)


def test_all_frames_cases_are_unchanged_by_the_mode(rx):  # noqa: F811
    """no data byte 0x7e between the flags: the same frames, dropped and reports with and without the mode"""
    blocks = [c[1] for c in Cs.cases()]
    assert _ex(rx, blocks, RAW) == _ex(rx, blocks, ALL)


def test_noise_streams_equal_the_model(rx):  # noqa: F811
    """blocks_craft's records (every eighth) and bursts of idle flags: streams no transmitter makes, nested candidates with data bytes 0x7e"""
    e = [(n, b) for n, b, _ in K.everything()][::8] + BR.many_flags()
    blocks = [b for _, b in e]
    frames, dropped, reps = _ex(rx, blocks, RAW, cap=8192)
    got = _by_block(frames, len(blocks))
    differ = 0
    for (name, blk), g, r in zip(e, got, reps):
        model, cnt = R.model(*blk)
        assert g == model[:R.NCAND], name
        assert _counts(r) == cnt, name
        ref = BR.model(*blk)
        for f in FRONT:
            assert getattr(r, f) == getattr(ref, f), (name, f)
        differ += (model, cnt) != A.model(*blk)
    assert dropped == sum(max(0, len(R.model(*blk)[0]) - R.NCAND) for _, blk in e) and differ > 3


def test_info_7e_and_nested(rx):  # noqa: F811
    """info bytes of 0x7e: the all-frames mode gives the frames without one, as it did; this mode all four.  X | fcs(X) | 7e | Y: the
    all-frames mode gives X, which was never sent; this mode the whole frame and nothing else"""
    name, blk, sent, whole = Cs.info_7e()
    nblk, nwhole, ninner = RC.nested()
    f1, d1, r1 = _ex(rx, [blk, nblk], ALL)
    f5, d5, r5 = _ex(rx, [blk, nblk], RAW)
    assert _by_block(f1, 2) == [whole, [ninner]] and _by_block(f5, 2) == [sent, [nwhole]] and d1 == d5 == 0
    assert [_counts(r) for r in r1] == [A.model(*blk)[1], A.model(*nblk)[1]]
    assert [_counts(r) for r in r5] == [R.model(*blk)[1], R.model(*nblk)[1]]


def test_rescued_row_through_all_four_kernels(rx):  # noqa: F811
    """the row that carries the second frame (a data byte 0x7e in it) has four byte errors: with soft=, with fb=, with both, each with and
    without a report -- k4_frames_raw, _raw_rep, _raw_fb, _raw_rep_fb -- the second frame arrives; without the row rules only the first"""
    bad, rel, fb, sent = RC.rescue()
    for report in (True, False):
        plain, _, _ = _ex(rx, [bad], RAW, report=report)
        assert [f[3] for f in plain] == sent[:1]
    seen = []
    for kw in (dict(rels=[rel]), dict(fbs=[fb]), dict(rels=[rel], fbs=[fb])):
        for report in (True, False):
            frames, dropped, reps = _ex(rx, [bad], RAW, report=report, **kw)
            assert [f[3] for f in frames] == sent and [f[1] for f in frames] == [0, 1] and dropped == 0
            seen.append(frames)
            if report:
                model, cnt = R.model(*bad, rel=rel if "rels" in kw else None, fb=fb if "fbs" in kw else None)
                assert model == sent and _counts(reps[0]) == cnt == dict(cand=2, too_short=0, bad_fcs=0, frames=2)
                assert reps[0].rows_rescued == 1 and reps[0].row_changed[1] == 4
    assert all(s == seen[0] for s in seen)


def test_modes_0_and_1_give_what_they_gave(rx):  # noqa: F811
    """the crafted cases of this mode through the modes that were there: mode 0 is vdl2gpu_decode_blocks_feedback, mode 1 the all-frames
    model; VDL2GPU_BLK_RAW_FLAGS alone is refused"""
    from vdlm2dec_amd import lib
    blocks = [c[1] for c in RC.cases()]
    assert _ex(rx, blocks, 0) == _ex(rx, blocks, 0, call="feedback")
    frames, dropped, reps = _ex(rx, blocks, ALL)
    got = _by_block(frames, len(blocks))
    for blk, g, r in zip(blocks, got, reps):
        model, cnt = A.model(*blk)
        assert g == model[:A.NCAND] and _counts(r) == cnt
    assert dropped == sum(max(0, len(A.model(*blk)[0]) - A.NCAND) for blk in blocks)
    arr, out = (lib.BurstT * 1)(), (lib.FrameT * 1)()
    assert rx.L.vdl2gpu_decode_blocks_ex(rx.h, arr, None, None, 1, out, 1, None, None, lib.BLK_RAW_FLAGS) == -1


def test_python_decode_blocks(rx):  # noqa: F811
    names = [c[0] for c in RC.cases()]
    _, blk, sent = RC.cases()[names.index("first-of-later")]
    assert rx.decode_blocks([blk], all_frames=True, raw_flags=True) == [(0, f) for f in sent]
    frames, reps = rx.decode_blocks([blk, blk], all_frames=True, raw_flags=True, report=True)
    assert frames == [(0, f) for f in sent] + [(1, f) for f in sent] and [r.frames for r in reps] == [3, 3]
    assert rx.decode_blocks([blk], all_frames=True) == [(0, sent[0])]
    with pytest.raises(ValueError):
        rx.decode_blocks([blk], raw_flags=True)


# ---------------------------------------------------------------------------------------------------------------------- the pipeline
def _signal():
    """one stream, one channel, 2 MS/s cs16, 0.16 s: bursts of 1, 2 and 3 frames at high SNR; every frame's info holds a byte 0x7e, and
    one frame's info begins with it -> (raw, samples, frames sent per burst)"""
    from vdlm2dec_amd import synth
    rng = np.random.default_rng(23)
    bursts, t = [], 0.003
    for k in (1, 2, 3):
        infos = []
        for j in range(k):
            info = bytearray(rng.integers(0, 256, int(rng.integers(5, 40)), dtype=np.uint8).tolist())
            info[0 if (k, j) == (2, 1) else int(rng.integers(1, len(info)))] = 0x7e
            infos.append(bytes(info))
        b = synth.Burst(chan=0, t0=t, info=b"", infos=infos, amp=40.0, cfo=float(rng.uniform(-200, 200)))
        bursts.append(b)
        t += b.duration() + 0.004
    ns = 327680              # 0.164 s in whole hand-off blocks
    assert t + 0.004 < ns / RATE
    raw = synth.synth_stream(synth.StreamSpec(rate=RATE, fo=[-50000], nsamples=ns, bursts=bursts, seed=5), "cs16")
    return raw, ns, [[synth.hdlc_frame(f) for f in b.frames()] for b in bursts]


def test_pipeline_delivers_frames_that_hold_a_7e(built):
    """With both flags all six frames come out in (end_dec, stream, chn, seq) order and are what was sent; with all_frames alone none of
    them arrives whole; with frames alone the first of each burst; the burst records are the same bytes in all three"""
    from vdlm2dec_amd.demod import Receiver, plan_channels
    raw, ns, sent = _signal()
    assert all(0x7e in f[1:-1] for s in sent for f in s)
    res = {}
    for mode in ("raw", "all", "ref"):
        with Receiver(RATE, plan_channels(S.FC, [-50000]), fmt="cs16", max_push=ns, frames=True, all_frames=mode != "ref",
                      raw_flags=mode == "raw") as r:
            assert (r.all_frames, r.raw_flags) == (mode != "ref", mode == "raw")
            r.push(raw)
            res[mode] = (_poll_records(r), _poll_frames(r), r.stats()["frames_dropped"])
    recs, frames, dropped = res["raw"]
    assert len(recs) == 3 and dropped == 0
    assert [f[4] for f in frames] == [f for s in sent for f in s]
    assert [f[:4] for f in frames] == sorted(f[:4] for f in frames) and [f[3] for f in frames] == [0, 0, 1, 0, 1, 2]
    recs1, frames1, _ = res["all"]
    assert not {f[4] for f in frames1} & {f for s in sent for f in s}
    recs0, frames0, dropped0 = res["ref"]
    assert [f[4] for f in frames0] == [s[0] for s in sent] and [f[3] for f in frames0] == [0, 0, 0] and dropped0 == 0
    assert recs0 == recs and recs1 == recs


def test_dropin_hands_frames_that_hold_a_7e_to_out(built, tmp_path):
    """the -DVDL2GPU_FRAMES build of dropin/vdl2gpu_rcv.c (oracle/_ref/ref_rtl_gpuf: the harness's out() writes an F line per frame):
    with VDL2GPU_RCV_RAW_FLAGS in the environment out() gets all six frames in order"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "oracle", "_ref", "ref_rtl_gpuf")
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/ref_rtl_gpuf not built (needs the reference's sources at build time)")
    # (as in test_gpu_allframes: a binary built from another dropin/vdl2gpu_rcv.c than this tree's is not the program this test is about)
    if b"VDL2GPU_RCV_RAW_FLAGS" not in open(exe, "rb").read():
        pytest.skip("oracle/_ref/ref_rtl_gpuf was not built from this tree's dropin/vdl2gpu_rcv.c: rebuild it (make -C oracle ref)")
    raw, ns, sent = _signal()
    iq = str(tmp_path / "iq.raw")
    raw.tofile(iq)
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = "/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    env.pop("VDL2GPU_RCV_ALL_FRAMES", None)
    env["VDL2GPU_RCV_RAW_FLAGS"] = "1"
    out = str(tmp_path / "out.txt")
    subprocess.run([exe, iq, "cs16", str(RATE), "-50000", str(S.FC - 50000), out, "0", ""], check=True, env=env, timeout=120)
    got = [ln.split()[-1] for ln in open(out) if ln.split()[0] == "F"]
    assert got == [f.hex() for s in sent for f in s]
