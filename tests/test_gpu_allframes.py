"""VDL2GPU_F_ALL_FRAMES on the GPU: crafted burst records through vdl2gpu_decode_blocks_ex with VDL2GPU_BLK_ALL_FRAMES against the CPU
model (tests/allframes_ref.py) and against what the transmitter put into the burst (tests/allframes_cases.py), the report's counts, the
row rules in front of it, mode 0, and the pipeline with the flag and without it."""
import ctypes as C

import numpy as np
import pytest

import allframes_cases as Cs
import allframes_ref as A
import blockrep_ref as BR
import blocks_craft as K
import feedback_ref as FR
import scenarios as S

pytestmark = pytest.mark.gpu

RATE = 2_000_000


@pytest.fixture(scope="module")
def rx(built):
    from vdlm2dec_amd.demod import Receiver, plan_channels
    with Receiver(RATE, plan_channels(S.FC, [-50000]), fmt="cu8", max_push=4096) as r:       # any handle serves the batch call
        yield r


def _fill(ctype, field, maps, n):
    if maps is None:
        return None
    arr = (ctype * n)()
    for i, m in enumerate(maps):
        m = np.ascontiguousarray(m, np.uint8).reshape(8, 255)
        C.memmove(C.addressof(getattr(arr[i], field)), m.ctypes.data, 8 * 255)
    return arr


def _ex(rx, blocks, mode, rels=None, fbs=None, report=True, cap=4096, call="ex"):
    """vdl2gpu_decode_blocks_ex itself (or, call="feedback", vdl2gpu_decode_blocks_feedback):
    ([(block, seq, len, hdata)], dropped, [BlockReport] or None)"""
    from vdlm2dec_amd import demod, lib
    n = len(blocks)
    arr = (lib.BurstT * n)()
    for i, (nbrow, nlbyte, data) in enumerate(blocks):
        arr[i].nbrow, arr[i].nlbyte, arr[i].chn, arr[i].Fr = nbrow, nlbyte, i % 7, 136_975_000 + i
        C.memmove(C.addressof(arr[i].data), bytes(data), 8 * 255)
    sarr, farr = _fill(lib.SoftT, "rel", rels, n), _fill(lib.FbT, "data", fbs, n)
    out = (lib.FrameT * cap)()
    dropped = C.c_int(-1)
    rarr = None
    if report:
        rarr = (lib.BlockRepT * n)()
        C.memset(rarr, 0xa5, C.sizeof(rarr))
    if call == "ex":
        nf = rx.L.vdl2gpu_decode_blocks_ex(rx.h, arr, sarr, farr, n, out, cap, C.byref(dropped), rarr, mode)
    else:
        nf = rx.L.vdl2gpu_decode_blocks_feedback(rx.h, arr, sarr, farr, n, out, cap, C.byref(dropped), rarr)
    assert nf >= 0, rx.L.vdl2gpu_last_error(rx.h)
    for i in range(nf):
        assert (out[i].chn, out[i].Fr, out[i].nbrow, out[i].nlbyte) == (out[i].block % 7, 136_975_000 + out[i].block) + tuple(blocks[out[i].block][:2])
    frames = [(out[i].block, out[i].seq, out[i].len, bytes(out[i].data[:out[i].len])) for i in range(nf)]
    return frames, dropped.value, [demod.BlockReport.from_c(r) for r in rarr] if report else None


def _by_block(frames, n):
    out = [[] for _ in range(n)]
    for block, seq, ln, data in frames:
        assert seq == len(out[block]) and ln == len(data)        # (block, seq) order, seq the rank in the burst
        out[block].append(data)
    return out


@pytest.fixture(scope="module")
def crafted(rx):
    """every crafted case in one call: (names, blocks, sent, frames per block, dropped, reports)"""
    from vdlm2dec_amd import lib
    cs = Cs.cases()
    blocks = [c[1] for c in cs]
    frames, dropped, reps = _ex(rx, blocks, lib.BLK_ALL_FRAMES)
    return [c[0] for c in cs], blocks, [c[2] for c in cs], _by_block(frames, len(blocks)), dropped, reps


def test_crafted_bursts_against_model_and_transmitter(crafted):
    """2 and 3 frames on single flags, 2 / 3 / 70 flags between frames, l = 13 and l = 12 in the middle, a bad FCS in the middle and in
    front, heavy stuffing, frame boundaries on both sides of a row boundary and of a lane's span, two and three flags in one span, fifty
    lanes without one, per = 1, eight rows: the frames are the model's and the transmitter's, the first 12 of a burst at most"""
    names, blocks, sent, got, dropped, reps = crafted
    assert {"two", "three", "flags2", "flags3", "l13", "l12", "badmid", "badfirst", "thirteen", "ff", "rowedge248", "rowedge249",
            "span-first", "span-last", "many13", "long+short", "tiny", "full8"} <= set(names)
    for name, blk, s, g in zip(names, blocks, sent, got):
        model = A.model(*blk)[0]
        assert model == s, name
        assert g == s[:A.NCAND], name
    assert dropped == sum(max(0, len(s) - A.NCAND) for s in sent) == 1 + 138


def test_crafted_bursts_report_counts(crafted):
    names, blocks, sent, got, dropped, reps = crafted
    for name, blk, r in zip(names, blocks, reps):
        cnt = A.model(*blk)[1]
        assert dict(cand=r.cand, too_short=r.too_short, bad_fcs=r.bad_fcs, frames=r.frames) == cnt, name
        assert r.cand == r.too_short + r.bad_fcs + r.frames
        ref = BR.model(*blk)             # everything in front of the candidates is the block path's without the mode
        for f in ("row_roots", "row_how", "row_changed", "bytes_changed", "rows_failed", "rows_rescued", "stuffed", "nbytes", "flag_at", "status"):
            assert getattr(r, f) == getattr(ref, f), (name, f)
        assert r.cand == ref.cand, name
    by = dict(zip(names, reps))
    assert (by["thirteen"].frames, by["many13"].frames) == (13, 150)         # frames counts those that pass, kept or not
    assert by["l12"].too_short == 1 and by["badmid"].bad_fcs == 1 and by["flags70"].too_short == 69


def test_seq_skips_what_does_not_pass(rx, crafted):
    """a middle frame with one FCS bit flipped: frames 1 and 3 arrive as seq 0 and 1; a first frame with a bad FCS: the reference's mode
    gives nothing, this mode the second frame"""
    from vdlm2dec_amd import lib
    names, blocks, sent, got, _, _ = crafted
    i, j = names.index("badmid"), names.index("badfirst")
    assert len(got[i]) == 2 and got[i] == sent[i] and len(got[j]) == 1
    ref, _, _ = _ex(rx, [blocks[i], blocks[j]], 0)
    assert [(b, s) for b, s, _, _ in ref] == [(0, 0)] and ref[0][3] == sent[i][0]
    al, _, _ = _ex(rx, [blocks[i], blocks[j]], lib.BLK_ALL_FRAMES)
    assert [(b, s) for b, s, _, _ in al] == [(0, 0), (0, 1), (1, 0)]


def test_info_bytes_ff_and_7e(rx, crafted):
    """Info bytes of 0xff: the heaviest stuffing, every boundary moves, all frames arrive (case "ff").  Info bytes of 0x7e: the un-stuffer
    hands a stuffed data byte 0x7e on as the byte 0x7e and the rule of include/vdl2gpu.h takes it for a flag, so such a frame is cut and
    does not pass; the kernel gives what the model gives, and of the frames sent those that hold no such byte."""
    from vdlm2dec_amd import lib
    names, _, sent, got, _, _ = crafted
    assert got[names.index("ff")] == sent[names.index("ff")]
    name, blk, s, whole = Cs.info_7e()
    frames, dropped, reps = _ex(rx, [blk], lib.BLK_ALL_FRAMES)
    model, cnt = A.model(*blk)
    assert [f[3] for f in frames] == model == whole and dropped == 0
    assert dict(cand=reps[0].cand, too_short=reps[0].too_short, bad_fcs=reps[0].bad_fcs, frames=reps[0].frames) == cnt


def test_single_frame_bursts_and_edge_blocks_equal_the_model(rx):
    """blocks_craft's records (every eighth): sizes to the last bit, runs of ones, streams no transmitter makes, the flag hunt's edges,
    nested candidates, idle flags -- frames and counts are the model's; where a burst has one frame and no data byte 0x7e, the reference's"""
    from vdlm2dec_amd import lib
    e = [(n, b) for n, b, _ in K.everything()][::8] + BR.many_flags()
    blocks = [b for _, b in e]
    frames, dropped, reps = _ex(rx, blocks, lib.BLK_ALL_FRAMES, cap=8192)
    got = _by_block(frames, len(blocks))
    nref = 0
    for (name, blk), g, r in zip(e, got, reps):
        model, cnt = A.model(*blk)
        assert g == model[:A.NCAND], name
        assert dict(cand=r.cand, too_short=r.too_short, bad_fcs=r.bad_fcs, frames=r.frames) == cnt, name
        nref += len(model) == 1
    assert dropped == sum(max(0, len(A.model(*blk)[0]) - A.NCAND) for _, blk in e) and nref > 60
    ref, _, _ = _ex(rx, blocks, 0, report=False, cap=8192)
    same = [i for i, g in enumerate(_by_block(ref, len(blocks))) if len(g) == 1 and 0x7e not in g[0][1:-1]]
    assert len(same) > 60 and all(got[i] == [f[3] for f in ref if f[0] == i] for i in same)


@pytest.mark.parametrize("how", ["soft", "fb", "soft+fb"])
def test_rescued_row_delivers_the_second_frame(rx, how):
    """the row that carries the second frame has four byte errors: without the row rules only the first frame arrives, with soft=, with fb=
    and with both the second one too; the report says how the row was repaired and counts as the model does"""
    from vdlm2dec_amd import lib
    bad, rel, fb, sent = Cs.rescue()
    plain, _, prep = _ex(rx, [bad], lib.BLK_ALL_FRAMES)
    assert [f[3] for f in plain] == sent[:1] and prep[0].row_how[1] == BR.FAIL and prep[0].frames == 1
    rels, fbs = ([rel] if "soft" in how else None), ([fb] if "fb" in how else None)
    frames, dropped, reps = _ex(rx, [bad], lib.BLK_ALL_FRAMES, rels=rels, fbs=fbs)
    model, cnt = A.model(*bad, rel=rels and rel, fb=fbs and fb)
    assert [f[3] for f in frames] == model == sent and [f[1] for f in frames] == [0, 1] and dropped == 0
    r = reps[0]
    assert dict(cand=r.cand, too_short=r.too_short, bad_fcs=r.bad_fcs, frames=r.frames) == cnt == dict(cand=2, too_short=0, bad_fcs=0, frames=2)
    want = FR.report(bad[2], fbs and fb, rels and rel, bad[0], bad[1])
    for f, v in want.items():
        assert getattr(r, f) == v, f
    assert r.row_how[1] in ((lib.ROW_FEEDBACK,) if fbs else (BR.SOFT2, BR.SOFT4)) and r.rows_rescued == 1 and r.row_changed[1] == 4
    # ... and the same frames from the kernels without a report
    again, _, _ = _ex(rx, [bad], lib.BLK_ALL_FRAMES, rels=rels, fbs=fbs, report=False)
    assert again == frames


def test_mode_0_is_decode_blocks_feedback(rx):
    """the same batch -- crafted bursts, nested candidates, a rescued row -- through vdl2gpu_decode_blocks_ex with mode 0 and through
    vdl2gpu_decode_blocks_feedback: frames, dropped and reports equal; an unknown mode bit is VDL2GPU_EINVAL"""
    from vdlm2dec_amd import lib
    bad, rel, fb, _ = Cs.rescue()
    blocks = [c[1] for c in Cs.cases()] + [b for _, b, _ in K.nested_blocks()] + [bad]
    n = len(blocks)
    none = np.full((8, 255), 255, np.uint8)
    rels, fbs = [none] * (n - 1) + [rel], [np.zeros((8, 255), np.uint8)] * (n - 1) + [fb]
    for kw in (dict(), dict(rels=rels), dict(rels=rels, fbs=fbs), dict(fbs=fbs, report=False)):
        a = _ex(rx, blocks, 0, **kw)
        b = _ex(rx, blocks, 0, call="feedback", **kw)
        assert a == b and len(a[0]) > n // 2
    arr, out = (lib.BurstT * 1)(), (lib.FrameT * 1)()
    assert rx.L.vdl2gpu_decode_blocks_ex(rx.h, arr, None, None, 1, out, 1, None, None, 2) == -1


def test_python_decode_blocks(rx):
    names = [c[0] for c in Cs.cases()]
    i = names.index("three")
    blk, sent = Cs.cases()[i][1], Cs.cases()[i][2]
    assert rx.decode_blocks([blk], all_frames=True) == [(0, f) for f in sent]
    frames, reps = rx.decode_blocks([blk, blk], all_frames=True, report=True)
    assert frames == [(0, f) for f in sent] + [(1, f) for f in sent] and [r.frames for r in reps] == [3, 3]
    assert rx.decode_blocks([blk]) == [(0, sent[0])]


# ---------------------------------------------------------------------------------------------------------------------- the pipeline
def _poll_frames(r):
    from vdlm2dec_amd import lib
    buf = (lib.FrameT * 64)()
    n = r.L.vdl2gpu_poll_frames(r.h, buf, 64)
    assert 0 <= n < 64
    return [(buf[i].end_dec, buf[i].stream, buf[i].chn, buf[i].seq, bytes(buf[i].data[:buf[i].len])) for i in range(n)]


def _poll_records(r):
    from vdlm2dec_amd import lib
    buf = (lib.BurstT * 64)()
    n = r.poll_raw(buf, 64)
    assert 0 <= n < 64
    return [bytes(buf[i]) for i in range(n)]


def _signal():
    """one stream, one channel, 2 MS/s cs16, 0.16 s: bursts of 1, 2 and 3 frames at high SNR -> (raw, samples, frames sent per burst)"""
    from vdlm2dec_amd import synth
    rng = np.random.default_rng(22)
    bursts, t = [], 0.003
    for k in (1, 2, 3):
        while True:      # (no byte 0x7e between a frame's flags, its FCS included: such a frame is cut, see test_info_bytes_ff_and_7e)
            infos = [bytes(rng.integers(0, 256, int(rng.integers(5, 40)), dtype=np.uint8).tolist()) for _ in range(k)]
            b = synth.Burst(chan=0, t0=t, info=b"", infos=infos, amp=40.0, cfo=float(rng.uniform(-200, 200)))
            if not any(0x7e in synth.hdlc_frame(f)[1:-1] for f in b.frames()):
                break
        bursts.append(b)
        t += b.duration() + 0.004
    ns = 327680              # 0.164 s in whole hand-off blocks
    assert t + 0.004 < ns / RATE
    raw = synth.synth_stream(synth.StreamSpec(rate=RATE, fo=[-50000], nsamples=ns, bursts=bursts, seed=5), "cs16")
    return raw, ns, [[synth.hdlc_frame(f) for f in b.frames()] for b in bursts]


def test_pipeline_delivers_every_frame(built):
    """With the flag all six frames come out in (end_dec, stream, chn, seq) order and are what was sent; without it the first of each
    burst; the burst records are the same bytes"""
    from vdlm2dec_amd.demod import Receiver, plan_channels
    raw, ns, sent = _signal()
    res = {}
    for flag in (True, False):
        with Receiver(RATE, plan_channels(S.FC, [-50000]), fmt="cs16", max_push=ns, frames=True, all_frames=flag) as r:
            assert r.all_frames is flag
            r.push(raw)
            res[flag] = (_poll_records(r), _poll_frames(r), r.stats()["frames_dropped"])
    recs, frames, dropped = res[True]
    assert len(recs) == 3 and dropped == 0
    assert [f[4] for f in frames] == [f for s in sent for f in s]
    assert [f[:4] for f in frames] == sorted(f[:4] for f in frames) and [f[3] for f in frames] == [0, 0, 1, 0, 1, 2]
    recs0, frames0, dropped0 = res[False]
    assert [f[4] for f in frames0] == [s[0] for s in sent] and [f[3] for f in frames0] == [0, 0, 0] and dropped0 == 0
    assert recs0 == recs


def test_dropin_hands_every_frame_to_out(built, tmp_path):
    """the -DVDL2GPU_FRAMES build of dropin/vdl2gpu_rcv.c (oracle/_ref/ref_rtl_gpuf: the harness's out() writes an F line per frame):
    with VDL2GPU_RCV_ALL_FRAMES in the environment out() gets all six frames in order, without it the first of each burst"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "oracle", "_ref", "ref_rtl_gpuf")
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/ref_rtl_gpuf not built (needs the reference's sources at build time)")
    # oracle/_ref is a build product that only a machine with the reference's sources can make: where the binary at hand was built from
    # another dropin/vdl2gpu_rcv.c than this tree's (it does not hold the switch's name), it is not the program this test is about
    if b"VDL2GPU_RCV_ALL_FRAMES" not in open(exe, "rb").read():
        pytest.skip("oracle/_ref/ref_rtl_gpuf was not built from this tree's dropin/vdl2gpu_rcv.c: rebuild it (make -C oracle ref)")
    raw, ns, sent = _signal()
    iq = str(tmp_path / "iq.raw")
    raw.tofile(iq)
    got = {}
    for flag in (True, False):
        env = dict(os.environ)
        env["LD_LIBRARY_PATH"] = "/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
        env.pop("VDL2GPU_RCV_ALL_FRAMES", None)
        if flag:
            env["VDL2GPU_RCV_ALL_FRAMES"] = "1"
        out = str(tmp_path / f"out{int(flag)}.txt")
        subprocess.run([exe, iq, "cs16", str(RATE), "-50000", str(S.FC - 50000), out, "0", ""], check=True, env=env, timeout=120)
        got[flag] = [ln.split()[-1] for ln in open(out) if ln.split()[0] == "F"]
    assert got[True] == [f.hex() for s in sent for f in s]
    assert got[False] == [s[0].hex() for s in sent]
