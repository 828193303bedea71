"""The CPU model of VDL2GPU_F_ALL_FRAMES (tests/allframes_ref.py) against the transmitter: what hdlc_payload_multi puts into a burst comes
out byte for byte, in order.  And the premise of the mode: the reference's block path (oracle.frames_of_block) gives exactly the first
frame of such a burst."""
import numpy as np
import pytest

from vdlm2dec_amd import synth

import allframes_cases as Cs
import allframes_ref as A
import blocks_craft as K


def _frames(rng, n, lo=0, hi=60):
    """n AVLC frames with distinct src addresses and no byte 0x7e between their flags, the FCS included (such a frame is cut: see
    test_a_data_byte_7e_cuts_its_frame)"""
    out = []
    while len(out) < n:
        f = synth.avlc_frame(bytes(rng.integers(0, 256, int(rng.integers(lo, hi + 1)), dtype=np.uint8).tolist()), src=(1 << 24) | (0x400000 + len(out)))
        if 0x7e not in synth.hdlc_frame(f)[1:-1]:
            out.append(f)
    return out


@pytest.mark.parametrize("nframes,flags", [(1, 1), (2, 1), (3, 1), (5, 1), (2, 2), (3, 3), (12, 1)])
def test_model_returns_what_the_transmitter_sent(oracle, nframes, flags):
    rng = np.random.default_rng(100 * nframes + flags)
    for _ in range(6):
        sent = _frames(rng, nframes)
        blk = K.block_of(synth.hdlc_payload_multi(sent, flags_between=flags))
        got, cnt = A.model(*blk)
        assert got == [synth.hdlc_frame(f) for f in sent]
        assert cnt == dict(cand=nframes + (nframes - 1) * (flags - 1), too_short=(nframes - 1) * (flags - 1), bad_fcs=0, frames=nframes)
        # the reference: every candidate starts at hdata[1], so only the first frame can check
        assert oracle.frames_of_block(*blk) == [synth.hdlc_frame(sent[0])]


def test_burst_objects_with_several_infos(oracle):
    b = synth.Burst(chan=1, t0=0.0, info=b"", infos=[b"", b"abc", bytes(range(40))])
    blk = K.block_of(b.payload())
    want = [synth.hdlc_frame(f) for f in b.frames()]
    assert A.model(*blk)[0] == want and len(want[0]) == 13
    assert oracle.frames_of_block(*blk) == want[:1]


@pytest.mark.parametrize("case", Cs.cases(), ids=[c[0] for c in Cs.cases()])
def test_crafted_cases_give_what_they_mean_to(oracle, case):
    name, blk, sent = case
    got, cnt = A.model(*blk)
    assert got == sent
    assert cnt["frames"] == len(sent) and cnt["cand"] == cnt["too_short"] + cnt["bad_fcs"] + cnt["frames"]
    ref = oracle.frames_of_block(*blk)
    if name == "badfirst":
        assert ref == [] and len(got) == 1          # the reference never gets past a first frame that fails
    else:
        assert ref == sent[:1]                      # ... and never beyond one that checks


def test_single_frame_bursts_are_the_reference(oracle):
    """segment 0 is the reference's first candidate: on blocks_craft's one-frame bursts that hold no data byte 0x7e the mode changes nothing"""
    n = 0
    for name, blk, want in K.sizes() + K.flag_hunt() + K.thresholds() + K.one_runs()[::25]:
        ref = oracle.frames_of_block(*blk)
        if any(0x7e in f[1:-1] for f in ref):
            continue
        assert A.model(*blk)[0] == ref, name
        n += 1
    assert n > 40


def test_a_data_byte_7e_cuts_its_frame():
    """the un-stuffer hands a stuffed data byte 0x7e on as the byte 0x7e, and the rule takes it for a flag (include/vdl2gpu.h)"""
    name, blk, sent, whole = Cs.info_7e()
    got, cnt = A.model(*blk)
    assert got == whole and len(whole) == 2 and len(sent) == 4
    assert cnt["cand"] == cnt["too_short"] + cnt["bad_fcs"] + cnt["frames"]


def test_rows_go_through_the_row_rule():
    bad, rel, fb, sent = Cs.rescue()
    assert A.model(*bad)[0] == sent[:1]             # rs() cannot repair the second frame's row
    assert A.model(*bad, rel=rel)[0] == sent and A.model(*bad, fb=fb)[0] == sent and A.model(*bad, rel=rel, fb=fb)[0] == sent
