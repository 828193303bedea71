"""The CPU model of VDL2GPU_F_RAW_FLAGS (tests/rawflags_ref.py) held to three things: the transmitter -- what hdlc_payload_multi puts
into a burst of frames of unrestricted bytes comes out byte for byte, in order; the model of VDL2GPU_F_ALL_FRAMES wherever no un-stuffed
byte 0x7e has a dropped zero inside; and the equivalence of the rule's two forms, on streams no transmitter makes as well."""
import numpy as np
import pytest

from vdlm2dec_amd import synth

import allframes_cases as Cs
import allframes_ref as A
import blockrep_ref as BR
import blocks_craft as K
import rawflags_cases as RC
import rawflags_ref as R


def _bodies(rng, n, total):
    """n bodies of 9 random bytes and more, any value, `total` bytes at most between them"""
    hi = min(249, total // n - 4)
    return [bytes(rng.integers(0, 256, int(rng.integers(9, hi + 1)), dtype=np.uint8).tolist()) for _ in range(n)]


@pytest.mark.parametrize("nframes", [1, 2, 3, 5, 12])
def test_model_returns_what_the_transmitter_sent(nframes):
    rng = np.random.default_rng(700 + nframes)
    with7e = cut = 0
    for _ in range(60):
        while True:     # (a last row of 1 or 2 bytes has no parity sent and does not survive rs(), see blocks_craft.sizes(): not such a burst)
            sent = _bodies(rng, nframes, 1800)
            blk = K.block_of(synth.hdlc_payload_multi(sent))
            if blk[1] > 2:
                break
        got, cnt = R.model(*blk)
        assert got == [synth.hdlc_frame(f) for f in sent]
        assert cnt == dict(cand=nframes, too_short=0, bad_fcs=0, frames=nframes)
        with7e += any(0x7e in synth.hdlc_frame(f)[1:-1] for f in sent)
        cut += A.model(*blk)[0] != got
    assert with7e > 5 and cut == with7e         # the all-frames rule loses exactly the bursts that hold such a byte


def test_a_first_byte_7e_is_kept():
    """m1 is the first byte behind the first flag that is no TRUE flag: a frame that begins with a data byte 0x7e keeps it"""
    names = [c[0] for c in RC.cases()]
    for n in ("first-of-first", "first-of-first-flags3"):
        _, blk, sent = RC.cases()[names.index(n)]
        assert sent[0][:2] == b"\x7e\x7e" and R.model(*blk)[0] == sent


@pytest.mark.parametrize("case", RC.cases(), ids=[c[0] for c in RC.cases()])
def test_crafted_cases_give_what_they_mean_to(case):
    name, blk, sent = case
    got, cnt = R.model(*blk)
    assert got == sent
    assert cnt["frames"] == len(sent) and cnt["cand"] == cnt["too_short"] + cnt["bad_fcs"] + cnt["frames"]
    assert R.has_data_7e(*blk) and RC.data_drops(blk)
    assert R.model(*blk, by_drop=True) == (got, cnt)


def test_crafted_cases_are_where_they_mean_to_be():
    by = {c[0]: c for c in RC.cases()}
    assert RC.data_drops(by["drop-bit7"][1])[0][0] % 8 == 7 and RC.data_drops(by["drop-bit0"][1])[0][0] % 8 == 0
    assert RC.data_drops(by["drop-row-last"][1])[0][0] == 8 * 249 - 1 and RC.data_drops(by["drop-row-first"][1])[0][0] == 8 * 249
    for name, bit in (("drop-span-last", 7), ("drop-span-first", 0)):
        blk = by[name][1]
        p = RC.data_drops(blk)[0][0]
        per = (RC.raw_bytes(blk) + 63) // 64
        assert per > 1 and p % 8 == bit and (p // 8) % per == (per - 1 if bit else 0)
    assert {q % 32 for _, q in RC.data_drops(by["mark31"][1])} == {31} and {q % 32 for _, q in RC.data_drops(by["mark32"][1])} == {0}
    for name, at in (("span-first", 0), ("span-last", -1)):
        blk = by[name][1]
        nb = len(R.unstuff(b"".join(np.frombuffer(blk[2], np.uint8).reshape(8, 255)[r, :(blk[1] if r == blk[0] - 1 else 249)].tobytes()
                                    for r in range(blk[0])))[0])
        per = (nb + 63) // 64
        assert per > 1 and any(q % per == at % per for _, q in RC.data_drops(blk))
    assert len(by["many13"][2]) == 150 and by["full8"][1][0] == 8
    assert len(R.unstuff(bytes(by["tiny"][1][2][:by["tiny"][1][1]]))[0]) <= 64           # per = 1
    for which, name in ((0, "fcs-low"), (1, "fcs-high")):
        assert by[name][2][1][-3 + which] == 0x7e and 0x7e not in by[name][2][1][1:-3]
    cnt = R.model(*by["badfcs"][1])[1]
    assert cnt == dict(cand=3, too_short=0, bad_fcs=1, frames=2)


def test_nested_frame():
    """body = X | fcs(X) | 7e | Y: the all-frames rule delivers the inner X, which was never sent; this one the whole frame and nothing else"""
    blk, whole, inner = RC.nested()
    assert A.model(*blk)[0] == [inner]
    assert R.model(*blk) == ([whole], dict(cand=1, too_short=0, bad_fcs=0, frames=1))


def test_info_7e_all_four_arrive():
    name, blk, sent, whole = Cs.info_7e()
    assert R.model(*blk)[0] == sent and len(sent) == 4 and A.model(*blk)[0] == whole and len(whole) == 2


def test_equal_to_the_all_frames_model_without_a_data_7e():
    """a burst without a data byte 0x7e between its flags: the same frames and counts with and without the mode"""
    blocks = [(c[0], c[1]) for c in Cs.cases()] + [(n, b) for n, b, _ in K.everything()][::8] + list(BR.many_flags())
    same = differ = 0
    for name, blk in blocks:
        if R.has_data_7e(*blk):
            differ += 1
            continue
        assert R.model(*blk) == A.model(*blk), name
        same += 1
    assert same > 100 and all(not R.has_data_7e(*c[1]) for c in Cs.cases())


def test_the_two_forms_of_the_rule_agree():
    """t7 == 6 and "no zero dropped at un-stuffed bit offset 8q + 6" are the same statement for a byte that un-stuffs to 0x7e, and t7 is
    1 for the others: on blocks_craft's records, which hold streams no transmitter makes"""
    n7e = ndata = 0
    for name, blk, _ in K.everything():
        nbrow, nlbyte, data = blk
        if not (1 <= nbrow <= 8 and 0 <= nlbyte <= 249):
            continue
        B, t7, drops = R.unstuff(R.source(nbrow, nlbyte, data, None, None))
        assert R.true_flags(B, t7) == R.true_flags_by_drop(B, drops), name
        for q, v in enumerate(B):
            if v == 0x7e:
                n7e += 1
                assert t7[q] in (1, 6) and not any(8 * q + n in drops for n in (1, 2, 3, 4, 5, 7)), name
                ndata += t7[q] == 1
    assert n7e > 1000 and ndata > 20


def test_rows_go_through_the_row_rule():
    bad, rel, fb, sent = RC.rescue()
    assert 0x7e in sent[1][1:-1]
    assert R.model(*bad)[0] == sent[:1]             # rs() cannot repair the second frame's row
    assert R.model(*bad, rel=rel)[0] == sent and R.model(*bad, fb=fb)[0] == sent and R.model(*bad, rel=rel, fb=fb)[0] == sent
