"""tests/blocks_craft.py against the oracle alone (no GPU): every crafted record gives the number of frames its builder means it
to give, and the plain-Python un-stuffing loop the builders steer by is the oracle's."""
import numpy as np
import pytest

import blocks_craft as K
from vdlm2dec_amd import synth

CAP = 1 << 16


def _raw_of(block) -> bytes:
    nbrow, nlbyte, data = block
    rows = np.frombuffer(data, np.uint8).reshape(8, 255)
    return b"".join(rows[r, :249 if r < nbrow - 1 else nlbyte].tobytes() for r in range(nbrow))


@pytest.mark.parametrize("group", ["sizes", "one_runs", "streams", "flag_hunt", "thresholds", "nested_blocks"])
def test_crafted_blocks_give_what_their_builders_intend(oracle, group):
    entries = getattr(K, group)()
    assert len(entries) >= {"sizes": 30, "one_runs": 651, "streams": 300, "flag_hunt": 18, "thresholds": 3, "nested_blocks": 11}[group]
    for name, block, intended in entries:
        frames = oracle.frames_of_block(*block, cap=CAP)
        assert len(frames) == intended, (name, len(frames))
        u = K.unstuff_ref(_raw_of(block))          # the rows are codewords: rs() leaves them alone (sizes(): but for one)
        if intended:
            assert [len(f) for f in frames] == [l for l in u.cands if len(frames) and bytes(u.hdata[:l]) in frames], name
            for f in frames:
                assert f == bytes(u.hdata[:len(f)]), name
        assert 1 <= block[0] <= 8 and 0 <= block[1] <= 249


def test_stuff_and_unstuff_are_inverse():
    rng = np.random.default_rng(1)
    for t0 in (0, 3, 5, 6, 9):
        bits = [int(b) for b in rng.integers(0, 2, 4000)] + [1] * 40 + [0, 1, 1, 1, 1, 1, 0, 1, 1, 1, 1, 1, 1]
        st = K.stuff(bits, t0)
        lead = K.FLAG + [0] * 9 + [1] * t0               # a flag, so that bytes are kept; then the run as the receiver has counted it
        u = K._unstuff_bits(lead + st)
        assert u.t == 1 and len(st) > len(bits)         # (the last six ones went out as 111110 1)
        got = [(u.hdata[i // 8] >> (i % 8)) & 1 for i in range(8 * len(u.hdata))][len(lead):len(lead) + len(bits)]
        assert got == bits and 8 * u.k + u.s == len(lead) + len(bits), t0
    assert K.bytes_of(K.bits_of(b"\x7e\x01\x80")) == b"\x7e\x01\x80" and K.bits_of(b"\x7e") == K.FLAG


def test_unstuff_ref_on_a_transmitted_payload(oracle):
    info = bytes(range(200, 256)) * 3
    raw = synth.hdlc_payload(synth.avlc_frame(info))
    u = K.unstuff_ref(raw)
    frames = oracle.frames_of_block(*synth.received_rows(raw))
    assert len(frames) == 1 and frames[0] == bytes(u.hdata[:u.cands[-1]]) and raw == K.frame(synth.avlc_frame(info))


def test_the_edges_are_there(oracle):
    """what the sets are for: the lengths, the runs, the lanes of 0xff, more than one frame a burst, more than the table of 12"""
    assert sorted({len(_raw_of(b)) for n, b, _ in K.sizes()}) == sorted(K.SIZES)
    assert any(1992 - 8 <= len(_raw_of(b)) <= 1992 for _, b, _ in K.one_runs())
    lanes = 0
    runs = set()
    for _, b, _ in K.streams():
        raw = _raw_of(b)
        per = (len(raw) + 63) // 64
        lanes += (b"\xff" * (3 * per)) in raw
        bits = "".join(map(str, K.bits_of(raw)))
        runs |= {len(r) for r in bits.split("0")}
    assert lanes >= 10 and set(range(5, 41)) <= runs
    assert {b[0] for _, b, _ in K.streams()} == set(range(1, 9))
    assert [i for _, _, i in K.thresholds()] == [0, 1, 1]
    assert sorted({i for _, _, i in K.nested_blocks()}) == sorted(K.NESTED)
    for name, b, _ in K.nested_blocks():
        fr = oracle.frames_of_block(*b, cap=CAP)
        assert all(fr[i] == fr[i + 1][:len(fr[i])] for i in range(len(fr) - 1)), name       # they share their start
        if name.endswith("-7e"):
            assert len(K.unstuff_ref(_raw_of(b)).cands) > len(fr), name                    # failing candidates in between
