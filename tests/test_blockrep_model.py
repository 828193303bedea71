"""The CPU model of the block report (tests/blockrep_ref.py) held to the oracle: its `frames` to oracle.frames_of_block (hard mode)
and soft_ref.soft_frames (soft mode), its candidate counts to blocks_craft.unstuff_ref where no row is touched, on the crafted
records of tests/blocks_craft.py, on variants of them with byte errors in one row (seeds fixed) and on tests/soft_cases.py.  The GPU
tests (tests/test_gpu_blockrep.py) then hold the kernel to the model by equality."""
import collections

import numpy as np

import blockrep_ref as M
import blocks_craft as K
import soft_cases
import soft_ref as R


def _identity(rep):
    assert rep.status == 0
    assert rep.cand == rep.too_short + rep.bad_fcs + rep.frames
    assert rep.bytes_changed == sum(rep.row_changed)
    assert rep.rows_failed == rep.row_how.count(M.FAIL)
    assert rep.rows_rescued == rep.row_how.count(M.SOFT2) + rep.row_how.count(M.SOFT4)


def _raw(block):
    nbrow, nlbyte, data = block
    return b"".join(data[255 * r:255 * r + (nlbyte if r == nbrow - 1 else 249)] for r in range(nbrow))


def test_crafted_blocks(oracle):
    """all of blocks_craft.everything(): frames as the oracle's block path, candidates as the un-stuffing loop itself"""
    seen = collections.Counter()
    entries = K.everything()
    assert len(entries) == 1013
    for name, block, _ in entries:
        rep = M.model(*block)
        _identity(rep)
        assert rep.frames == len(oracle.frames_of_block(*block)), name
        assert rep.row_how[block[0]:] == (M.NONE,) * (8 - block[0]) and rep.row_roots[block[0]:] == (0,) * (8 - block[0]), name
        if all(h == M.CLEAN for h in rep.row_how[:block[0]]):
            u = K.unstuff_ref(_raw(block))
            assert rep.bytes_changed == 0 and rep.row_roots == (0,) * 8, name
            assert rep.cand == len(u.cands) and rep.too_short == sum(l < 13 for l in u.cands), name
            assert rep.nbytes == (8 * len(_raw(block)) - rep.stuffed) // 8, name
            assert (rep.flag_at >= 0) == (u.k >= 1), name
            seen["clean"] += 1
        seen["too_short"] += rep.too_short > 0
        seen["bad_fcs"] += rep.bad_fcs > 0
        seen["noflag"] += rep.flag_at == -1
        seen["many"] += rep.frames >= 13
    assert seen["clean"] >= 100      # (a short last row is not clean: its unsent parity is received as zeros and restored as erasures)
    for what in ("too_short", "bad_fcs", "noflag", "many"):
        assert seen[what] > 0, what


def test_corrupted_variants(oracle):
    """1, 3, 4, 5 or 9 byte errors in one row, without and with a reliability map that marks them; and rows the soft rule cannot
    rescue.  Every row outcome occurs: CLEAN, REF, FAIL in hard mode (there is no trial there); all five in soft mode."""
    hard, soft = collections.Counter(), collections.Counter()
    cases = M.variants() + M.soft_fail_cases()
    assert len(cases) > 600
    for name, block, rel, nerr in cases:
        rep = M.model(*block)
        _identity(rep)
        assert rep.frames == len(oracle.frames_of_block(*block)), name
        assert rep.rows_rescued == 0, name
        hard.update(rep.row_how[:block[0]])
        srep = M.model(*block, rel=rel)
        _identity(srep)
        assert srep.frames == len(R.soft_frames(np.frombuffer(block[2], np.uint8), rel, block[0], block[1])), name
        assert srep.row_roots == rep.row_roots, name      # the reference's run on the received row, in either mode
        soft.update(srep.row_how[:block[0]])
        if nerr <= 3 and block[1] > 67:                   # no row has fixed erasures: up to three errors are within the code's reach
            assert rep.bytes_changed == nerr and rep.rows_failed == 0, name
    assert set(hard) == {M.CLEAN, M.REF, M.FAIL}
    assert set(soft) == {M.CLEAN, M.REF, M.SOFT2, M.SOFT4, M.FAIL}
    for name, block, rel, _ in M.soft_fail_cases():
        assert M.model(*block, rel=rel).rows_failed == 1, name


def test_soft_cases(oracle):
    soft = collections.Counter()
    for nbrow, nlbyte, data, rel, sent, r, nerr, _ in soft_cases.cases():
        rep = M.model(nbrow, nlbyte, data.tobytes(), rel=rel)
        _identity(rep)
        assert rep.frames == len(R.soft_frames(data, rel, nbrow, nlbyte))
        blk, how = R.row_rule(data, rel, nbrow, nlbyte)
        want = {"s2": M.SOFT2, "s4": M.SOFT4, "fail": M.FAIL}
        assert [rep.row_how[i] for i in range(nbrow) if how[i] != "ref"] == [want[h] for h in how if h != "ref"]
        if np.array_equal(blk[r], sent[r]):               # the row came back as sent (not a miscorrection): every error was changed
            assert rep.row_changed[r] == nerr
        soft.update(rep.row_how[:nbrow])
    assert soft[M.SOFT2] and soft[M.SOFT4] and soft[M.FAIL]


def test_many_flags(oracle):
    """bursts of idle flags: the candidate counters far beyond 1023, against the un-stuffing loop itself and the oracle's frames"""
    big = 0
    for name, block in M.many_flags():
        rep = M.model(*block)
        _identity(rep)
        assert rep.rows_failed == 0 and rep.bytes_changed == 0, name      # the un-stuffer reads the rows as received
        u = K.unstuff_ref(_raw(block))
        assert rep.cand == len(u.cands) and rep.too_short == sum(l < 13 for l in u.cands), name
        assert rep.frames == len(oracle.frames_of_block(*block, cap=1 << 16)), name
        big += rep.bad_fcs >= 1024
    want = {name: M.model(*block) for name, block in M.many_flags()}
    assert (want["flags1980"].cand, want["flags1980"].bad_fcs, want["flags1980"].frames) == (1980, 1970, 0)
    assert want["flags1023"].bad_fcs == 1013 and want["flags1034"].bad_fcs == 1024 and want["flags1034"].too_short == 10
    f = want["frame+flags"]
    assert (f.cand, f.too_short, f.bad_fcs, f.frames) == (1501, 0, 1500, 1)
    assert big >= 5


def test_header_out_of_range():
    z = (0,) * 8
    for nbrow, nlbyte in ((0, 10), (9, 10), (1, 250), (-1, 0), (1, -1)):
        rep = M.model(nbrow, nlbyte, bytes(2040))
        assert rep.status == 1 and rep == M._zero(1) and rep.row_how == z
