"""The block kernel (k4_frames) at its edges, against the reference's blk_thread as the oracle restates it: the records of
tests/blocks_craft.py -- un-stuffing over lane, word and row boundaries, streams no transmitter makes, the flag hunt, the length
threshold, nested candidates and the table of 12, max_frames, the grid-stride loop.  tests/test_blocks_craft.py holds the records to
what they are meant to be; every test here also asserts the size of the list it compares."""
import collections
import ctypes as C

import pytest

import blocks_craft as K
import scenarios as S

pytestmark = pytest.mark.gpu
CAP = 1 << 16


@pytest.fixture(scope="module")
def rx(built):
    from vdlm2dec_amd.demod import Receiver, plan_channels
    with Receiver(2_000_000, plan_channels(S.FC, [-50000]), fmt="cu8", max_push=4096) as r:
        yield r


_cache = {}


def _frames(oracle, block):
    if block not in _cache:
        _cache[block] = oracle.frames_of_block(*block, cap=CAP)
    return _cache[block]


def _want(oracle, blocks):
    return [(i, f) for i, b in enumerate(blocks) for f in _frames(oracle, b)]


def _compare(rx, oracle, entries, max_frames=0):
    blocks = [b for _, b, _ in entries]
    want = _want(oracle, blocks)
    assert len(want) == sum(i for _, _, i in entries)
    got = rx.decode_blocks(blocks, max_frames=max_frames)
    if got != want:
        bad = sorted({i for i, _ in set(got) ^ set(want)})
        assert not bad, [entries[i][0] for i in bad[:20]]
    assert got == want
    return want


def test_sizes(rx, oracle):
    """a frame that fills 13 .. 1992 data bytes to the last bit (one byte a lane, up to 32; empty trailing lanes), and the same with
    the closing flag's last bit cut off"""
    want = _compare(rx, oracle, K.sizes())
    assert len(want) == 14 and len(K.sizes()) == 30


def test_one_runs_across_lanes(rx, oracle):
    assert len(_compare(rx, oracle, K.one_runs())) == 651


def test_streams_no_transmitter_makes(rx, oracle):
    assert len(_compare(rx, oracle, K.streams())) == 300


def test_flag_hunt(rx, oracle):
    e = K.flag_hunt()
    got = dict((n, i) for n, _, i in e)
    assert got["stray01"] == 0 and got["stray01-without"] == 1 and got["stray80"] == 0 and got["stray80-without"] == 1
    assert len(_compare(rx, oracle, e)) == len(e) - 2


def test_length_threshold(rx, oracle):
    want = _compare(rx, oracle, K.thresholds())
    assert [len(f) for _, f in want] == [13, 14]


def _direct(rx, blocks, max_frames):
    """vdl2gpu_decode_blocks itself: Receiver.decode_blocks refuses a result with frames dropped"""
    from vdlm2dec_amd import lib
    arr = (lib.BurstT * len(blocks))()
    for i, (nbrow, nlbyte, data) in enumerate(blocks):
        arr[i].nbrow, arr[i].nlbyte = nbrow, nlbyte
        C.memmove(C.addressof(arr[i].data), data, 8 * 255)
    out = (lib.FrameT * max_frames)()
    dropped = C.c_int(-1)
    nf = rx.L.vdl2gpu_decode_blocks(rx.h, arr, len(blocks), out, max_frames, C.byref(dropped))
    assert nf >= 0
    return [(out[i].block, out[i].seq, bytes(out[i].data[:out[i].len])) for i in range(nf)], dropped.value


def test_nested_candidates(rx, oracle):
    """m candidates that share their start, data bytes 0x7e between them: up to the table's 12 in order and length; of 13 and 14, 12
    distinct ones and the rest counted"""
    e = K.nested_blocks()
    small = [x for x in e if x[2] <= 12]
    want = _compare(rx, oracle, small, max_frames=64)       # (the default room is four frames a record)
    assert len(want) == 2 * (2 + 3 + 12) + 3
    got, dropped = _direct(rx, [b for _, b, _ in small], len(want))
    assert dropped == 0 and [(i, f) for i, _, f in got] == want
    assert [s for _, s, _ in got] == [s for _, b, _ in small for s in range(len(_frames(oracle, b)))]        # seq counts within a burst
    for name, b, m in e:
        if m > 12:
            frames = _frames(oracle, b)
            assert len(frames) == m
            got, dropped = _direct(rx, [b], 64)
            assert dropped == m - 12 and len(got) == 12, name
            assert len({f for _, _, f in got}) == 12 and all(f in frames for _, _, f in got), name
            assert [s for _, s, _ in got] == list(range(12))


def test_max_frames(rx, oracle):
    e = K.nested_blocks()[:6] + K.flag_hunt() + K.thresholds()
    blocks = [b for _, b, _ in e]
    want = collections.Counter(_want(oracle, blocks))
    F = sum(want.values())
    assert F == sum(i for _, _, i in e) and F > 40
    got, dropped = _direct(rx, blocks, F - 3)
    assert len(got) == F - 3 and dropped == 3
    assert len({(i, s) for i, s, _ in got}) == F - 3
    assert not collections.Counter((i, f) for i, _, f in got) - want
    got, dropped = _direct(rx, blocks, F)
    assert dropped == 0 and collections.Counter((i, f) for i, _, f in got) == want


def test_grid_stride(rx, oracle):
    """more than two grids of records (vdl2gpu_decode_blocks launches at most 32 blocks a compute unit), with records the kernel has
    to skip between them"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 2 * 32 * cus + 37
    assert n > 32 * cus
    pool = [x for x in K.everything() if x[1][0] <= 2 and x[2] <= 12]       # (more than 12 frames a burst: test_nested_candidates)
    assert len(pool) > 700
    skips = [(0, 10), (9, 10), (2, -1), (2, 250)]
    data = pool[0][1][2]
    blocks, want = [], []
    k = 0
    while len(blocks) < n:
        if len(blocks) % 51 == 50:
            nbrow, nlbyte = skips[(len(blocks) // 51) % 4]
            blocks.append((nbrow, nlbyte, data))      # (the rows of a frame: it is the header that has to stop the kernel)
            continue
        b = pool[k % len(pool)][1]
        k += 1
        want += [(len(blocks), f) for f in _frames(oracle, b)]
        blocks.append(b)
    assert len(blocks) == n and len(want) > n // 2 and sum(1 for b in blocks if b[0] in (0, 9) or b[1] in (-1, 250)) >= n // 51
    got = rx.decode_blocks(blocks, max_frames=len(want) + 64)
    assert got == want
