"""The widest handles: 64 and 65 streams of 8 channels (512 and 520 channel slots, slot = stream * 8 + channel), every stream a
different recording with its own channel plan, every stream against its own oracle run -- records, df / ppm bits, Fr and the
stream index.  The rest of the suite runs real data in slots below 80 only.

  * 64 streams is the widest handle whose speculative payload decode uses the 16-word redo mask (sel_mode 1, S * 8 <= 512);
    with the region scan dropped, repairs reach every word of it.  65 streams take the repaired selection (sel_mode 2).
  * With max_push = 1 << 25 the planes of the upper streams lie more than 4 GiB behind the first plane of the handle."""
import functools
from concurrent.futures import ThreadPoolExecutor
from types import SimpleNamespace

import numpy as np
import pytest

import scenarios as S
from test_gpu_levels import _check_exact
from vdlm2dec_amd import lib

pytestmark = pytest.mark.gpu

RATE = 2_000_000


@functools.lru_cache(maxsize=None)
def _inputs(n):
    return S.distinct_streams(n)


def _oracle(O, ins):
    """every stream's bursts on the CPU, the streams side by side (the oracle's calls release the GIL)"""
    with ThreadPoolExecutor(16) as ex:
        return list(ex.map(lambda x: O.run_oracle(x[0], "cs16", RATE, x[1], x[2]), ins))


def _rx(ins, **kw):
    from vdlm2dec_amd.demod import Receiver, plan_channels
    return Receiver(RATE, [plan_channels(fc, fo) for _, fo, fc in ins], fmt="cs16", **kw)


def _bits(x):
    return np.float32(x).view(np.uint32).item()


def _rec(b):
    return (b.chn, b.trig_dec, b.end_dec, b.nbrow, b.nlbyte, b.data, _bits(b.df), _bits(b.ppm))


def _check(got, want, ins):
    """every stream's records are its oracle's, each once, and carry that stream's index and channel frequencies"""
    by = {}
    for b in got:
        by.setdefault(b.stream, []).append(b)
    assert set(by) <= set(range(len(ins))), sorted(set(by) - set(range(len(ins))))
    for s, (_, fo, fc) in enumerate(ins):
        mine = by.get(s, [])
        assert sorted(_rec(b) for b in mine) == sorted(_rec(b) for b in want[s]), s
        assert all(b.Fr == fc + fo[b.chn] for b in mine), s
    assert len(got) == sum(len(w) for w in want)
    assert min(len(w) for w in want) >= 20


def _frames(O, want):
    return sorted((b.chn, f) for b in want for f in O.frames_of_block(b.nbrow, b.nlbyte, b.data))


@pytest.mark.timeout(300)
def test_64_streams_of_8_channels(built, oracle):
    ins = _inputs(64)
    want = _oracle(oracle, ins)
    raw = np.stack([r for r, _, _ in ins])
    n = raw.shape[1] // 2
    got = []
    with _rx(ins, max_push=1 << 19) as rx:
        pos = 0
        for k in (300_001, 524_288, 99_999, n):
            e = min(n, pos + k)
            rx.push(raw[:, 2 * pos:2 * e])
            got += rx.poll_ready()
            pos = e
        got += rx.poll()
        st = rx.stats()
    assert pos == n
    _check(got, want, ins)
    assert st["serial_redos"] == 0, st


@pytest.mark.timeout(300)
def test_64_streams_with_repairs_in_every_mask_word(built, oracle, monkeypatch):
    """The region scan dropped: nearly every burst needs a repair round, in all 512 slots, so all 16 words of the redo mask are
    written and read.  Records, frames (K4 reads the mask too) and levels after the repairs are the oracle's / the definition's.
    stats.repairs counts the whole handle: the last 8 streams' inputs on a handle of their own show that the top slots are
    repaired as well."""
    monkeypatch.setenv("VDL2GPU_REPAIR_ROUNDS", "2")
    ins = _inputs(64)
    want = _oracle(oracle, ins)
    raw = np.stack([r for r, _, _ in ins])
    n = raw.shape[1] // 2
    with _rx(ins, max_push=n, keep_dec=True, frames=True, levels=True, flags=lib.F_TEST_NOREGION) as rx:
        rx.push(raw)
        got = rx.poll()
        frames = rx.poll_frames()
        st = rx.stats()
        assert st["repairs"] > 0, st
        _check(got, want, ins)
        for s in range(64):
            assert sorted((c, f) for t, c, f in frames if t == s) == _frames(oracle, want[s]), s
        assert len(frames) == sum(len(_frames(oracle, w)) for w in want) and st["frames_dropped"] == 0
        for s in (0, 31, 63):
            _check_exact(rx, [b for b in got if b.stream == s], SimpleNamespace(rate=RATE), "cs16")
    with _rx(ins[56:], max_push=n, flags=lib.F_TEST_NOREGION) as rx:
        rx.push(raw[56:])
        top = rx.poll()
        st8 = rx.stats()
    assert st8["repairs"] > 0, st8
    _check(top, want[56:], ins[56:])


@pytest.mark.timeout(300)
def test_the_512_slot_edge_from_both_sides(built, oracle):
    """The same distinct streams with repairs forced on 64 streams (sel_mode 1, the redo mask) and on 65 (sel_mode 2, the
    repaired selection): both the oracle's, so both the same."""
    ins = _inputs(65)
    want = _oracle(oracle, ins)
    raw = np.stack([r for r, _, _ in ins])
    res = {}
    for nstr in (64, 65):
        with _rx(ins[:nstr], max_push=1 << 19, flags=lib.F_TEST_NOREGION) as rx:
            got = rx.run(raw[:nstr])
            st = rx.stats()
        assert st["repairs"] > 0, (nstr, st)
        _check(got, want[:nstr], ins[:nstr])
        res[nstr] = sorted((b.stream,) + _rec(b) for b in got)
    assert res[64] == [r for r in res[65] if r[0] < 64]


def _handle_bytes(nstr, max_push, push, sdrclk=500, sample_bytes=4):
    """create_impl's big allocations (vdl2gpu.hip): the three plane sets, the three item lists (80 bytes an item) -- and the two
    input buffers a host push of ``push`` samples allocates"""
    jmax = 21 * max_push // sdrclk + 2
    cap = (49152 + jmax + 64 + 15) // 16 * 16
    tiles_max = (49152 + min(jmax, 48 * 84000)) // 1024 + 2
    priv = min(131072, max(32768, (64 * tiles_max + 4095) // 4096 * 4096))
    item_cap = priv + max(priv // 2, 32768)
    return cap, 3 * nstr * 8 * cap * 8, 3 * nstr * 8 * item_cap * 80, 2 * nstr * push * sample_bytes


@pytest.mark.timeout(300)
def test_planes_beyond_4_gib_of_the_first(built, oracle):
    """max_push = 1 << 25 on 64 streams: a stream's planes are 93 MB, and the planes of slots 369..511 (streams 46..63) start
    more than 4 GiB behind the handle's first plane.  Every kernel must address them with 64-bit offsets; only 1 Mi samples are
    pushed.  The handle takes 41 GB (38 GiB) of device memory: 35.3 GB of planes and item lists (estimated below from
    create_impl's formulas), the rest candidate tables, clusters, burst descriptors and records."""
    import torch
    ins = _inputs(64)
    want = _oracle(oracle, ins)
    raw = np.stack([r for r, _, _ in ins])
    n = raw.shape[1] // 2
    max_push = 1 << 25
    cap, planes, items, inbuf = _handle_bytes(64, max_push, n)
    assert 8 * cap * 8 < 1 << 32 < (64 * 8 - 1) * cap * 8
    assert -(-(1 << 32) // (cap * 8)) == 369          # the first slot whose plane starts at 4 GiB or more
    est = planes + items + inbuf
    assert est < 40e9, est
    torch.cuda.init()
    free0, total = torch.cuda.mem_get_info(0)
    assert free0 > est + 4e9, (free0, est)
    with _rx(ins, max_push=max_push) as rx:
        free1, _ = torch.cuda.mem_get_info(0)
        got = rx.run(raw)
        free2, _ = torch.cuda.mem_get_info(0)
        st = rx.stats()
    print(f"\nhandle of 64 streams, max_push {max_push}: estimated planes {planes / 1e9:.2f} GB + item lists {items / 1e9:.2f} GB "
          f"+ input buffers {inbuf / 1e9:.2f} GB = {est / 1e9:.2f} GB; measured create {(free0 - free1) / 1e9:.2f} GB, "
          f"after the push {(free0 - free2) / 1e9:.2f} GB")
    # planes and item lists are most of what create_impl allocates (measured: 1.17 times as much in all)
    assert planes + items < free0 - free1 < 1.3 * (planes + items), (free0, free1, planes + items)
    _check(got, want, ins)
    assert st["serial_redos"] == 0 and st["overflowed"] == 0, st
