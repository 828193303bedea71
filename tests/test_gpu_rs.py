"""The block kernel's RS(255,249) decoder row by row (vdl2gpu_debug_rs -> k4_rs_row) == rs() (rs.c:81-291) as the oracle restates
it (vo_rs_decode, pinned to the reference in test_oracle_vs_ref.py): the return value, all 255 bytes and the root positions of a
success, bit for bit -- for rows rs() repairs, miscorrects and gives up on alike.  The frame-level tests see none of the latter two:
such a burst yields no frame on either side.  tests/test_rs_cases.py holds the row sets' own claims against the oracle."""
import ctypes as C

import numpy as np
import pytest

import rs_cases as R
import scenarios as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rx(built):
    from vdlm2dec_amd.demod import Receiver, plan_channels
    with Receiver(2_000_000, plan_channels(S.FC, [-50000]), fmt="cu8", max_push=4096) as r:
        yield r


def _run(rx, c):
    got = rx.debug_rs(c.rows, c.eras, c.ne)
    R.same(got, c.want())
    return got


def test_every_position(rx, oracle):
    """one error at each of the 255 positions, 0x01 / 0x80 / 0xff, under 0, 2 and 4 erasures: erased positions included, erased bytes
    that are right (zero Forney numerator) in every row with erasures"""
    c = R.every_position()
    assert c.in_capacity().all() and np.array_equal(c.want()[1], c.clean) and c.n == 9 * 255 + 12
    _run(rx, c)


def test_every_pair(rx, oracle):
    """all 32 385 pairs of positions: roots in one and in two Chien groups, adjacent, (0, 254)"""
    c = R.every_pair()
    assert c.n == 32385 and np.array_equal(c.want()[1], c.clean) and (c.want()[0] == 2).all()
    _run(rx, c)


def test_triples_and_capacity_edges(rx, oracle):
    c = R.triples_and_edges()
    cap = c.in_capacity()
    assert np.array_equal(c.want()[1][cap], c.clean[cap]) and 26000 <= cap.sum() < c.n
    _run(rx, c)


def test_arbitrary_erasures(rx, oracle):
    c = R.arbitrary_erasures()
    cap = c.in_capacity()
    assert np.array_equal(c.want()[1][cap], c.clean[cap]) and 5000 <= cap.sum() < c.n
    for k in range(7):
        assert (c.ne == k).sum() >= 1000
    _run(rx, c)


@pytest.mark.parametrize("regime", [0, 2, 4])
def test_beyond_capacity(rx, oracle, regime):
    """noise and 3..5 errors: -1, miscorrections (16 % of noise rows without erasures, 98 % with four), a return of 4 without
    erasures and of 5 with two -- classified by the oracle's own result before the device is asked"""
    k = R.beyond_classes(regime)
    print(regime, k)
    assert k["fail"] > 0 and k["miscorrected_noise"] > 0
    assert regime != 0 or k["ret4"] > 0
    assert regime != 2 or k["ret5"] > 0
    _run(rx, R.beyond_capacity(regime))


def test_degenerate_rows(rx, oracle):
    c = R.degenerate()
    got = _run(rx, c)
    z = c.want()[0] == 0
    assert z.sum() >= 8 and np.array_equal(got[2][z], c.eras[z])       # zero syndromes: eras untouched, garbage and all
    ret, rows, eras = rx.debug_rs(np.zeros((0, 255), np.uint8), np.zeros((0, 6), np.int32), np.zeros(0, np.int32))
    assert ret.size == 0 and rows.size == 0


def test_einval(rx):
    from vdlm2dec_amd import lib
    L = rx.L
    rows, eras, ne, ret = (C.c_uint8 * 255)(), (C.c_int * 6)(), (C.c_int * 1)(), (C.c_int * 1)()
    p = [C.cast(a, C.c_void_p) for a in (rows, eras, ne, ret)]
    assert L.vdl2gpu_debug_rs(rx.h, *p, 1) == 0
    assert L.vdl2gpu_debug_rs(None, *p, 1) == -1
    assert L.vdl2gpu_debug_rs(rx.h, None, None, None, None, 0) == 0
    for k in range(4):
        q = list(p)
        q[k] = None
        assert L.vdl2gpu_debug_rs(rx.h, *q, 1) == -1
    for bad in (-1, 7):
        ne[0] = bad
        assert L.vdl2gpu_debug_rs(rx.h, *p, 1) == -1
    ne[0] = 2
    for bad in (-1, 255):
        eras[1] = bad
        assert L.vdl2gpu_debug_rs(rx.h, *p, 1) == -1
    eras[1], eras[2] = 254, 255          # behind the erasures: not looked at
    assert L.vdl2gpu_debug_rs(rx.h, *p, 1) == 0 and ret[0] == 0
    with pytest.raises(lib.Vdl2GpuError):
        rx.debug_rs(np.zeros((1, 255), np.uint8), np.zeros((1, 6), np.int32), np.array([9], np.int32))
