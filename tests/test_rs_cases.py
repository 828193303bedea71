"""What the row sets of tests/rs_cases.py claim to contain, held against the oracle alone (no GPU): a comparison on the device proves
something only if the classes of rows it is about are there."""
import numpy as np
import pytest

import rs_cases as R


def test_codewords_are_codewords(oracle):
    cw = R.codewords()
    ret, rows, _ = R.oracle_rs(cw, np.zeros((len(cw), 6), np.int32), np.zeros(len(cw), np.int32))
    assert not ret.any() and np.array_equal(rows, cw)


@pytest.mark.parametrize("name", ["every_position", "every_pair", "triples_and_edges", "arbitrary_erasures", "degenerate"])
def test_rows_within_capacity_are_restored(oracle, name):
    """2 * errors + erasures <= 6: rs() gives the codeword back, the roots it names are the erasures and the errors"""
    c = getattr(R, name)()
    ret, rows, eras = c.want()
    cap = c.in_capacity()
    assert np.array_equal(rows[cap], c.clean[cap]) and (ret[cap] >= 0).all()
    assert cap.sum() >= {"every_position": 2295, "every_pair": 32385, "triples_and_edges": 26000, "arbitrary_erasures": 5000,
                         "degenerate": 14}[name]
    if name in ("every_position", "every_pair"):
        assert cap.all()
    else:
        assert not cap.all() or name == "degenerate"      # and rows beyond it


def test_every_position_meets_erased_bytes_right_and_wrong(oracle):
    c = R.every_position()
    ret = c.want()[0]
    wrong = (c.rows != c.clean).sum(axis=1)
    assert set(ret[(c.ne == 0) & (wrong == 1)]) == {1} and set(ret[wrong == 0]) == {0}
    assert set(ret[(c.ne == 2) & (wrong == 1)]) == {2, 3}     # the error on an erased byte, and beside two erased bytes that are right
    assert set(ret[(c.ne == 4) & (wrong == 1)]) == {4, 5}


def test_last_row_shapes(oracle):
    """nlbyte <= 2: no parity was transmitted, four erasures stand over six missing bytes -- rs() cannot restore that row"""
    rng = np.random.default_rng(5)
    for nlbyte in R.NLBYTES:
        c = R.Case([R.last_row(rng, nlbyte, e) for e in (False, True)])
        assert list(c.ne) == [4 if nlbyte <= 30 else (2 if nlbyte <= 67 else 0)] * 2
        assert not c.rows[0, max(nlbyte, 0):249].any() or nlbyte == 249
        ret, rows, _ = c.want()
        if nlbyte > 2:
            assert c.in_capacity().all() and np.array_equal(rows, c.clean)
        elif c.clean[0, 249] and c.clean[0, 250]:
            assert not c.in_capacity().any()


@pytest.mark.parametrize("regime", [0, 2, 4])
def test_beyond_capacity_holds_every_class(oracle, regime):
    k = R.beyond_classes(regime)
    assert k["fail"] > 0 and k["miscorrected_noise"] > 0, k
    if regime == 0:
        assert k["ret4"] > 0, k
    if regime == 2:
        assert k["ret5"] > 0, k
