"""Rows for the row-level comparison of the block kernel's RS decoder with rs() (rs.c:81-291): tests/test_gpu_rs.py runs them on the
device, tests/test_rs_cases.py holds what each set claims to contain against the oracle alone.

The decoder is linear: what it does to a row depends on the error pattern, not on the codeword under it, so a handful of codewords
from synth.rs_parity serve every set.  Every set is built once per process, and so is the oracle's answer to it."""
import ctypes as C
import functools

import numpy as np

from oracle import oracle as O
from vdlm2dec_amd import synth

REGIME = {0: [], 2: [253, 254], 4: [251, 252, 253, 254]}      # set_eras(), vdlm2.c:63-82
NLBYTES = (0, 1, 2, 3, 30, 31, 67, 68, 249)


class Case:
    """rows (n, 255) uint8, eras (n, 6) int32, ne (n,) int32; clean: the codeword under each row, has_clean: whether there is one"""

    def __init__(self, parts):
        self.rows = np.ascontiguousarray(np.concatenate([p[0] for p in parts]), np.uint8)
        self.eras = np.ascontiguousarray(np.concatenate([p[1] for p in parts]), np.int32)
        self.ne = np.ascontiguousarray(np.concatenate([p[2] for p in parts]), np.int32)
        self.clean = np.concatenate([p[3] if p[3] is not None else np.zeros_like(p[0]) for p in parts])
        self.has_clean = np.concatenate([np.full(len(p[0]), p[3] is not None) for p in parts])
        self.n = len(self.rows)
        assert self.eras.shape == (self.n, 6) and self.ne.shape == (self.n,) and self.rows.shape == (self.n, 255)
        self._want = None

    def in_capacity(self) -> np.ndarray:
        """2 * errors + erasures <= 6, an error being a wrong byte at a position that is not erased"""
        wrong = self.rows != self.clean
        erased = np.zeros((self.n, 255), bool)
        for k in range(6):
            m = self.ne > k
            erased[np.nonzero(m)[0], self.eras[m, k]] = True
        return self.has_clean & (2 * (wrong & ~erased).sum(axis=1) + self.ne <= 6)

    def want(self):
        """(ret, rows, eras) as the oracle's rs() leaves them"""
        if self._want is None:
            self._want = oracle_rs(self.rows, self.eras, self.ne)
        return self._want


def oracle_rs(rows, eras, ne):
    fn = C.cast(O.lib().vo_rs_decode, C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int))
    rows, eras = rows.copy(), eras.copy()
    ret = np.zeros(len(rows), np.int32)
    rp, ep = rows.ctypes.data, eras.ctypes.data
    for i, k in enumerate(ne.tolist()):
        ret[i] = fn(rp + 255 * i, ep + 24 * i, k)
    return ret, rows, eras


def same(got, want):
    """bit for bit what the issue of a row is: the return value, the 255 bytes, and the root positions of a success"""
    ret = want[0]
    assert np.array_equal(got[0], ret), np.nonzero(got[0] != ret)[0][:10]
    bad = np.nonzero((got[1] != want[1]).any(axis=1))[0]
    assert bad.size == 0, (bad[:10], ret[bad[:10]])
    mask = np.arange(6)[None, :] < ret[:, None]
    assert np.array_equal(got[2][mask], want[2][mask])


@functools.lru_cache(maxsize=None)
def codewords(k: int = 16) -> np.ndarray:
    rng = np.random.default_rng(2718)
    cw = np.zeros((k, 255), np.uint8)
    cw[:, :249] = rng.integers(0, 256, (k, 249), dtype=np.uint8)
    for i in range(k):
        cw[i, 249:] = synth.rs_parity(cw[i, :249].tolist())
    return cw


def _eras_of(n, positions):
    e = np.zeros((n, 6), np.int32)
    e[:, :len(positions)] = positions
    return e, np.full(n, len(positions), np.int32)


def _distinct(rng, n, k):
    """k distinct positions of 0..254 per row"""
    return np.argsort(rng.random((n, 255)), axis=1)[:, :k].astype(np.int64)


def _hit(rows, pos, mag):
    rows[np.arange(len(rows))[:, None], pos] ^= mag.astype(np.uint8)


def _fixed_regime(rng, n, regime, nerr_lo, nerr_hi):
    """codewords with nerr_lo..nerr_hi errors outside the regime's erasures; an erased byte is garbage half of the time"""
    cw = codewords()
    clean = cw[rng.integers(0, len(cw), n)]
    rows = clean.copy()
    span = 255 - len(REGIME[regime])      # the regimes erase the row's last bytes
    pos = np.argsort(rng.random((n, span)), axis=1)[:, :nerr_hi]
    mag = rng.integers(1, 256, (n, nerr_hi))
    mag[np.arange(nerr_hi)[None, :] >= rng.integers(nerr_lo, nerr_hi + 1, n)[:, None]] = 0
    _hit(rows, pos, mag)
    for p in REGIME[regime]:
        rows[:, p] ^= (rng.integers(0, 256, n) * rng.integers(0, 2, n)).astype(np.uint8)
    return (rows,) + _eras_of(n, REGIME[regime]) + (clean,)


@functools.lru_cache(maxsize=None)
def every_position() -> Case:
    cw = codewords()
    parts = []
    for regime, er in REGIME.items():
        for mag in (0x01, 0x80, 0xff):
            clean = np.repeat(cw[regime % len(cw)][None, :], 255, axis=0)
            rows = clean.copy()
            rows[np.arange(255), np.arange(255)] ^= mag
            parts.append((rows,) + _eras_of(255, er) + (clean,))
        parts.append((cw[:4].copy(),) + _eras_of(4, er) + (cw[:4],))       # nothing wrong at all, erased or not
    return Case(parts)


@functools.lru_cache(maxsize=None)
def every_pair() -> Case:
    rng = np.random.default_rng(31)
    i, j = np.triu_indices(255, 1)
    n = len(i)
    assert n == 32385
    clean = codewords()[rng.integers(0, len(codewords()), n)]
    rows = clean.copy()
    _hit(rows, np.stack([i, j], axis=1), rng.integers(1, 256, (n, 2)))
    return Case([(rows,) + _eras_of(n, []) + (clean,)])


FORCED_TRIPLES = [(0, 1, 2), (252, 253, 254), (63, 64, 65), (127, 128, 191), (249, 250, 251), (249, 251, 254), (250, 252, 253)]


def last_row(rng, nlbyte: int, with_error: bool):
    """the last row of a burst as the receiver leaves it (synth.received_rows: what is not transmitted is zero), its erasures
    (set_eras) and the codeword the transmitter computed.  nlbyte == 249 takes a byte count no whole-byte payload has: the row is
    then a full one with all its parity, which is what any row but the last is"""
    if nlbyte == 249:
        payload = bytes(rng.integers(0, 256, 249 + 5, dtype=np.uint8).tolist())
        r = 0
    else:
        payload = bytes(rng.integers(0, 256, 249 + nlbyte, dtype=np.uint8).tolist())
        r = 1
    nbrow, nl, data = synth.received_rows(payload)
    assert nbrow == 2 and (r == 0 or nl == nlbyte)
    row = np.frombuffer(data, np.uint8).reshape(8, 255)[r].copy()
    clean = row.copy()
    clean[249:] = synth.rs_parity(clean[:249].tolist())
    if with_error:
        row[int(rng.integers(0, max(nlbyte, 1)))] ^= int(rng.integers(1, 256))
    regime = 4 if nlbyte <= 30 else (2 if nlbyte <= 67 else 0)
    return (row[None, :],) + _eras_of(1, REGIME[regime]) + (clean[None, :],)


@functools.lru_cache(maxsize=None)
def triples_and_edges() -> Case:
    rng = np.random.default_rng(32)
    cw = codewords()
    n = 20000
    clean = cw[rng.integers(0, len(cw), n)]
    rows = clean.copy()
    _hit(rows, _distinct(rng, n, 3), rng.integers(1, 256, (n, 3)))
    parts = [(rows,) + _eras_of(n, []) + (clean,)]
    m = len(FORCED_TRIPLES)
    clean = cw[:m]
    rows = clean.copy()
    _hit(rows, np.array(FORCED_TRIPLES), rng.integers(1, 256, (m, 3)))
    parts.append((rows,) + _eras_of(m, []) + (clean,))
    parts.append(_fixed_regime(rng, 3000, 2, 2, 2))     # in capacity: 2 * 2 + 2
    parts.append(_fixed_regime(rng, 3000, 2, 3, 3))     # beyond it
    parts.append(_fixed_regime(rng, 3000, 4, 1, 1))     # 2 * 1 + 4
    parts.append(_fixed_regime(rng, 3000, 4, 2, 2))
    for nlbyte in NLBYTES:
        for _ in range(8):
            parts.append(last_row(rng, nlbyte, False))
            parts.append(last_row(rng, nlbyte, True))
    return Case(parts)


@functools.lru_cache(maxsize=None)
def arbitrary_erasures() -> Case:
    """0..4 erasures anywhere in the row (the soft row rule's), and a smaller lot of 5 and 6 (rs() takes up to NROOTS); 0..4 errors
    elsewhere; an erased byte is garbage half of the time; eras[] behind the erasures holds garbage that nothing may read"""
    rng = np.random.default_rng(33)
    cw = codewords()
    parts = []
    for n, ne_hi, nerr_hi in ((20000, 4, 4), (3000, 6, 2)):
        ne = rng.integers(0 if ne_hi == 4 else 5, ne_hi + 1, n).astype(np.int32)
        perm = _distinct(rng, n, 12)
        clean = cw[rng.integers(0, len(cw), n)]
        rows = clean.copy()
        used = np.arange(6)[None, :] < ne[:, None]
        mag = rng.integers(0, 256, (n, 6)) * rng.integers(0, 2, (n, 6)) * used
        _hit(rows, perm[:, :6], mag)
        emag = rng.integers(1, 256, (n, nerr_hi))
        emag[np.arange(nerr_hi)[None, :] >= rng.integers(0, nerr_hi + 1, n)[:, None]] = 0
        _hit(rows, perm[:, 6:6 + nerr_hi], emag)
        eras = np.where(used, perm[:, :6], rng.integers(-2**31, 2**31, (n, 6))).astype(np.int32)
        parts.append((rows, eras, ne, clean))
    return Case(parts)


N_NOISE = 20000


@functools.lru_cache(maxsize=None)
def beyond_capacity(regime: int) -> Case:
    """N_NOISE rows of noise, then as many codewords with 3..5 errors"""
    rng = np.random.default_rng(40 + regime)
    noise = rng.integers(0, 256, (N_NOISE, 255), dtype=np.uint8)
    return Case([(noise,) + _eras_of(N_NOISE, REGIME[regime]) + (None,), _fixed_regime(rng, N_NOISE, regime, 3, 5)])


def beyond_classes(regime: int) -> dict:
    """how many rows of beyond_capacity(regime) the oracle puts in each class the comparison has to contain"""
    ret, rows, _ = beyond_capacity(regime).want()
    changed = (rows != beyond_capacity(regime).rows).any(axis=1)
    return {"fail": int((ret == -1).sum()), "miscorrected_noise": int(((ret[:N_NOISE] >= 0) & changed[:N_NOISE]).sum()),
            "ret4": int((ret == 4).sum()), "ret5": int((ret == 5).sum()), "fail_changed": int(((ret == -1) & changed).sum())}


GARBAGE = [-5, 9999, 0x7fffffff, -0x80000000, 255, 254]


@functools.lru_cache(maxsize=None)
def degenerate() -> Case:
    cw = codewords()
    z = np.zeros((1, 255), np.uint8)
    first, last = z.copy(), z.copy()
    first[0, 0], last[0, 254] = 0x5a, 0x01
    parts = []
    for er in REGIME.values():
        for rows, clean in ((z, z), (z + 0xff, z + 0xff), (first, z), (last, z)):
            parts.append((rows.astype(np.uint8),) + _eras_of(1, er) + (clean.astype(np.uint8),))
    parts.append((cw[:1].copy(), np.array([GARBAGE], np.int32), np.zeros(1, np.int32), cw[:1]))
    parts.append((cw[1:2].copy(), np.array([[7, 200] + GARBAGE[:4]], np.int32), np.full(1, 2, np.int32), cw[1:2]))
    return Case(parts)
