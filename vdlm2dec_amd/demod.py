"""Host-side mirror of the reference's receive interface, over the C ABI.

The reference starts one ``rcv_thread(thread_param_t*)`` per channel (main.c:228-231)
and each hands ``msgblk_t`` bursts to ``decodeVdlm2`` (d8psk.c:201).  ``Receiver`` keeps
those names and meanings: it is configured with the same ``(chn, Fr, Fo)`` triples and
``SDRINRATE``; ``push()`` plays the producer's Bar1/Bar2 hand-off of one sample block
(rtl.c:283-294) for *all* channels; ``poll()`` yields ``Burst`` objects carrying exactly the
``msgblk_t`` fields.  All DSP happens in libvdl2gpu.so on the GPU.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np

from . import lib as _lib

STEPRATE = 25000           # vdlm2.h:33
RTLINBUFSZ = 16 * 4096     # vdlm2.h:35 (bytes per RTL hand-off = 32768 complex samples)


@dataclass(frozen=True)
class ThreadParam:
    """thread_param_t, vdlm2.h:49-52."""
    chn: int
    Fr: int
    Fo: int


@dataclass(frozen=True)
class Level:
    """vdl2gpu_level_t: the burst's signal and noise level (Receiver(levels=True); definitions in include/vdl2gpu.h)."""
    sig_dbfs: float
    noise_dbfs: float          # NaN with noise_blocks == 0
    sig_power: float
    noise_power: float         # NaN with noise_blocks == 0
    sym_first_dec: int
    nsym: int
    subphase: int
    noise_blocks: int

    @classmethod
    def from_c(cls, v) -> "Level":
        return cls(v.sig_dbfs, v.noise_dbfs, v.sig_power, v.noise_power, v.sym_first_dec, v.nsym, v.subphase, v.noise_blocks)


@dataclass(frozen=True)
class Carrier:
    """vdl2gpu_carrier_t: the burst's true carrier offset and phase-error spread (Receiver(carrier=True); definitions in include/vdl2gpu.h)."""
    nsym: int
    sum_e: int
    sum_e2: int
    dphi: float                # rad per symbol beyond the data
    freq_hz: float             # positive: the carrier lies above the channel centre as mixed
    ppm: float
    rms_rad: float             # near pi/8: not to be trusted

    @classmethod
    def from_c(cls, v) -> "Carrier":
        return cls(v.nsym, v.sum_e, v.sum_e2, v.dphi, v.freq_hz, v.ppm, v.rms_rad)


@dataclass(frozen=True)
class BlockReport:
    """vdl2gpu_blockrep_t: what the block path made of a burst (Receiver(frames=True, block_report=True), decode_blocks(report=True);
    definitions in include/vdl2gpu.h)."""
    row_roots: Tuple[int, ...]     # per row: rs()'s return value for the received row (-1: it failed)
    row_how: Tuple[int, ...]       # per row: lib.ROW_NONE / CLEAN / REF / SOFT2 / SOFT4 / FAIL / FEEDBACK
    row_changed: Tuple[int, ...]   # per row: transmitted bytes the decode changed
    bytes_changed: int
    rows_failed: int
    rows_rescued: int
    stuffed: int                   # zeros the un-stuffer dropped
    nbytes: int                    # whole un-stuffed bytes
    flag_at: int                   # un-stuffed byte that completes the first flag, -1: never
    cand: int                      # calls of check_frame(): cand == too_short + bad_fcs + frames
    too_short: int                 # "error too short"
    bad_fcs: int                   # "error crc"
    frames: int
    status: int                    # 1: header out of range, nothing ran

    @classmethod
    def from_c(cls, v) -> "BlockReport":
        return cls(tuple(v.row_roots), tuple(v.row_how), tuple(v.row_changed), v.bytes_changed, v.rows_failed, v.rows_rescued,
                   v.stuffed, v.nbytes, v.flag_at, v.cand, v.too_short, v.bad_fcs, v.frames, v.status)


@dataclass(frozen=True)
class SymClock:
    """vdl2gpu_symclk_t: the burst's symbol timing, clock drift and fine arrival time (Receiver(symclk=True); definitions in
    include/vdl2gpu.h)."""
    sym_first_dec: int
    nsym: int
    nseg: int
    toa_sample: float          # input-sample time of the centre of the first symbol behind the unique word
    tau0: float                # 84 kS/s samples; positive: the symbol centres lie later than the grid sym_first_dec + 8 k
    clock_ppm: float           # positive: the transmitter's symbols come faster than 10 500 a second; NaN with nseg == 1
    tau_rms: float             # NaN with nseg == 1
    e: np.ndarray              # float32 (22, 8): the sums, zero from segment nseg on
    tau_s: Tuple[float, ...]   # the nseg segments' unwrapped timing, derived from e as the library derives it

    @classmethod
    def from_c(cls, v, sdrinrate: int) -> "SymClock":
        e = np.frombuffer(bytes(v.e), np.float32).reshape(_lib.SYMCLK_SEGS, 8).copy()
        tau = ()
        if v.nsym > 0:
            tau = symclk_from_sums(v.sym_first_dec, v.nsym, e, sdrinrate).tau_s
        return cls(v.sym_first_dec, v.nsym, v.nseg, v.toa_sample, v.tau0, v.clock_ppm, v.tau_rms, e, tau)


def symclk_from_sums(sym_first_dec: int, nsym: int, e, sdrinrate: int) -> SymClock:
    """vdl2gpu_symclk_from_sums: the derived values of a symbol-clock record, as the library computes them (no GPU needed).
    e: the sums of at least the first ceil(nsym / 256) segments, (segments, 8)."""
    nseg = (nsym + _lib.SYMCLK_SEG - 1) // _lib.SYMCLK_SEG
    ee = np.ascontiguousarray(np.asarray(e, np.float32).reshape(-1, 8)[:max(nseg, 0)])
    if nsym > 0 and ee.shape[0] < nseg:
        raise ValueError("e holds fewer segments than nsym needs")
    c = _lib.SymClkT()
    tau = (C.c_double * _lib.SYMCLK_SEGS)()
    rc = _lib.load().vdl2gpu_symclk_from_sums(sym_first_dec, nsym, ee.ctypes.data_as(C.POINTER(C.c_float)), sdrinrate, C.byref(c), tau)
    if rc < 0:
        raise _lib.Vdl2GpuError("vdl2gpu_symclk_from_sums failed")
    return SymClock(c.sym_first_dec, c.nsym, c.nseg, c.toa_sample, c.tau0, c.clock_ppm, c.tau_rms,
                    np.frombuffer(bytes(c.e), np.float32).reshape(_lib.SYMCLK_SEGS, 8).copy(), tuple(tau[:c.nseg]))


@dataclass(frozen=True)
class Tracked:
    """vdl2gpu_trk_t: the burst's rows sliced with a sampling instant tracked in segments of 256 symbols (Receiver(tracked=True);
    definitions in include/vdl2gpu.h)."""
    data: np.ndarray           # uint8 (8, 255), laid out as the record's data[]
    d_first: int               # quarter samples: the first segment's offset ...
    d_last: int                # ... the last segment's ...
    d_min: int                 # ... and the least and greatest of the burst
    d_max: int
    nseg: int
    raw: bytes                 # the 2048 bytes of the entry

    @classmethod
    def from_c(cls, v) -> "Tracked":
        return cls(_rows(v.data), v.d_first, v.d_last, v.d_min, v.d_max, v.nseg, bytes(v))


def carrier_from_sums(df: float, Fr: int, nsym: int, sum_e: int, sum_e2: int) -> Carrier:
    """vdl2gpu_carrier_from_sums: the derived values of a carrier record, as the library computes them (no GPU needed)."""
    c = _lib.CarrierT()
    rc = _lib.load().vdl2gpu_carrier_from_sums(df, Fr, nsym, sum_e, sum_e2, C.byref(c))
    if rc < 0:
        raise _lib.Vdl2GpuError("vdl2gpu_carrier_from_sums failed")
    return Carrier.from_c(c)


@dataclass
class Burst:
    """The msgblk_t fields the DSP fills (vdlm2.h:39-47) plus stream-time stamps."""
    stream: int
    chn: int
    Fr: int
    nbrow: int
    nlbyte: int
    df: float
    ppm: float
    trig_dec: int
    end_dec: int
    trig_sample: int
    end_sample: int
    data: bytes            # 8 rows x 255 bytes, row-major
    level: Optional[Level] = None   # Receiver(levels=True) only; not part of key()
    soft: Optional[np.ndarray] = None   # Receiver(soft_rs=True) only: uint8 (8, 255) byte reliabilities; not part of key()
    carrier: Optional[Carrier] = None   # Receiver(carrier=True) only; not part of key()
    report: Optional[BlockReport] = None   # Receiver(frames=True, block_report=True) only; not part of key()
    fb: Optional[np.ndarray] = None   # Receiver(feedback=True) only: uint8 (8, 255), the rows sliced with decision feedback; not part of key()
    clock: Optional[SymClock] = None   # Receiver(symclk=True) only; not part of key()
    trk: Optional["Tracked"] = None   # Receiver(tracked=True) only: the rows sliced with a tracked sampling instant; not part of key()

    def key(self):
        return (self.stream, self.chn, self.nbrow, self.nlbyte, self.data)


def _rows(v) -> np.ndarray:
    return np.frombuffer(bytes(v), np.uint8).reshape(8, 255).copy()


# The side columns of a burst, in the order of the collectors' arguments: Receiver keyword (and attribute), flag, record type, and the
# Burst field's value of a record.  (The Burst fields themselves follow `data` in this order.)
_COLUMNS = (
    ("levels", _lib.F_LEVELS, _lib.LevelT, Level.from_c),
    ("soft_rs", _lib.F_SOFT_RS, _lib.SoftT, lambda v: _rows(v.rel)),
    ("carrier", _lib.F_CARRIER, _lib.CarrierT, Carrier.from_c),
    ("block_report", _lib.F_BLOCK_REPORT, _lib.BlockRepT, BlockReport.from_c),
    ("feedback", _lib.F_FEEDBACK, _lib.FbT, lambda v: _rows(v.data)),
    ("symclk", _lib.F_SYMCLK, _lib.SymClkT, None),     # (SymClock.from_c wants the receiver's rate: _collect)
)
# ... and the columns behind the symbol clock, in the order of vdl2gpu_poll_tracked's arguments (_COLUMNS is what vdl2gpu_poll_symclk takes)
_ALL_COLUMNS = _COLUMNS + (
    ("tracked", _lib.F_TRACKED, _lib.TrkT, Tracked.from_c),
)


def plan_channels(fc: int, offsets: Sequence[int]) -> List[ThreadParam]:
    """thread_param_t list the way rtl.c:245-247 fills it: Fo = Fr - Fc."""
    return [ThreadParam(chn=i, Fr=fc + fo, Fo=fo) for i, fo in enumerate(offsets)]


class Receiver:
    def __init__(self, sdrinrate: int, channels: Sequence[ThreadParam] | Sequence[Sequence[ThreadParam]],
                 fmt: str = "cu8", max_push: int = 1 << 22, device: int = 0, sdrclk: int = 0,
                 max_bursts: int = 0, keep_dec: bool = False, serial: bool = False, full_scan: bool = False,
                 frames: bool = False, rtl_quirk: bool = False, flags: int = 0, testhooks: bool = False,
                 levels: bool = False, soft_rs: bool = False, exact_fo: bool = False, carrier: bool = False,
                 block_report: bool = False, feedback: bool = False, all_frames: bool = False, raw_flags: bool = False,
                 symclk: bool = False, tracked: bool = False):
        # tracked: VDL2GPU_F_TRACKED, every burst's rows sliced a second time with a tracked sampling instant (Burst.trk); with frames=True
        # the block path makes a second attempt with them for a burst of which the first passes no candidate
        # symclk: VDL2GPU_F_SYMCLK, every burst's symbol timing, clock drift and fine arrival time (Burst.clock)
        # raw_flags: VDL2GPU_F_RAW_FLAGS (needs all_frames=True), a stuffed data byte 0x7e is told from a flag, so frames that hold one arrive
        # all_frames: VDL2GPU_F_ALL_FRAMES (needs frames=True), the block path hands on every frame of a burst, not only the first
        # feedback: VDL2GPU_F_FEEDBACK, every burst's rows sliced a second time with decision feedback (Burst.fb); with frames=True the
        # block path takes a row the reference cannot decode from them
        # block_report: VDL2GPU_F_BLOCK_REPORT (needs frames=True), what the block path made of every burst (Burst.report)
        # carrier: VDL2GPU_F_CARRIER, every burst's carrier offset and phase-error spread (Burst.carrier)
        # exact_fo: VDL2GPU_F_EXACT_FO, channel offsets off the 25 kHz grid with a phase-continuous oscillator (include/vdl2gpu.h)
        # testhooks: load libvdl2gpu_test.so, the build that honours F_TEST_NOREGION / VDL2GPU_PRIM_DROP / VDL2GPU_SPLIT_SAMPLES
        if raw_flags and not all_frames:
            raise ValueError("raw_flags=True needs all_frames=True")
        self.L = _lib.load(testhooks=testhooks or bool(flags & _lib.F_TEST_NOREGION))
        if channels and isinstance(channels[0], ThreadParam):
            channels = [list(channels)]
        self.nstreams = len(channels)
        self.nbch = len(channels[0])
        if any(len(c) != self.nbch for c in channels):
            raise ValueError("every stream needs the same number of channels")
        self.fmt = fmt
        self.rate = sdrinrate
        self.sample_bytes = _lib.SAMPLE_BYTES[fmt]
        self._chan = (_lib.ChanT * (self.nstreams * self.nbch))()
        for s, plan in enumerate(channels):
            for c, tp in enumerate(plan):
                self._chan[s * self.nbch + c] = _lib.ChanT(tp.chn, tp.Fr, tp.Fo)
        cfg = _lib.ConfigT()
        cfg.struct_size = C.sizeof(_lib.ConfigT)
        cfg.sdrinrate = sdrinrate
        cfg.sdrclk = sdrclk
        cfg.fmt = _lib.FMT[fmt]
        cfg.nbch = self.nbch
        cfg.nstreams = self.nstreams
        cfg.chan = self._chan
        cfg.max_push = max_push
        cfg.device = device
        cfg.max_bursts = max_bursts
        asked = dict(levels=levels, soft_rs=soft_rs, carrier=carrier, block_report=block_report, feedback=feedback, symclk=symclk, tracked=tracked)
        switches = [(keep_dec, _lib.F_KEEP_DEC), (serial, _lib.F_SERIAL), (full_scan, _lib.F_FULLSCAN), (frames, _lib.F_FRAMES),
                    (rtl_quirk, _lib.F_RTL_QUIRK), (exact_fo, _lib.F_EXACT_FO), (all_frames, _lib.F_ALL_FRAMES),
                    (raw_flags, _lib.F_RAW_FLAGS)] + [(asked[kw], flag) for kw, flag, _, _ in _ALL_COLUMNS]
        cfg.flags = flags | sum(flag for on, flag in switches if on)     # (one bit each)
        self.max_push = max_push
        for kw, flag, _, _ in _ALL_COLUMNS:     # self.levels, .soft_rs, .carrier, .block_report, .feedback, .symclk, .tracked: by keyword or by `flags`
            setattr(self, kw, bool(cfg.flags & flag))
        self.all_frames = bool(cfg.flags & _lib.F_ALL_FRAMES)
        self.raw_flags = bool(cfg.flags & _lib.F_RAW_FLAGS)
        self.h = C.c_void_p()
        rc = self.L.vdl2gpu_create(C.byref(cfg), C.byref(self.h))
        if rc != 0:
            self.h = None
            raise _lib.Vdl2GpuError(f"vdl2gpu_create failed: {self.L.vdl2gpu_strerror(rc).decode()}")

    # -------------------------------------------------------------------- data path
    def _check(self, rc: int):
        if rc < 0:
            msg = self.L.vdl2gpu_last_error(self.h).decode()
            raise _lib.Vdl2GpuError(f"{self.L.vdl2gpu_strerror(rc).decode()}: {msg}")
        return rc

    def push(self, raw: np.ndarray):
        """One hand-off of host samples. ``raw``: 1-D (single stream) or [nstreams, n] raw array."""
        a = np.ascontiguousarray(raw)
        if a.ndim == 1:
            a = a[None, :]
        if a.shape[0] != self.nstreams:
            raise ValueError("first dimension must be nstreams")
        nbytes = a.shape[1] * a.itemsize
        n = nbytes // self.sample_bytes
        self._check(self.L.vdl2gpu_push(self.h, a.ctypes.data_as(C.c_void_p), n, nbytes, _lib.MEM_HOST))
        return n

    # ------------------------------------------------------------------ ingest ring (include/vdl2gpu.h)
    def ring_init(self, slot_samples: int, nslots: int = 4):
        self._check(self.L.vdl2gpu_ring_init(self.h, slot_samples, nslots))
        self._ring_slot_samples = slot_samples

    def ring_acquire(self) -> np.ndarray:
        """The next slot of page-locked host memory as a [nstreams, slot_bytes] uint8 view: fill it in
        place (first ``nsamples * sample_bytes`` bytes of every row), then ``ring_commit(nsamples)``."""
        stride = C.c_size_t(0)
        p = self.L.vdl2gpu_ring_acquire(self.h, C.byref(stride))
        if not p:
            raise RuntimeError("vdl2gpu_ring_acquire: " + self.L.vdl2gpu_last_error(self.h).decode())
        buf = (C.c_uint8 * (stride.value * self.nstreams)).from_address(p)
        return np.frombuffer(buf, dtype=np.uint8).reshape(self.nstreams, stride.value)

    def ring_commit(self, nsamples: int):
        self._check(self.L.vdl2gpu_ring_commit(self.h, nsamples))

    def push_device(self, ptr: int, nsamples: int, stream_stride_bytes: int = 0):
        """Samples already resident in HBM (e.g. ``tensor.data_ptr()``)."""
        self._check(self.L.vdl2gpu_push(self.h, C.c_void_p(ptr), nsamples, stream_stride_bytes, _lib.MEM_DEVICE))

    def sync(self):
        self._check(self.L.vdl2gpu_sync(self.h))

    def _collect(self, ready: bool, max_bursts: int) -> List[Burst]:
        out: List[Burst] = []
        buf = (_lib.BurstT * max_bursts)()
        cols = [(typ * max_bursts)() if getattr(self, kw) else None for kw, _, typ, _ in _ALL_COLUMNS]
        # the widest collector serves every handle: a column the handle lacks is None, "not wanted" (include/vdl2gpu.h)
        fn = self.L.vdl2gpu_poll_tracked_ready if ready else self.L.vdl2gpu_poll_tracked
        while True:
            n = self._check(fn(self.h, buf, *cols, max_bursts))
            for i in range(n):
                b = buf[i]
                out.append(Burst(b.stream, b.chn, b.Fr, b.nbrow, b.nlbyte, b.df, b.ppm, b.trig_dec, b.end_dec,
                                 b.trig_sample, b.end_sample, bytes(b.data),
                                 *[None if v is None else (conv(v[i]) if conv else SymClock.from_c(v[i], self.rate))
                                   for v, (_, _, _, conv) in zip(cols, _ALL_COLUMNS)]))
            if n < max_bursts:
                return out

    def poll(self, max_bursts: int = 4096) -> List[Burst]:
        """Every burst of everything pushed so far (with its Level on a levels=True receiver)."""
        return self._collect(False, max_bursts)

    def poll_ready(self, max_bursts: int = 4096) -> List[Burst]:
        """Bursts of pushes the GPU has already finished; never waits."""
        return self._collect(True, max_bursts)

    def _poll_cols_raw(self, name: str, ready: bool, buf, cols, max_bursts: int) -> int:
        fn = getattr(self.L, name + ("_ready" if ready else ""))
        return self._check(fn(self.h, buf, *cols, max_bursts))

    # vdl2gpu_poll_levels / _soft / _carrier / _report / _feedback / _symclk (kv: a (lib.SymClkT * n) or None) (and their _ready forms) into caller-owned arrays: buf a
    # (lib.BurstT * n), lv / sv / cv / rv / fv a (lib.LevelT / SoftT / CarrierT / BlockRepT / FbT * n) or None
    def poll_levels_raw(self, buf, lv, max_bursts: int, ready: bool = False) -> int:
        return self._poll_cols_raw("vdl2gpu_poll_levels", ready, buf, (lv,), max_bursts)

    def poll_soft_raw(self, buf, lv, sv, max_bursts: int, ready: bool = False) -> int:
        return self._poll_cols_raw("vdl2gpu_poll_soft", ready, buf, (lv, sv), max_bursts)

    def poll_carrier_raw(self, buf, lv, sv, cv, max_bursts: int, ready: bool = False) -> int:
        return self._poll_cols_raw("vdl2gpu_poll_carrier", ready, buf, (lv, sv, cv), max_bursts)

    def poll_report_raw(self, buf, lv, sv, cv, rv, max_bursts: int, ready: bool = False) -> int:
        return self._poll_cols_raw("vdl2gpu_poll_report", ready, buf, (lv, sv, cv, rv), max_bursts)

    def poll_feedback_raw(self, buf, lv, sv, cv, rv, fv, max_bursts: int, ready: bool = False) -> int:
        return self._poll_cols_raw("vdl2gpu_poll_feedback", ready, buf, (lv, sv, cv, rv, fv), max_bursts)

    def poll_symclk_raw(self, buf, lv, sv, cv, rv, fv, kv, max_bursts: int, ready: bool = False) -> int:
        return self._poll_cols_raw("vdl2gpu_poll_symclk", ready, buf, (lv, sv, cv, rv, fv, kv), max_bursts)

    def poll_tracked_raw(self, buf, lv, sv, cv, rv, fv, kv, tv, max_bursts: int, ready: bool = False) -> int:
        return self._poll_cols_raw("vdl2gpu_poll_tracked", ready, buf, (lv, sv, cv, rv, fv, kv, tv), max_bursts)

    def poll_ready_raw(self, buf, max_bursts: int) -> int:
        """vdl2gpu_poll_ready: bursts of pushes that have already finished; never waits."""
        return self._check(self.L.vdl2gpu_poll_ready(self.h, buf, max_bursts))

    def poll_raw(self, buf, max_bursts: int) -> int:
        """vdl2gpu_poll into a caller-owned (lib.BurstT * max_bursts) array; no Python objects."""
        return self._check(self.L.vdl2gpu_poll(self.h, buf, max_bursts))

    def run(self, raw: np.ndarray, block: Optional[int] = None) -> List[Burst]:
        """Feed a whole recording in ``block``-sample hand-offs and return every burst."""
        a = np.ascontiguousarray(raw)
        if a.ndim == 1:
            a = a[None, :]
        per = self.sample_bytes // a.itemsize
        n = a.shape[1] // per
        block = block or self.max_push
        out: List[Burst] = []
        for s in range(0, n, block):
            e = min(n, s + block)
            self.push(a[:, s * per:e * per])
            out += self.poll()
        return out

    # ------------------------------------------------------------------ block path
    def decode_blocks(self, blocks: Sequence, max_frames: int = 0, soft=None, report: bool = False, fb=None, all_frames: bool = False,
                      raw_flags: bool = False, trk=None):
        """blk_thread for a batch (vdlm2.c:84-161): (index of the block, hdata) of every frame the
        reference would pass to out().  ``blocks``: Burst objects or (nbrow, nlbyte, data) tuples.
        ``soft``: one (8, 255) uint8 reliability map per block (Burst.soft): the soft row rule of include/vdl2gpu.h
        (vdl2gpu_decode_blocks_soft); None: the reference's block path.
        ``report``: return (frames, [BlockReport of every block]) (vdl2gpu_decode_blocks_report), on any handle.
        ``fb``: one (8, 255) uint8 array of decision-feedback rows per block (Burst.fb): a row the reference cannot decode is taken from
        them if it decodes there (vdl2gpu_decode_blocks_feedback), on any handle; None: not.
        ``all_frames``: every frame of a burst, by the rule of VDL2GPU_F_ALL_FRAMES (vdl2gpu_decode_blocks_ex with
        VDL2GPU_BLK_ALL_FRAMES), on any handle; the frames of a block come in stream order.
        ``raw_flags`` (with ``all_frames``): the rule of VDL2GPU_F_RAW_FLAGS, a stuffed data byte 0x7e is no flag (VDL2GPU_BLK_RAW_FLAGS).
        ``trk``: one (8, 255) uint8 array of timing-tracked rows per block (Burst.trk.data): a block of which the first attempt passes no
        candidate gets the second attempt of vdl2gpu_trk_t (vdl2gpu_decode_blocks_tracked), on any handle; None: not."""
        if raw_flags and not all_frames:
            raise ValueError("raw_flags=True needs all_frames=True")
        n = len(blocks)
        if n == 0:
            return ([], []) if report else []
        arr = (_lib.BurstT * n)()
        for i, b in enumerate(blocks):
            nbrow, nlbyte, data = (b.nbrow, b.nlbyte, b.data) if hasattr(b, "nbrow") else b
            arr[i].nbrow, arr[i].nlbyte = nbrow, nlbyte
            C.memmove(C.addressof(arr[i].data), bytes(data), min(len(data), 8 * 255))
            if hasattr(b, "chn"):
                arr[i].stream, arr[i].chn, arr[i].Fr = b.stream, b.chn, b.Fr
        cap = max_frames or (12 if all_frames else 4) * n
        out = (_lib.FrameT * cap)()
        dropped = C.c_int(0)
        sarr = None
        if soft is not None:
            if len(soft) != n:
                raise ValueError("one reliability map per block")
            sarr = (_lib.SoftT * n)()
            for i, m in enumerate(soft):
                m = np.ascontiguousarray(m, np.uint8).reshape(8, 255)
                C.memmove(C.addressof(sarr[i].rel), m.ctypes.data, 8 * 255)
        farr = None
        if fb is not None:
            if len(fb) != n:
                raise ValueError("one set of feedback rows per block")
            farr = (_lib.FbT * n)()
            for i, m in enumerate(fb):
                m = np.ascontiguousarray(m, np.uint8).reshape(8, 255)
                C.memmove(C.addressof(farr[i].data), m.ctypes.data, 8 * 255)
        tarr = None
        if trk is not None:
            if len(trk) != n:
                raise ValueError("one set of tracked rows per block")
            tarr = (_lib.TrkT * n)()
            for i, m in enumerate(trk):
                m = np.ascontiguousarray(m, np.uint8).reshape(8, 255)
                C.memmove(C.addressof(tarr[i].data), m.ctypes.data, 8 * 255)
        rarr = (_lib.BlockRepT * n)() if report else None
        # (soft NULL: hard mode; rep NULL: exactly vdl2gpu_decode_blocks_soft, and with both exactly vdl2gpu_decode_blocks; fb NULL: the
        # library's vdl2gpu_decode_blocks_report, which the older calls go through as well)
        if tarr is not None:
            mode = (_lib.BLK_ALL_FRAMES | (_lib.BLK_RAW_FLAGS if raw_flags else 0)) if all_frames else 0
            nf = self._check(self.L.vdl2gpu_decode_blocks_tracked(self.h, arr, sarr, farr, tarr, n, out, cap, C.byref(dropped), rarr, mode))
        elif all_frames:
            nf = self._check(self.L.vdl2gpu_decode_blocks_ex(self.h, arr, sarr, farr, n, out, cap, C.byref(dropped), rarr,
                                                             _lib.BLK_ALL_FRAMES | (_lib.BLK_RAW_FLAGS if raw_flags else 0)))
        elif farr is None:
            nf = self._check(self.L.vdl2gpu_decode_blocks_report(self.h, arr, sarr, n, out, cap, C.byref(dropped), rarr))
        else:
            nf = self._check(self.L.vdl2gpu_decode_blocks_feedback(self.h, arr, sarr, farr, n, out, cap, C.byref(dropped), rarr))
        if dropped.value:
            raise _lib.Vdl2GpuError(f"{dropped.value} frames dropped: raise max_frames")
        frames = [(out[i].block, bytes(out[i].data[:out[i].len])) for i in range(nf)]
        return (frames, [BlockReport.from_c(r) for r in rarr]) if report else frames

    def poll_frames(self, max_frames: int = 4096) -> List[Tuple[int, int, bytes]]:
        """(stream, chn, hdata) of every frame of everything pushed so far (needs frames=True)."""
        out = []
        buf = (_lib.FrameT * max_frames)()
        while True:
            n = self._check(self.L.vdl2gpu_poll_frames(self.h, buf, max_frames))
            out += [(buf[i].stream, buf[i].chn, bytes(buf[i].data[:buf[i].len])) for i in range(n)]
            if n < max_frames:
                return out

    # ------------------------------------------------------------------ bookkeeping
    def stats(self) -> dict:
        st = _lib.StatsT()
        self._check(self.L.vdl2gpu_get_stats(self.h, C.byref(st)))
        return {n: getattr(st, n) for n, _ in _lib.StatsT._fields_}

    def timing(self, reset: bool = False) -> dict:
        t = _lib.TimingT()
        self._check(self.L.vdl2gpu_get_timing(self.h, C.byref(t), int(reset)))
        return {n: getattr(t, n) for n, _ in _lib.TimingT._fields_}

    # ------------------------------------------------------------------ diagnostics
    def debug_dec(self, stream: int, ch: int, max_complex: int = 1 << 24) -> np.ndarray:
        buf = np.empty(2 * max_complex, np.float32)
        n = self.L.vdl2gpu_debug_dec(self.h, stream, ch, buf.ctypes.data_as(C.c_void_p), max_complex)
        self._check(int(n))
        return buf[:2 * n].view(np.complex64).copy()

    def debug_k1(self) -> dict:
        """channeliser launches since the handle was created, by kernel: k1_channelise with the LO table in LDS (`general_lds`) or in
        global memory (`general_global`: rates off the 25 kHz grid whose table does not fit LDS), `k1_pp`, `k1_fast`"""
        buf = (C.c_ulonglong * 4)()
        self._check(self.L.vdl2gpu_debug_k1(self.h, buf, 4))
        return dict(zip(("general_lds", "general_global", "k1_pp", "k1_fast"), (int(v) for v in buf)))

    def debug_atan2f(self, y: np.ndarray, x: np.ndarray) -> np.ndarray:
        y = np.ascontiguousarray(y, np.float32)
        x = np.ascontiguousarray(x, np.float32)
        out = np.empty_like(y)
        self._check(self.L.vdl2gpu_debug_atan2f(self.h, y.ctypes.data_as(C.c_void_p), x.ctypes.data_as(C.c_void_p),
                                                out.ctypes.data_as(C.c_void_p), y.size))
        return out

    def debug_rs(self, rows: np.ndarray, eras: np.ndarray, no_eras: np.ndarray):
        """rs() (rs.c:81-291) of every row on the device, through the block kernel's own row decoder: rows (n, 255) uint8,
        eras (n, 6) and no_eras (n,) int32 -> (ret, rows, eras) as rs() leaves them; the arguments are not modified."""
        rows = np.array(rows, np.uint8, order="C").reshape(-1, 255)
        n = rows.shape[0]
        eras = np.array(eras, np.int32, order="C").reshape(n, 6)
        no_eras = np.ascontiguousarray(no_eras, np.int32).reshape(n)
        ret = np.zeros(n, np.int32)
        self._check(self.L.vdl2gpu_debug_rs(self.h, rows.ctypes.data_as(C.c_void_p), eras.ctypes.data_as(C.c_void_p),
                                            no_eras.ctypes.data_as(C.c_void_p), ret.ctypes.data_as(C.c_void_p), n))
        return ret, rows, eras

    def debug_cands(self, stream: int, ch: int, max_cands: int = 6144) -> np.ndarray:
        buf = np.zeros((max_cands, 6), np.int32)
        n = self._check(self.L.vdl2gpu_debug_cands(self.h, stream, ch, buf.ctypes.data_as(C.c_void_p), max_cands))
        return buf[:n].copy()

    def host_profile(self, reset: bool = False) -> dict:
        """seconds of the calling thread inside vdl2gpu_push since the last reset: `enqueue` (launches and event operations) and
        `wait_for_ring` (blocked until the GPU has finished the push whose output ring, tables and planes this one reuses)"""
        buf = (C.c_double * 8)()
        self._check(self.L.vdl2gpu_get_host_profile(self.h, buf, int(reset)))
        v = list(buf)
        return {"wait_input": v[0], "enqueue": v[1] + v[3] + v[5], "wait_for_ring": v[2], "spill": v[4], "event_wait": v[6], "pushes": int(v[7])}

    def debug_clheads(self, stream: int, ch: int, max_cands: int = 6144) -> np.ndarray:
        """(n_s_rel, packed) per candidate of the last push, in debug_cands()'s order: where and how the idle search resumes."""
        buf = np.zeros((max_cands, 2), np.int32)
        n = self._check(self.L.vdl2gpu_debug_clheads(self.h, stream, ch, buf.ctypes.data_as(C.c_void_p), max_cands))
        return buf[:n].copy()

    def debug_heads(self, max_entries: int = 1 << 16) -> np.ndarray:
        """Header soft bits of every trigger of the last push (needs flags=lib.F_DEBUG_HEADS): structured array
        (nstar, sc, clk0, p2err, perr, err, pfr, soft[25])."""
        dt = np.dtype([("nstar", "<i8"), ("sc", "<i4"), ("clk0", "<i4"), ("p2err", "<f4"), ("perr", "<f4"),
                       ("err", "<f4"), ("pfr", "<f4"), ("soft", "<f4", (25,)), ("pad", "<u4")])
        buf = np.zeros(max_entries, dt)
        n = self._check(self.L.vdl2gpu_debug_heads(self.h, buf.ctypes.data_as(C.c_void_p), max_entries))
        return buf[:n].copy()

    def debug_counters(self, n: int = 16, reset: bool = True):
        buf = (C.c_ulonglong * max(64, n))()     # (64 words; the test library has 96: its escape and invariant counters lie behind)
        self._check(self.L.vdl2gpu_debug_counters(self.h, buf, n, int(reset)))
        return list(buf[:n])

    def close(self):
        if getattr(self, "h", None):
            self.L.vdl2gpu_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def choose_fc(freqs: Sequence[int], sdrinrate: int = 2_000_000, tuner: str = "rtl"):
    """The reference's frequency plan for a list of channel frequencies in Hz.

    tuner "rtl": chooseFc() of rtl.c:123-160, Fo = Fr - Fc (rtl.c:245-247); returns (Fc, [ThreadParam...]).
    tuner "air": chooseFc() of air.c:47-70, Fo = Fr - (Fc + SDRINRATE/4) (air.c:182-184); returns
    (Fc, [ThreadParam...], (r10, r11)) with the two R820T2 filter registers the reference writes at 5 MS/s.
    Fc == 0 means the reference refuses the list ("Frequencies too far apart")."""
    L = _lib.load()
    n = len(freqs)
    fr = (C.c_uint * n)(*[int(f) for f in freqs])
    fo = (C.c_int * n)()
    fc = C.c_uint(0)
    if tuner == "rtl":
        rc = L.vdl2gpu_choose_fc_rtl(fr, n, sdrinrate, C.byref(fc), fo)
        extra = None
    elif tuner == "air":
        r10, r11 = C.c_int(0), C.c_int(0)
        rc = L.vdl2gpu_choose_fc_air(fr, n, sdrinrate, C.byref(fc), fo, C.byref(r10), C.byref(r11))
        extra = (r10.value, r11.value)
    else:
        raise ValueError("tuner must be 'rtl' or 'air'")
    if rc < 0:
        raise _lib.Vdl2GpuError("vdl2gpu_choose_fc failed: " + L.vdl2gpu_strerror(rc).decode())
    plan = [ThreadParam(chn=i, Fr=int(freqs[i]), Fo=int(fo[i])) for i in range(n)]
    return (fc.value, plan) if extra is None else (fc.value, plan, extra)


def lo_table(sdrinrate: int, fo: int) -> np.ndarray:
    """Host LO table exactly as the library uploads it (d8psk.c:353-357)."""
    L = _lib.load()
    n = L.vdl2gpu_lo_len(sdrinrate)       # SDRINRATE / STEPRATE on the 25 kHz grid, the oscillator's true period off it
    buf = np.empty(2 * n, np.float32)
    rc = L.vdl2gpu_lo_table(sdrinrate, fo, buf.ctypes.data_as(C.c_void_p), n)
    if rc < 0:
        raise _lib.Vdl2GpuError("vdl2gpu_lo_table failed")
    return buf.view(np.complex64).copy()


def exact_fo_split(fo: int) -> Tuple[int, int]:
    """(Fg, Fd) of VDL2GPU_F_EXACT_FO: the 25 kHz grid point the mixer takes and the rest, -12500 <= Fd < 12500."""
    fg = STEPRATE * ((fo + STEPRATE // 2) // STEPRATE)
    return fg, fo - fg


def exact_fo_tables(sdrinrate: int) -> Tuple[np.ndarray, np.ndarray]:
    """(T_hi, T_lo) of VDL2GPU_F_EXACT_FO exactly as the library uploads them, complex64."""
    L = _lib.load()
    n = L.vdl2gpu_exact_fo_tables(sdrinrate, None, 0, None)
    if n < 0:
        raise _lib.Vdl2GpuError("vdl2gpu_exact_fo_tables failed")
    hi, lo = np.empty(2 * n, np.float32), np.empty(2 * 4096, np.float32)
    if L.vdl2gpu_exact_fo_tables(sdrinrate, hi.ctypes.data_as(C.c_void_p), n, lo.ctypes.data_as(C.c_void_p)) != n:
        raise _lib.Vdl2GpuError("vdl2gpu_exact_fo_tables failed")
    return hi.view(np.complex64).copy(), lo.view(np.complex64).copy()


def exact_fo_index(a: int, e: int, sdrinrate: int, fd_hz: int) -> int:
    """phase index of the window whose first and last inputs are samples a and e of the stream (vdl2gpu_exact_fo_index)"""
    k = _lib.load().vdl2gpu_exact_fo_index(a, e, sdrinrate, fd_hz)
    if k < 0:
        raise _lib.Vdl2GpuError("vdl2gpu_exact_fo_index failed")
    return int(k)


def plan(total_in: int, n: int, sdrclk: int, lo_len: int) -> Tuple[int, int, int, int]:
    """(c0, no0, nf0, nout): decimation schedule of one push (d8psk.c:374-381 closed form)."""
    L = _lib.load()
    c0, no0, nf0, nout = C.c_int(), C.c_int(), C.c_int(), C.c_int64()
    rc = L.vdl2gpu_plan(total_in, n, sdrclk, lo_len, C.byref(c0), C.byref(no0), C.byref(nf0), C.byref(nout))
    if rc < 0:
        raise _lib.Vdl2GpuError("vdl2gpu_plan failed")
    return c0.value, no0.value, nf0.value, nout.value
