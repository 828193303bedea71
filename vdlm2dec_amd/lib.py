"""ctypes binding of libvdl2gpu.so (the C ABI in include/vdl2gpu.h).

The library is the product; this module only loads it.  There is no Python or
CPU fallback: if the shared object is missing, or no HIP device is present when a
handle is created, an exception is raised.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libvdl2gpu.so")
LIB_TEST_PATH = os.path.join(_HERE, "libvdl2gpu_test.so")   # the same sources with -DVDL2GPU_TESTHOOKS (tests only)

FMT = {"cu8": 0, "cs16": 1, "cf32": 2, "f32": 3, "cs8": 4, "s16": 5}
SAMPLE_BYTES = {"cu8": 2, "cs16": 4, "cf32": 8, "f32": 4, "cs8": 2, "s16": 2}
MEM_HOST, MEM_DEVICE = 0, 1
F_KEEP_DEC = 1
F_SERIAL = 2
F_FULLSCAN = 4
F_TEST_NOREGION = 8
F_FRAMES = 16
F_RTL_QUIRK = 32
F_DEBUG_HEADS = 64
F_LEVELS = 128
F_SOFT_RS = 256
F_EXACT_FO = 512
F_CARRIER = 1024
F_BLOCK_REPORT = 2048
# vdl2gpu_blockrep_t.row_how (VDL2GPU_ROW_*)
ROW_NONE, ROW_CLEAN, ROW_REF, ROW_SOFT2, ROW_SOFT4, ROW_FAIL = range(6)
ROW_FEEDBACK = 6    # (VDL2GPU_F_FEEDBACK) the record's decision-feedback row replaced the row
F_FEEDBACK = 4096
F_ALL_FRAMES = 8192     # (VDL2GPU_F_ALL_FRAMES, needs F_FRAMES) the block path hands on every frame of a burst
BLK_ALL_FRAMES = 1      # vdl2gpu_decode_blocks_ex's mode word (VDL2GPU_BLK_*)
F_RAW_FLAGS = 16384     # (VDL2GPU_F_RAW_FLAGS, needs F_ALL_FRAMES) a flag is six adjacent ones of the stuffed stream: a data byte 0x7e is data
BLK_RAW_FLAGS = 4       # ... in the mode word, beside BLK_ALL_FRAMES
F_SYMCLK = 32768        # (VDL2GPU_F_SYMCLK) every burst's symbol timing, clock drift and fine arrival time (vdl2gpu_symclk_t)
SYMCLK_SEG, SYMCLK_SEGS = 256, 22      # VDL2GPU_SYMCLK_SEG symbols a segment, VDL2GPU_SYMCLK_SEGS segments a record
F_TRACKED = 65536       # (VDL2GPU_F_TRACKED) every burst's payload sliced a second time with a tracked sampling instant (vdl2gpu_trk_t)
TRK_SEG, TRK_SEGS = 256, 22            # VDL2GPU_TRK_SEG, VDL2GPU_TRK_SEGS
ROW_TRACKED = 7         # VDL2GPU_ROW_TRACKED: block report, row_how
# status of a cluster head (vdl2gpu_debug_clheads()'s packed word: cl_pack() in csrc/vdl2gpu_types.h)
CL_STEADY, CL_DEFER_FIRST, CL_NONSTEADY = 0, 1, 2


# vdl2gpu_debug_counters(): slot of every named development counter (enum K2Dbg in csrc/vdl2gpu_types.h without its K2_DBG_ prefix;
# tests/test_shared_words.py holds the two together).  Slots from ESC_REG on exist in the test library only.
DBG = {
    "K2B_RING_TICKS": 0, "K2B_REST_TICKS": 1, "K2B_SAMPLED": 2, "K2B_TRIG": 3, "K2B_EVAL": 4, "K2B_MAX_TICKS": 5,
    "K2B_STEADY": 6, "K2B_REJ": 7, "K2B_ORD_TICKS0": 8, "K2B_ORD_COUNT0": 12,
    "K2C_LOAD_TICKS": 16, "K2C_TABLES_TICKS": 17, "K2C_WALK_TICKS": 18, "K2C_PUBLISH_TICKS": 19, "K2C_CALLS": 20,
    "REPAIRED": 24, "K2C_REPLAYS": 25, "K2C_NONSTEADY": 26, "K2C_CANDS": 27, "K2C_VISITED": 28, "K2C_SERIAL_SAMPLES": 29,
    "VERIFY_INSTANTS": 30, "PROBE_STAGE0": 32, "REGION_STAGE0": 48,
    "ESC_REG": 64, "ESC_SEG": 65, "ESC_VIS": 66, "ESC_WIN": 67, "ESC_MERGE": 68, "ESC_SLOG": 69, "ESC_STAGE": 70,
    "INV_B_CLUSTER": 71, "INV_B_DECODE": 72, "INV_B_RECORD": 73, "INV_A": 74, "ESC_MERGE_SORT": 75,
    "ESC_PATCH_ABANDON": 76, "CHK_B_CLUSTER": 77, "CHK_B_DECODE": 78, "CHK_B_RECORD": 79, "CHK_A": 80,
}
# the sixteen stage slots behind PROBE_STAGE0 and REGION_STAGE0 (enum K2aStage without its K2A_ST_ prefix, lower case)
DBG_STAGES = ("stage_in", "fir_unit", "barrier_samples", "steps", "screen", "unused5", "unused6", "unused7",
              "screen_end", "barrier_tile", "unused10", "passes", "tiles_or_wait", "park", "unused14", "instants")
DBG_WORDS, DBG_WORDS_TEST = 64, 96      # VDL2_DBG_WORDS of the product and of the test library


def dbg_stages(counters, base):
    """'name value, ...' of the stage slots that counted, base = DBG["PROBE_STAGE0"] or DBG["REGION_STAGE0"]"""
    return ", ".join("%s %d" % (name, counters[base + i]) for i, name in enumerate(DBG_STAGES) if counters[base + i])


def cl_unpack(packed):
    """(status, r_s, nslots, ntrig, nrej, nburst) of a cluster head's packed word, as the device's cl_*() accessors read it"""
    p = int(packed) & 0xffffffff
    return p & 3, p >> 2 & 3, p >> 4 & 15, p >> 8 & 255, p >> 16 & 255, p >> 24 & 255


# every symbol include/vdl2gpu.h declares
EXPORTS = (
    "vdl2gpu_abi_version", "vdl2gpu_create", "vdl2gpu_destroy", "vdl2gpu_push", "vdl2gpu_sync",
    "vdl2gpu_ring_init", "vdl2gpu_ring_acquire", "vdl2gpu_ring_commit",
    "vdl2gpu_poll", "vdl2gpu_poll_ready", "vdl2gpu_poll_levels", "vdl2gpu_poll_levels_ready", "vdl2gpu_poll_soft", "vdl2gpu_poll_soft_ready", "vdl2gpu_poll_carrier", "vdl2gpu_poll_carrier_ready", "vdl2gpu_poll_report", "vdl2gpu_poll_report_ready", "vdl2gpu_poll_feedback", "vdl2gpu_poll_feedback_ready", "vdl2gpu_poll_symclk", "vdl2gpu_poll_symclk_ready", "vdl2gpu_poll_tracked", "vdl2gpu_poll_tracked_ready", "vdl2gpu_pending", "vdl2gpu_inflight", "vdl2gpu_get_stats", "vdl2gpu_get_timing", "vdl2gpu_get_host_profile", "vdl2gpu_last_error",
    "vdl2gpu_strerror", "vdl2gpu_burst_to_msgblk", "vdl2gpu_decode_blocks", "vdl2gpu_decode_blocks_soft", "vdl2gpu_decode_blocks_report", "vdl2gpu_decode_blocks_feedback", "vdl2gpu_decode_blocks_ex", "vdl2gpu_decode_blocks_tracked", "vdl2gpu_poll_frames", "vdl2gpu_poll_frames_ready", "reversebits", "vdl2gpu_lo_len", "vdl2gpu_lo_table", "vdl2gpu_plan",
    "vdl2gpu_exact_fo_tables", "vdl2gpu_exact_fo_index", "vdl2gpu_carrier_from_sums", "vdl2gpu_symclk_from_sums",
    "vdl2gpu_choose_fc_rtl", "vdl2gpu_choose_fc_air",
    "vdl2gpu_debug_dec", "vdl2gpu_debug_k1", "vdl2gpu_debug_lo", "vdl2gpu_debug_atan2f", "vdl2gpu_debug_rs", "vdl2gpu_debug_counters", "vdl2gpu_debug_cands", "vdl2gpu_debug_clheads", "vdl2gpu_debug_fail", "vdl2gpu_debug_segs", "vdl2gpu_debug_heads",
)


class ChanT(C.Structure):
    _fields_ = [("chn", C.c_int32), ("Fr", C.c_int32), ("Fo", C.c_int32)]


class ConfigT(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("sdrinrate", C.c_uint32), ("sdrclk", C.c_uint32),
                ("fmt", C.c_int32), ("nbch", C.c_int32), ("nstreams", C.c_int32),
                ("chan", C.POINTER(ChanT)), ("max_push", C.c_uint64), ("device", C.c_int32),
                ("max_bursts", C.c_uint32), ("flags", C.c_uint32)]


class BurstT(C.Structure):
    _fields_ = [("stream", C.c_int32), ("chn", C.c_int32), ("Fr", C.c_int32), ("nbrow", C.c_int32),
                ("nlbyte", C.c_int32), ("df", C.c_float), ("ppm", C.c_float),
                ("trig_dec", C.c_int64), ("end_dec", C.c_int64), ("trig_sample", C.c_int64),
                ("end_sample", C.c_int64), ("data", (C.c_uint8 * 255) * 8)]


class LevelT(C.Structure):
    """vdl2gpu_level_t (VDL2GPU_F_LEVELS): 40 bytes, see include/vdl2gpu.h for the definitions."""
    _fields_ = [("sig_dbfs", C.c_float), ("noise_dbfs", C.c_float), ("sig_power", C.c_float), ("noise_power", C.c_float),
                ("sym_first_dec", C.c_int64), ("nsym", C.c_int32), ("subphase", C.c_int32), ("noise_blocks", C.c_int32),
                ("reserved", C.c_int32)]


class SoftT(C.Structure):
    """vdl2gpu_soft_t (VDL2GPU_F_SOFT_RS): 2048 bytes, the reliability of every payload byte (include/vdl2gpu.h)."""
    _fields_ = [("rel", (C.c_uint8 * 255) * 8), ("reserved", C.c_uint8 * 8)]


class CarrierT(C.Structure):
    """vdl2gpu_carrier_t (VDL2GPU_F_CARRIER): 32 bytes, the burst's phase-error sums and the carrier offset and spread the host derives
    from them (include/vdl2gpu.h)."""
    _fields_ = [("nsym", C.c_int32), ("sum_e", C.c_int32), ("sum_e2", C.c_uint32), ("reserved", C.c_int32),
                ("dphi", C.c_float), ("freq_hz", C.c_float), ("ppm", C.c_float), ("rms_rad", C.c_float)]


class BlockRepT(C.Structure):
    """vdl2gpu_blockrep_t (VDL2GPU_F_BLOCK_REPORT): 48 bytes, what the block path made of a burst -- RS outcome per row, un-stuffing,
    flag hunt and FCS counts (include/vdl2gpu.h)."""
    _fields_ = [("row_roots", C.c_int8 * 8), ("row_how", C.c_uint8 * 8), ("row_changed", C.c_uint8 * 8),
                ("bytes_changed", C.c_uint16), ("rows_failed", C.c_uint16), ("rows_rescued", C.c_uint16), ("stuffed", C.c_uint16),
                ("nbytes", C.c_uint16), ("flag_at", C.c_int16), ("cand", C.c_uint16), ("too_short", C.c_uint16),
                ("bad_fcs", C.c_uint16), ("frames", C.c_uint16), ("status", C.c_int32)]


class FbT(C.Structure):
    """vdl2gpu_fb_t (VDL2GPU_F_FEEDBACK): 2048 bytes, the rows of the burst sliced a second time with decision feedback, laid out as the
    record's data[] (include/vdl2gpu.h)."""
    _fields_ = [("data", (C.c_uint8 * 255) * 8), ("reserved", C.c_uint8 * 8)]


class SymClkT(C.Structure):
    """vdl2gpu_symclk_t (VDL2GPU_F_SYMCLK): 744 bytes, the burst's square-law timing sums by segment of 256 symbols and the symbol timing,
    clock drift and arrival time the host derives from them (include/vdl2gpu.h)."""
    _fields_ = [("sym_first_dec", C.c_int64), ("nsym", C.c_int32), ("nseg", C.c_int32), ("toa_sample", C.c_double),
                ("tau0", C.c_float), ("clock_ppm", C.c_float), ("tau_rms", C.c_float), ("reserved", C.c_int32),
                ("e", (C.c_float * 8) * 22)]


class TrkT(C.Structure):
    """vdl2gpu_trk_t (VDL2GPU_F_TRACKED): 2048 bytes, the rows of the timing-tracked slice laid out as the record's data[], and the
    quarter-sample offsets the segments chose (include/vdl2gpu.h)."""
    _fields_ = [("data", (C.c_uint8 * 255) * 8), ("d_first", C.c_int8), ("d_last", C.c_int8), ("d_min", C.c_int8), ("d_max", C.c_int8),
                ("nseg", C.c_uint8), ("reserved", C.c_uint8 * 3)]


class FrameT(C.Structure):
    _fields_ = [("stream", C.c_int32), ("chn", C.c_int32), ("Fr", C.c_int32), ("nbrow", C.c_int32),
                ("nlbyte", C.c_int32), ("len", C.c_int32), ("block", C.c_int32), ("seq", C.c_int32),
                ("df", C.c_float), ("ppm", C.c_float), ("trig_dec", C.c_int64), ("end_dec", C.c_int64),
                ("data", C.c_uint8 * 2000)]


class StatsT(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("samples_in", "dec_samples", "sync_evals", "triggers",
                                          "header_rejects", "bursts", "deferrals", "candidates", "serial_redos", "serial_samples", "overflowed",
                                          "frames_dropped", "repairs")]


class TimingT(C.Structure):
    _fields_ = [("channelise_ms", C.c_double), ("demod_ms", C.c_double), ("scan_ms", C.c_double),
                ("cluster_ms", C.c_double), ("resolve_ms", C.c_double), ("other_ms", C.c_double),
                ("channelise_fast_ms", C.c_double), ("fast_pushes", C.c_uint64),
                ("pushes", C.c_uint64), ("samples", C.c_uint64)]


class Vdl2GpuError(RuntimeError):
    pass


_libs = {}


def load(testhooks: bool = False):
    """Load libvdl2gpu.so (or, for the tests' handicaps, libvdl2gpu_test.so); raises if the HIP
    extension has not been built."""
    if testhooks in _libs:
        return _libs[testhooks]
    path = LIB_TEST_PATH if testhooks else LIB_PATH
    if not testhooks and os.environ.get("VDL2GPU_LIB"):
        path = os.environ["VDL2GPU_LIB"]      # development: another build of the same library (scripts/dev/abv.sh compares variants on one box)
    if testhooks and os.environ.get("VDL2GPU_LIB_TEST"):
        path = os.environ["VDL2GPU_LIB_TEST"]  # development: another -DVDL2GPU_TESTHOOKS build (bisecting with scripts/soak.py)
    if not os.path.exists(path):
        raise Vdl2GpuError(
            f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    if not os.environ.get("VDL2GPU_NO_TORCH"):
        # PyTorch wheels bundle their own libamdhip64.so.7 / libhsa-runtime64; two HSA runtimes in
        # one process cannot both own the GPU.  Importing torch first makes its runtime the one this
        # library binds to (same SONAME), so tensors' device pointers can be pushed directly.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    L = C.CDLL(path)
    L.vdl2gpu_abi_version.restype = C.c_int
    L.vdl2gpu_create.restype = C.c_int
    L.vdl2gpu_create.argtypes = [C.POINTER(ConfigT), C.POINTER(C.c_void_p)]
    L.vdl2gpu_destroy.restype = None
    L.vdl2gpu_destroy.argtypes = [C.c_void_p]
    L.vdl2gpu_push.restype = C.c_int
    L.vdl2gpu_push.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int]
    L.vdl2gpu_ring_init.restype = C.c_int
    L.vdl2gpu_ring_init.argtypes = [C.c_void_p, C.c_size_t, C.c_int]
    L.vdl2gpu_ring_acquire.restype = C.c_void_p
    L.vdl2gpu_ring_acquire.argtypes = [C.c_void_p, C.POINTER(C.c_size_t)]
    L.vdl2gpu_ring_commit.restype = C.c_int
    L.vdl2gpu_ring_commit.argtypes = [C.c_void_p, C.c_size_t]
    L.vdl2gpu_sync.restype = C.c_int
    L.vdl2gpu_sync.argtypes = [C.c_void_p]
    L.vdl2gpu_poll.restype = C.c_int
    L.vdl2gpu_poll.argtypes = [C.c_void_p, C.POINTER(BurstT), C.c_int]
    L.vdl2gpu_poll_ready.restype = C.c_int
    L.vdl2gpu_poll_ready.argtypes = [C.c_void_p, C.POINTER(BurstT), C.c_int]
    L.vdl2gpu_pending.restype = C.c_int
    L.vdl2gpu_poll_levels.restype = C.c_int
    L.vdl2gpu_poll_levels.argtypes = [C.c_void_p, C.POINTER(BurstT), C.POINTER(LevelT), C.c_int]
    L.vdl2gpu_poll_levels_ready.restype = C.c_int
    L.vdl2gpu_poll_levels_ready.argtypes = [C.c_void_p, C.POINTER(BurstT), C.POINTER(LevelT), C.c_int]
    L.vdl2gpu_pending.argtypes = [C.c_void_p]
    L.vdl2gpu_poll_soft.restype = C.c_int
    L.vdl2gpu_poll_soft.argtypes = [C.c_void_p, C.POINTER(BurstT), C.POINTER(LevelT), C.POINTER(SoftT), C.c_int]
    L.vdl2gpu_poll_soft_ready.restype = C.c_int
    L.vdl2gpu_poll_soft_ready.argtypes = [C.c_void_p, C.POINTER(BurstT), C.POINTER(LevelT), C.POINTER(SoftT), C.c_int]
    L.vdl2gpu_poll_carrier.restype = C.c_int
    L.vdl2gpu_poll_carrier.argtypes = [C.c_void_p, C.POINTER(BurstT), C.POINTER(LevelT), C.POINTER(SoftT), C.POINTER(CarrierT), C.c_int]
    L.vdl2gpu_poll_carrier_ready.restype = C.c_int
    L.vdl2gpu_poll_carrier_ready.argtypes = [C.c_void_p, C.POINTER(BurstT), C.POINTER(LevelT), C.POINTER(SoftT), C.POINTER(CarrierT), C.c_int]
    L.vdl2gpu_poll_report.restype = C.c_int
    L.vdl2gpu_poll_report.argtypes = [C.c_void_p, C.POINTER(BurstT), C.POINTER(LevelT), C.POINTER(SoftT), C.POINTER(CarrierT), C.POINTER(BlockRepT), C.c_int]
    L.vdl2gpu_poll_report_ready.restype = C.c_int
    L.vdl2gpu_poll_report_ready.argtypes = [C.c_void_p, C.POINTER(BurstT), C.POINTER(LevelT), C.POINTER(SoftT), C.POINTER(CarrierT), C.POINTER(BlockRepT), C.c_int]
    L.vdl2gpu_poll_feedback.restype = C.c_int
    L.vdl2gpu_poll_feedback.argtypes = [C.c_void_p, C.POINTER(BurstT), C.POINTER(LevelT), C.POINTER(SoftT), C.POINTER(CarrierT), C.POINTER(BlockRepT), C.POINTER(FbT), C.c_int]
    L.vdl2gpu_poll_feedback_ready.restype = C.c_int
    L.vdl2gpu_poll_feedback_ready.argtypes = [C.c_void_p, C.POINTER(BurstT), C.POINTER(LevelT), C.POINTER(SoftT), C.POINTER(CarrierT), C.POINTER(BlockRepT), C.POINTER(FbT), C.c_int]
    L.vdl2gpu_poll_symclk.restype = C.c_int
    L.vdl2gpu_poll_symclk.argtypes = [C.c_void_p, C.POINTER(BurstT), C.POINTER(LevelT), C.POINTER(SoftT), C.POINTER(CarrierT), C.POINTER(BlockRepT), C.POINTER(FbT),
                                      C.POINTER(SymClkT), C.c_int]
    L.vdl2gpu_poll_symclk_ready.restype = C.c_int
    L.vdl2gpu_poll_symclk_ready.argtypes = L.vdl2gpu_poll_symclk.argtypes
    L.vdl2gpu_poll_tracked.restype = C.c_int
    L.vdl2gpu_poll_tracked.argtypes = [C.c_void_p, C.POINTER(BurstT), C.POINTER(LevelT), C.POINTER(SoftT), C.POINTER(CarrierT), C.POINTER(BlockRepT), C.POINTER(FbT),
                                       C.POINTER(SymClkT), C.POINTER(TrkT), C.c_int]
    L.vdl2gpu_poll_tracked_ready.restype = C.c_int
    L.vdl2gpu_poll_tracked_ready.argtypes = L.vdl2gpu_poll_tracked.argtypes
    L.vdl2gpu_symclk_from_sums.restype = C.c_int
    L.vdl2gpu_symclk_from_sums.argtypes = [C.c_int64, C.c_int, C.POINTER(C.c_float), C.c_uint, C.POINTER(SymClkT), C.POINTER(C.c_double)]
    L.vdl2gpu_carrier_from_sums.restype = C.c_int
    L.vdl2gpu_carrier_from_sums.argtypes = [C.c_float, C.c_int, C.c_int, C.c_int, C.c_uint, C.POINTER(CarrierT)]
    L.vdl2gpu_get_stats.restype = C.c_int
    L.vdl2gpu_get_stats.argtypes = [C.c_void_p, C.POINTER(StatsT)]
    L.vdl2gpu_get_timing.restype = C.c_int
    L.vdl2gpu_get_timing.argtypes = [C.c_void_p, C.POINTER(TimingT), C.c_int]
    L.vdl2gpu_get_host_profile.restype = C.c_int
    L.vdl2gpu_get_host_profile.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int]
    L.vdl2gpu_last_error.restype = C.c_char_p
    L.vdl2gpu_last_error.argtypes = [C.c_void_p]
    L.vdl2gpu_strerror.restype = C.c_char_p
    L.vdl2gpu_strerror.argtypes = [C.c_int]
    L.vdl2gpu_burst_to_msgblk.restype = C.c_int
    L.vdl2gpu_burst_to_msgblk.argtypes = [C.POINTER(BurstT), C.c_void_p, C.c_size_t]
    L.vdl2gpu_decode_blocks.restype = C.c_int
    L.vdl2gpu_decode_blocks.argtypes = [C.c_void_p, C.POINTER(BurstT), C.c_int, C.POINTER(FrameT), C.c_int,
                                        C.POINTER(C.c_int)]
    L.vdl2gpu_decode_blocks_soft.restype = C.c_int
    L.vdl2gpu_decode_blocks_soft.argtypes = [C.c_void_p, C.POINTER(BurstT), C.POINTER(SoftT), C.c_int, C.POINTER(FrameT), C.c_int,
                                             C.POINTER(C.c_int)]
    L.vdl2gpu_decode_blocks_report.restype = C.c_int
    L.vdl2gpu_decode_blocks_report.argtypes = [C.c_void_p, C.POINTER(BurstT), C.POINTER(SoftT), C.c_int, C.POINTER(FrameT), C.c_int,
                                               C.POINTER(C.c_int), C.POINTER(BlockRepT)]
    L.vdl2gpu_decode_blocks_feedback.restype = C.c_int
    L.vdl2gpu_decode_blocks_feedback.argtypes = [C.c_void_p, C.POINTER(BurstT), C.POINTER(SoftT), C.POINTER(FbT), C.c_int, C.POINTER(FrameT), C.c_int,
                                                 C.POINTER(C.c_int), C.POINTER(BlockRepT)]
    L.vdl2gpu_decode_blocks_ex.restype = C.c_int
    L.vdl2gpu_decode_blocks_ex.argtypes = [C.c_void_p, C.POINTER(BurstT), C.POINTER(SoftT), C.POINTER(FbT), C.c_int, C.POINTER(FrameT), C.c_int,
                                           C.POINTER(C.c_int), C.POINTER(BlockRepT), C.c_uint32]
    L.vdl2gpu_decode_blocks_tracked.restype = C.c_int
    L.vdl2gpu_decode_blocks_tracked.argtypes = [C.c_void_p, C.POINTER(BurstT), C.POINTER(SoftT), C.POINTER(FbT), C.POINTER(TrkT), C.c_int, C.POINTER(FrameT),
                                                C.c_int, C.POINTER(C.c_int), C.POINTER(BlockRepT), C.c_uint32]
    L.vdl2gpu_poll_frames.restype = C.c_int
    L.vdl2gpu_poll_frames.argtypes = [C.c_void_p, C.POINTER(FrameT), C.c_int]
    L.vdl2gpu_poll_frames_ready.restype = C.c_int
    L.vdl2gpu_poll_frames_ready.argtypes = [C.c_void_p, C.POINTER(FrameT), C.c_int]
    L.reversebits.restype = C.c_uint
    L.reversebits.argtypes = [C.c_uint, C.c_int]
    L.vdl2gpu_lo_len.restype = C.c_int
    L.vdl2gpu_lo_len.argtypes = [C.c_uint]
    L.vdl2gpu_lo_table.restype = C.c_int
    L.vdl2gpu_lo_table.argtypes = [C.c_uint, C.c_int, C.c_void_p, C.c_int]
    L.vdl2gpu_plan.restype = C.c_int
    L.vdl2gpu_plan.argtypes = [C.c_uint64, C.c_uint64, C.c_uint, C.c_uint, C.POINTER(C.c_int),
                               C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int64)]
    L.vdl2gpu_exact_fo_tables.restype = C.c_int
    L.vdl2gpu_exact_fo_tables.argtypes = [C.c_uint, C.c_void_p, C.c_int, C.c_void_p]
    L.vdl2gpu_exact_fo_index.restype = C.c_int64
    L.vdl2gpu_exact_fo_index.argtypes = [C.c_uint64, C.c_uint64, C.c_uint, C.c_int]
    L.vdl2gpu_choose_fc_rtl.restype = C.c_int
    L.vdl2gpu_choose_fc_rtl.argtypes = [C.POINTER(C.c_uint), C.c_int, C.c_uint, C.POINTER(C.c_uint), C.POINTER(C.c_int)]
    L.vdl2gpu_choose_fc_air.restype = C.c_int
    L.vdl2gpu_choose_fc_air.argtypes = [C.POINTER(C.c_uint), C.c_int, C.c_uint, C.POINTER(C.c_uint), C.POINTER(C.c_int),
                                        C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.vdl2gpu_debug_dec.restype = C.c_int64
    L.vdl2gpu_debug_dec.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64]
    L.vdl2gpu_debug_k1.restype = C.c_int
    L.vdl2gpu_debug_k1.argtypes = [C.c_void_p, C.POINTER(C.c_ulonglong), C.c_int]
    L.vdl2gpu_debug_lo.restype = C.c_int
    L.vdl2gpu_debug_lo.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]
    L.vdl2gpu_debug_atan2f.restype = C.c_int
    L.vdl2gpu_debug_atan2f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    L.vdl2gpu_debug_rs.restype = C.c_int
    L.vdl2gpu_debug_rs.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    L.vdl2gpu_debug_fail.restype = C.c_int
    L.vdl2gpu_debug_fail.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    L.vdl2gpu_debug_segs.restype = C.c_int
    L.vdl2gpu_debug_segs.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]
    L.vdl2gpu_debug_cands.restype = C.c_int
    L.vdl2gpu_debug_cands.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]
    L.vdl2gpu_debug_clheads.restype = C.c_int
    L.vdl2gpu_debug_clheads.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]
    L.vdl2gpu_debug_heads.restype = C.c_int
    L.vdl2gpu_debug_heads.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    L.vdl2gpu_debug_counters.restype = C.c_int
    L.vdl2gpu_debug_counters.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    _libs[testhooks] = L
    return L
