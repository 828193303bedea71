"""numpy restatement of the per-burst levels (VDL2GPU_F_LEVELS; the definitions are in include/vdl2gpu.h).

x: one channel's 84 kS/s plane (complex, x[n] = stream time n), mflt: the 65 channel-filter taps."""
from __future__ import annotations

import numpy as np

GUARD, NEVAL, BLOCK = 512, 256, 32
FS = {"cu8": 128.0, "cs16": 32768.0, "cf32": 1.0, "f32": 1.0}


def s_values(x: np.ndarray, n: np.ndarray, c: int, mflt: np.ndarray) -> np.ndarray:
    """S(n, c) = sum_j x[n - 16 + j] * mflt[c + 4j] over j >= 0, c + 4j <= 64 (float64)."""
    taps = np.asarray(mflt, np.float64)[c::4]
    n = np.asarray(n, np.int64)
    idx = n[:, None] - 16 + np.arange(len(taps))[None, :]
    return (np.asarray(x, np.complex128)[idx] * taps[None, :]).sum(axis=1)


def levels(x: np.ndarray, mflt: np.ndarray, first: int, nsym: int, c: int):
    """(sig_power, noise_power, noise_blocks) of a burst whose symbols are first + 8k (k < nsym) at sub-phase c."""
    sig = float(np.mean(np.abs(s_values(x, first + 8 * np.arange(nsym), c, mflt)) ** 2))
    means = []
    for b in range(NEVAL // BLOCK):
        i = np.arange(BLOCK * b, BLOCK * b + BLOCK)
        m = first - GUARD - 8 * i
        if m[-1] - 16 < 0:
            continue
        means.append(float(np.mean(np.abs(s_values(x, m, 0, mflt)) ** 2)))
    noise = float(np.median(means)) if means else float("nan")
    return sig, noise, len(means)


def scale_k(fmt: str, sdrinrate: int, mflt: np.ndarray) -> float:
    """K: |S|^2 of a full-scale complex tone at the channel centre.  The channeliser averages the input samples of an output
    (d8psk.c:378), so such a tone leaves it at FS whatever sdrinrate is."""
    return (FS[fmt] * float(np.sum(np.asarray(mflt, np.float64)[0::4]))) ** 2


def mflt_taps() -> np.ndarray:
    """The 65 taps as the library holds them (csrc/vdl2_tables.inc)."""
    import os
    import re
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vdlm2dec_amd", "csrc", "vdl2_tables.inc")
    text = open(path).read()
    body = text[text.index("VDL2_TABLE_BEGIN(mflt, 65)"):]
    body = body[:body.index("VDL2_TABLE_END")]
    words = [int(w, 16) for w in re.findall(r"VDL2_F32\((0x[0-9a-f]+)u\)", body)]
    assert len(words) == 65
    return np.array(words, np.uint32).view(np.float32)
