"""Crafted blocks for the soft row rule (tests/soft_ref.py, include/vdl2gpu.h vdl2gpu_soft_t): real AVLC frames, RS-encoded as the
transmitter does, with byte errors injected into one row either on its least reliable bytes or on reliable ones."""
from __future__ import annotations

import numpy as np

from vdlm2dec_amd import synth

import soft_ref as R

# payload lengths (bytes) that give every last-row regime: nlbyte <= 2, <= 30, <= 67, > 67, for 1 .. 8 rows
LENGTHS = (20, 60, 100, 200, 249 + 2, 249 + 25, 249 + 60, 249 + 150, 2 * 249 + 1, 2 * 249 + 40, 3 * 249 + 100, 4 * 249 + 20,
           5 * 249 + 66, 6 * 249 + 2, 7 * 249 + 200, 8 * 249 - 20)


def _payload(rng, n):
    """an HDLC payload of exactly n bytes holding one AVLC frame (flag fill behind it)"""
    p = synth.hdlc_payload(synth.avlc_frame(bytes(rng.integers(0, 256, max(1, n - 30), dtype=np.uint8).tolist())))
    while len(p) > n:
        p = synth.hdlc_payload(synth.avlc_frame(bytes(rng.integers(0, 256, max(1, n - 30 - (len(p) - n)), dtype=np.uint8).tolist())))
    return p + b"\x7e" * (n - len(p))


def cases(seed=77):
    """[(nbrow, nlbyte, received data (8, 255), rel (8, 255), sent data (8, 255), row, nerr, on_least)]"""
    rng = np.random.default_rng(seed)
    out = []
    for n in LENGTHS:
        nbrow, nlbyte, rows = synth.received_rows(_payload(rng, n))
        sent = np.frombuffer(rows, np.uint8).reshape(8, 255).copy()
        for r in range(nbrow):
            by, eras, p = R.row_params(r, nbrow, nlbyte)
            cand = list(range(by)) + list(range(249, 249 + p))
            room = 6 - len(eras)
            if room < 4 or len(cand) < 8:
                continue
            for nerr in ((4, 5) if room == 6 else (2, 3)):
                for on_least in (True, False):
                    rel = np.full((8, 255), 255, np.uint8)
                    for rr in range(nbrow):
                        b2, _, p2 = R.row_params(rr, nbrow, nlbyte)
                        rel[rr, :b2] = rng.integers(120, 256, b2)
                        rel[rr, 249:249 + p2] = rng.integers(120, 256, p2)
                    pick = rng.choice(len(cand), size=2 * nerr, replace=False)
                    low, other = [cand[i] for i in pick[:nerr]], [cand[i] for i in pick[nerr:]]
                    for j, c in enumerate(low):          # the least reliable bytes of the row
                        rel[r, c] = 5 + 3 * j
                    data = sent.copy()
                    for c in (low if on_least else other):
                        data[r, c] ^= int(rng.integers(1, 256))
                    out.append((nbrow, nlbyte, data, rel, sent, r, nerr, on_least))
    return out
