"""What VDL2GPU_F_TRACKED gains: frames delivered, the reference's block path against the one with the second attempt, over a grid of
symbol-clock offsets, burst lengths and noise levels, 16 bursts a point (one burst a stream, cs16 at 2 MS/s, fo 100 kHz, amp 30: the
generator of tests/test_tracked_model.py with the seed counting on).

    sym_ppm 0, +-25, +-50, +-100   x   info 230 / 700 / 1625 bytes   x   noise 1.7 and 26 (near the floor: at 28 the reference loses half the 700-byte bursts at 0 ppm)

At every point the GPU must equal the model (tests/tracked_ref.py on the CPU model's plane: the column byte for byte, the frames of
tracked_ref.second_attempt), and no frame may appear that was not sent; the script exits non-zero otherwise.  A burst the detector does
not find counts as not delivered on both sides.

    python scripts/tracked_gain.py [--bursts 16] [--noise 1.7 26] [--ppm ...] [--info ...]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import soft_ref as R  # noqa: E402
import tracked_ref as T  # noqa: E402
from test_tracked_model import FC, FO, RATE, table_case  # noqa: E402
from oracle import oracle as O  # noqa: E402
from vdlm2dec_amd import synth  # noqa: E402
from vdlm2dec_amd.demod import Receiver, plan_channels  # noqa: E402


def point(plan, ppm, info, noise, nbursts, pn):
    """(sent, found, reference frames, tracked frames, rows taken) of one grid point; raises on any GPU / model difference"""
    sent = found = ref = trk = taken_rows = 0
    for seed in range(nbursts):
        raw, tx = table_case(seed, ppm, noise=noise, n=info)
        nbrow, nlbyte, rows = synth.received_rows(tx.payload())
        want = O.frames_of_block(nbrow, nlbyte, rows)
        sent += len(want)
        ch = O.OracleChannel(RATE, FO, FC + FO, tap_dec=True)
        ch.feed(raw, "cs16")
        x, blocks = ch.dec(), ch.blocks()
        ch.close()
        model = {}
        for b in blocks:
            col = T.burst_column(x, b.nbrow, b.nlbyte, b.df, b.end_dec, pn)
            fr, _, taken = T.second_attempt(b.data, col["data"], None, None, b.nbrow, b.nlbyte)
            model[b.trig_dec] = (b, col, fr, taken)
        out = []
        for on in (False, True):     # (a handle per burst: its stream time starts at 0, as the model's does)
            with Receiver(RATE, plan, fmt="cs16", max_push=raw.size // 2, frames=True, tracked=on) as rx:
                rx.push(raw)
                bursts = rx.poll()
                out.append((bursts, [f for _, _, f in rx.poll_frames()]))
        (pb, pf), (tb, tf) = out
        if sorted(b.key() for b in pb) != sorted(b.key() for b in tb) or sorted((0, b.chn, b.nbrow, b.nlbyte, b.data) for b, _, _, _ in model.values()) != sorted(b.key() for b in pb):
            raise SystemExit(f"tracked_gain: the burst records differ (ppm {ppm} info {info} noise {noise} seed {seed})")
        m_ref, m_trk = [], []
        for b in tb:
            mb, col, fr, taken = model[b.trig_dec]
            if b.trk.raw != T.column_bytes(col):
                raise SystemExit(f"tracked_gain: the GPU's column is not the model's (ppm {ppm} info {info} noise {noise} seed {seed})")
            m_ref += O.frames_of_block(mb.nbrow, mb.nlbyte, mb.data)
            m_trk += fr
            taken_rows += len(taken)
        if sorted(pf) != sorted(m_ref) or sorted(tf) != sorted(m_trk):
            raise SystemExit(f"tracked_gain: the GPU's frames are not the model's (ppm {ppm} info {info} noise {noise} seed {seed})")
        if any(f not in want for f in pf + tf):
            raise SystemExit(f"tracked_gain: a frame that was not sent (ppm {ppm} info {info} noise {noise} seed {seed})")
        found += len(tb)
        ref += len(pf)
        trk += len(tf)
    return sent, found, ref, trk, taken_rows


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--bursts", type=int, default=16)
    ap.add_argument("--ppm", type=float, nargs="+", default=[0, 25, -25, 50, -50, 100, -100])
    ap.add_argument("--info", type=int, nargs="+", default=[230, 700, 1625])
    ap.add_argument("--noise", type=float, nargs="+", default=[1.7, 26.0])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tracked_gain: needs a GPU")
    pn = R.pn_bits()
    plan = plan_channels(FC, (FO,))
    print("# frames delivered of the frames sent: the reference's block path / with VDL2GPU_F_TRACKED; GPU == model at every point")
    print("# noise  info  sym_ppm  sent  bursts found  reference  tracked  rows taken by attempt B")
    total = [0, 0, 0]
    for noise in a.noise:
        for info in a.info:
            for ppm in a.ppm:
                sent, found, ref, trk, rows = point(plan, ppm, info, noise, a.bursts, pn)
                print(f"{noise:6.1f} {info:5d} {ppm:+8.0f} {sent:5d} {found:13d} {ref:10d} {trk:8d} {rows:6d}", flush=True)
                total = [total[0] + sent, total[1] + ref, total[2] + trk]
    print(json.dumps({"sent": total[0], "reference": total[1], "tracked": total[2], "gpu_equals_model": True, "unsent_frames": 0}))


if __name__ == "__main__":
    main()
