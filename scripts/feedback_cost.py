"""What VDL2GPU_F_FEEDBACK costs: the headline workload with the block path (8 ch @ 2 MS/s cs16, frames=True, device-resident samples,
bench.py's recordings and push size), without and with the flag, alternating x3, on one box.  Prints ms per step and the frames per
step, and checks that the burst records are byte-identical between the two modes, that every frame of the plain mode is also a frame
with the flag, and that every record with the flag carries rows.  For the payload kernel's own time beside its sibling's run it under
rocprofv3 --kernel-trace --stats with --mode off / --mode on (one mode per run): k2d_payload against k2d_payload_fb.

    python scripts/feedback_cost.py [--steps 4] [--warmup 2] [--rounds 3] [--mode both|off|on] [--bps 4.0]
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from vdlm2dec_amd import lib, synth  # noqa: E402
from vdlm2dec_amd.demod import Receiver, plan_channels  # noqa: E402


def run(dev, batch, feedback, steps, warmup):
    buf = (lib.BurstT * 16384)()
    fv = (lib.FbT * 16384)() if feedback else None
    fbuf = (lib.FrameT * 8192)()      # (allocated once: 16 MB)
    h = hashlib.sha256()
    nrec = nrows = nframes = 0
    with Receiver(2_000_000, plan_channels(bench.FC, synth.DEFAULT_FO_8CH), fmt="cs16", max_push=batch, max_bursts=1 << 18,
                  frames=True, feedback=feedback) as rx:
        def drain(timed):
            nonlocal nrec, nrows, nframes
            while True:
                n = rx.poll_feedback_raw(buf, None, None, None, None, fv, 16384)
                if timed:
                    h.update(C.string_at(C.addressof(buf), n * C.sizeof(lib.BurstT)))
                    nrec += n
                    if feedback:
                        nrows += sum(any(fv[i].data[0]) for i in range(0, n, max(1, n // 64)))
                if n < 16384:
                    break
            while True:
                n = rx._check(rx.L.vdl2gpu_poll_frames(rx.h, fbuf, 8192))
                if timed:
                    nframes += n
                if n < 8192:
                    break
        for _ in range(warmup):
            rx.push_device(dev.data_ptr(), batch)
            drain(False)
        rx.sync()
        t0 = time.perf_counter()
        for _ in range(steps):
            rx.push_device(dev.data_ptr(), batch)
            drain(True)
        rx.sync()
        dt = time.perf_counter() - t0
        rx.push_device(dev.data_ptr(), batch)       # once more, untimed: the frames themselves
        while rx.poll_feedback_raw(buf, None, None, None, None, fv, 16384) == 16384:
            pass
        frames = [(c, f) for _, c, f in rx.poll_frames(1 << 14)]
        assert len(frames) * steps == nframes, (len(frames), nframes)
    assert not feedback or nrows > 0 or nrec == 0, "records without feedback rows"
    return dt / steps * 1e3, h.hexdigest(), nrec, frames


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--tiles", type=int, default=16, help="4.2 MS tiles per push (bench.py's headline push: 16)")
    ap.add_argument("--bps", type=float, default=4.0, help="bursts per second and channel offered (bench.py's headline: 4)")
    ap.add_argument("--mode", default="both", choices=["both", "off", "on"])
    a = ap.parse_args()
    modes = {"both": (False, True), "off": (False,), "on": (True,)}[a.mode]
    tiles = [bench.make_tile(1234 + 1000 * v, "cs16", 2_000_000, synth.DEFAULT_FO_8CH, a.bps)[1] for v in range(4)]
    raw = np.concatenate([tiles[k % len(tiles)] for k in range(a.tiles)])
    batch = raw.size // 2
    dev = torch.from_numpy(raw).to("cuda:0")
    ms = {m: [] for m in modes}
    digest, frames = {}, {}
    for _ in range(a.rounds):
        for m in modes:
            t, d, n, fr = run(dev, batch, m, a.steps, a.warmup)
            ms[m].append(t)
            assert digest.setdefault(m, (d, n)) == (d, n), "a mode is not deterministic"
            frames[m] = fr
    res = {("feedback" if m else "plain"): {"ms_per_step": [round(x, 3) for x in ms[m]], "median": round(float(np.median(ms[m])), 3),
                                             "min": round(min(ms[m]), 3), "frames_per_step": len(frames[m])} for m in modes}
    if len(modes) == 2:
        res["records_identical"] = digest[False] == digest[True]
        res["plain_frames_kept"] = set(frames[False]) <= set(frames[True])
        res["bursts_per_step"] = digest[False][1] // a.steps
        res["added_pct_median"] = round(100 * (np.median(ms[True]) / np.median(ms[False]) - 1), 2)
        res["added_pct_min"] = round(100 * (min(ms[True]) / min(ms[False]) - 1), 2)
    print(json.dumps({f"headline_8ch_2MSps_cs16_frames_bps{a.bps:g}": res}), flush=True)
    if len(modes) == 2 and not (res["records_identical"] and res["plain_frames_kept"]):
        sys.exit("feedback_cost: the records differ between the modes, or a frame was lost")


if __name__ == "__main__":
    main()
