"""What VDL2GPU_F_RAW_FLAGS costs and what it is worth, against VDL2GPU_F_ALL_FRAMES alone in the same run: the headline workload (8 ch @
2 MS/s cs16, device-resident samples, bench.py's recordings and push size) with frames=True, all_frames and all_frames + raw_flags
alternating x3.  Prints ms per step (median, min, max) and the frames collected per step in both modes, and checks that the burst records
are identical between the two.  --frames-per-burst N puts N AVLC frames into every burst of the recordings, as in allframes_cost.py.  For
the block kernel's own time run it under rocprofv3 --kernel-trace --stats with --mode all / --mode raw (one mode per run: k4_frames_all
against k4_frames_raw).

    python scripts/rawflags_cost.py [--steps 4] [--warmup 2] [--rounds 3] [--mode both|all|raw] [--frames-per-burst 1]
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


def run(dev, batch, raw_flags, steps, warmup):
    """allframes_cost.run with all_frames=True and raw_flags as given"""
    buf = (lib.BurstT * 16384)()
    fbuf = (lib.FrameT * 4096)()
    h = hashlib.sha256()
    nrec = nfr = 0
    with Receiver(2_000_000, plan_channels(bench.FC, synth.DEFAULT_FO_8CH), fmt="cs16", max_push=batch, max_bursts=1 << 18,
                  frames=True, all_frames=True, raw_flags=raw_flags) as rx:
        def drain(timed):
            nonlocal nrec, nfr
            while True:
                n = rx.poll_raw(buf, 16384)
                if timed:
                    h.update(C.string_at(C.addressof(buf), n * C.sizeof(lib.BurstT)))
                    nrec += n
                if n < 16384:
                    break
            while True:
                m = rx._check(rx.L.vdl2gpu_poll_frames(rx.h, fbuf, 4096))
                nfr += m if timed else 0
                if m < 4096:
                    return
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
        dropped = rx.stats()["frames_dropped"]
    return dt / steps * 1e3, h.hexdigest(), nrec, nfr, dropped


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--tiles", type=int, default=16, help="4.2 MS tiles per push (bench.py's headline push: 16)")
    ap.add_argument("--mode", default="both", choices=["both", "all", "raw"])
    ap.add_argument("--frames-per-burst", type=int, default=1, help="AVLC frames in every burst of the recordings (1: bench.py's own)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("rawflags_cost: needs a GPU (a timing taken anywhere else says nothing)")
    modes = {"both": (False, True), "all": (False,), "raw": (True,)}[a.mode]
    if a.frames_per_burst == 1:
        tiles = [bench.make_tile(1234 + 1000 * v, "cs16", 2_000_000, synth.DEFAULT_FO_8CH, 4.0)[1] for v in range(4)]
    else:
        tiles = [synth.synth_stream(synth.random_scenario(2_000_000, synth.DEFAULT_FO_8CH, bench.TILE, seed=1234 + 1000 * v, bursts_per_s=4.0,
                                                          info_max=240, frames_per_burst=a.frames_per_burst), "cs16") for v in range(4)]
    raw = np.concatenate([tiles[k % len(tiles)] for k in range(a.tiles)])
    batch = raw.size // 2
    dev = torch.from_numpy(raw).to("cuda:0")
    ms = {m: [] for m in modes}
    digest = {}
    for _ in range(a.rounds):           # alternating: a drift of the box falls on both
        for m in modes:
            t, d, n, f, dr = run(dev, batch, m, a.steps, a.warmup)
            ms[m].append(t)
            assert digest.setdefault(m, (d, n, f, dr)) == (d, n, f, dr), "a mode is not deterministic"
    res = {("all_frames+raw_flags" if m else "all_frames"): {"ms_per_step": [round(x, 3) for x in ms[m]], "median": round(float(np.median(ms[m])), 3),
                                                             "min": round(min(ms[m]), 3), "max": round(max(ms[m]), 3),
                                                             "frames_per_step": digest[m][2] // a.steps, "frames_dropped": digest[m][3]} for m in modes}
    res["frames_per_burst_sent"] = a.frames_per_burst
    res["bursts_per_step"] = digest[modes[0]][1] // a.steps
    if len(modes) == 2:
        res["records_identical"] = digest[False][:2] == digest[True][:2]
        res["added_pct_median"] = round(100 * (np.median(ms[True]) / np.median(ms[False]) - 1), 2)
    print(json.dumps({"headline_8ch_2MSps_cs16_frames": res}), flush=True)
    if len(modes) == 2 and not res["records_identical"]:
        sys.exit("rawflags_cost: the burst records differ between the modes")


if __name__ == "__main__":
    main()
