"""What VDL2GPU_F_TRACKED costs: the headline workload (8 ch @ 2 MS/s cs16, device-resident samples, bench.py's recordings and push
size) with the block path in the pipeline (frames), without and with the flag, alternating x3.  Prints ms per step (median, min, max)
and checks that the burst records are identical between the two modes and that every record of the flagged runs carries a column
(nseg > 0).  For the kernels' own time run it under rocprofv3 --kernel-trace --stats with --mode on (k_tracked_rows,
k_export_tracked, k4_frames_trk).

    python scripts/tracked_cost.py [--steps 4] [--warmup 2] [--rounds 3] [--mode both|off|on]
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


def run(dev, batch, on, steps, warmup):
    buf = (lib.BurstT * 16384)()
    tv = (lib.TrkT * 16384)() if on else None
    h = hashlib.sha256()
    nrec = ncol = 0
    with Receiver(2_000_000, plan_channels(bench.FC, synth.DEFAULT_FO_8CH), fmt="cs16", max_push=batch, max_bursts=1 << 18,
                  frames=True, tracked=on) as rx:
        def drain(timed):
            nonlocal nrec, ncol
            while True:
                n = rx.poll_tracked_raw(buf, None, None, None, None, None, None, tv, 16384)
                if timed:
                    h.update(C.string_at(C.addressof(buf), n * C.sizeof(lib.BurstT)))
                    nrec += n
                    if on:      # (one numpy reduction: a Python loop over the records would be timed as the flag's cost)
                        ncol += int((np.frombuffer(tv, np.uint8).reshape(-1, C.sizeof(lib.TrkT))[:n, lib.TrkT.nseg.offset] > 0).sum())
                if n < 16384:
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
    assert not on or ncol == nrec, f"{ncol} of {nrec} records carry a column"
    return dt / steps * 1e3, h.hexdigest(), nrec


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--tiles", type=int, default=16, help="4.2 MS tiles per push (bench.py's headline push: 16)")
    ap.add_argument("--mode", default="both", choices=["both", "off", "on"])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tracked_cost: needs a GPU (a timing taken anywhere else says nothing)")
    modes = {"both": (False, True), "off": (False,), "on": (True,)}[a.mode]
    tiles = [bench.make_tile(1234 + 1000 * v, "cs16", 2_000_000, synth.DEFAULT_FO_8CH, 4.0)[1] for v in range(4)]
    raw = np.concatenate([tiles[k % len(tiles)] for k in range(a.tiles)])
    batch = raw.size // 2
    dev = torch.from_numpy(raw).to("cuda:0")
    ms = {m: [] for m in modes}
    digest = {}
    for _ in range(a.rounds):           # alternating: a drift of the box falls on both
        for m in modes:
            t, d, n = run(dev, batch, m, a.steps, a.warmup)
            ms[m].append(t)
            assert digest.setdefault(m, (d, n)) == (d, n), "a mode is not deterministic"
    res = {("tracked" if m else "frames"): {"ms_per_step": [round(x, 3) for x in ms[m]], "median": round(float(np.median(ms[m])), 3),
                                          "min": round(min(ms[m]), 3), "max": round(max(ms[m]), 3)} for m in modes}
    if len(modes) == 2:
        res["records_identical"] = digest[False] == digest[True]
        res["bursts_per_step"] = digest[False][1] // a.steps
        res["added_pct_median"] = round(100 * (np.median(ms[True]) / np.median(ms[False]) - 1), 2)
    print(json.dumps({"headline_8ch_2MSps_cs16": res}), flush=True)
    if len(modes) == 2 and not res["records_identical"]:
        sys.exit("tracked_cost: the records differ between the modes")


if __name__ == "__main__":
    main()
