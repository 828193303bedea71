"""What VDL2GPU_F_BLOCK_REPORT costs: the headline workload (8 ch @ 2 MS/s cs16, device-resident samples, bench.py's recordings and
push size) with frames=True, without and with the flag, alternating x3.  Prints ms per step (median, min, max) and checks that the
burst records and the number of frames are identical between the two modes and that the reports' `frames` add up to the frames
collected.  For the block kernel's own time run it under rocprofv3 --kernel-trace --stats with --mode off / --mode on (one mode per
run: k4_frames against k4_frames_rep).

    python scripts/blockrep_cost.py [--steps 4] [--warmup 2] [--rounds 3] [--mode both|off|on]
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


def run(dev, batch, report, steps, warmup):
    buf = (lib.BurstT * 16384)()
    rv = (lib.BlockRepT * 16384)() if report else None
    fbuf = (lib.FrameT * 4096)()
    h = hashlib.sha256()
    nrec = nfr = nrep = 0
    with Receiver(2_000_000, plan_channels(bench.FC, synth.DEFAULT_FO_8CH), fmt="cs16", max_push=batch, max_bursts=1 << 18,
                  frames=True, block_report=report) as rx:
        def drain(timed):
            nonlocal nrec, nfr, nrep
            while True:
                n = rx.poll_report_raw(buf, None, None, None, rv, 16384)
                if timed:
                    h.update(C.string_at(C.addressof(buf), n * C.sizeof(lib.BurstT)))
                    nrec += n
                    if report:      # (one numpy sum: a Python loop over the records would be timed as the flag's cost)
                        nrep += int(np.frombuffer(rv, np.uint16).reshape(-1, C.sizeof(lib.BlockRepT) // 2)[:n, lib.BlockRepT.frames.offset // 2].sum())
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
    assert not report or nrep == nfr + dropped, f"the reports count {nrep} frames, {nfr} were collected and {dropped} dropped"
    return dt / steps * 1e3, h.hexdigest(), nrec, nfr


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
        sys.exit("blockrep_cost: needs a GPU (a timing taken anywhere else says nothing)")
    modes = {"both": (False, True), "off": (False,), "on": (True,)}[a.mode]
    tiles = [bench.make_tile(1234 + 1000 * v, "cs16", 2_000_000, synth.DEFAULT_FO_8CH, 4.0)[1] for v in range(4)]
    raw = np.concatenate([tiles[k % len(tiles)] for k in range(a.tiles)])
    batch = raw.size // 2
    dev = torch.from_numpy(raw).to("cuda:0")
    ms = {m: [] for m in modes}
    digest = {}
    for _ in range(a.rounds):           # alternating: a drift of the box falls on both
        for m in modes:
            t, d, n, f = run(dev, batch, m, a.steps, a.warmup)
            ms[m].append(t)
            assert digest.setdefault(m, (d, n, f)) == (d, n, f), "a mode is not deterministic"
    res = {("block_report" if m else "plain"): {"ms_per_step": [round(x, 3) for x in ms[m]], "median": round(float(np.median(ms[m])), 3),
                                                "min": round(min(ms[m]), 3), "max": round(max(ms[m]), 3)} for m in modes}
    if len(modes) == 2:
        res["records_and_frames_identical"] = digest[False] == digest[True]
        res["bursts_per_step"] = digest[False][1] // a.steps
        res["frames_per_step"] = digest[False][2] // a.steps
        res["added_pct_median"] = round(100 * (np.median(ms[True]) / np.median(ms[False]) - 1), 2)
    print(json.dumps({"headline_8ch_2MSps_cs16_frames": res}), flush=True)
    if len(modes) == 2 and not res["records_and_frames_identical"]:
        sys.exit("blockrep_cost: the records or the frames differ between the modes")


if __name__ == "__main__":
    main()
