"""What the rotation of VDL2GPU_F_EXACT_FO costs the channeliser: 8 channels of cs16 at 2 MS/s, device-resident input, every
channel 4100 Hz off the 25 kHz grid (30 ppm at 136.9 MHz), one push of --periods periods of the dump schedule (1 ms each) per
step.  The same build, the flag off and on in turn, three timed runs each (synchronous: push + poll), reported as median, min and
max of ms per push, and the channeliser's own time per push from vdl2gpu_get_timing in a fourth run with every push staged
(VDL2GPU_STAGE_EVERY=1), with the K1 kernels that ran (vdl2gpu_debug_k1).  Without the flag the mixer takes the reference's
jumping table of the same offsets: the same work but for the rotation.  With --pp the same on k1_pp (VDL2GPU_K1_PP).

    python scripts/exact_fo_cost.py [--periods 512] [--steps 6] [--warmup 2] [--pp]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vdlm2dec_amd import lib, synth  # noqa: E402
from vdlm2dec_amd.demod import Receiver, plan_channels  # noqa: E402

FC = 136_975_000
RATE = 2_000_000
FD = 4_100
TILE_PERIODS = 64


def _drain(rx, buf):
    n_all = 0
    while True:
        n = rx.poll_raw(buf, 16384)
        n_all += n
        if n < 16384:
            return n_all


def run(fos, flag, dev_ptr, n, steps, warmup, env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)          # the library reads its knobs when a handle is created
    try:
        buf = (lib.BurstT * 16384)()
        with Receiver(RATE, plan_channels(FC, fos), fmt="cs16", max_push=n, max_bursts=1 << 18, exact_fo=flag) as rx:
            for _ in range(warmup):
                rx.push_device(dev_ptr, n)
                _drain(rx, buf)
            rx.sync()
            rx.timing(reset=True)
            nrec = 0
            t0 = time.perf_counter()
            for _ in range(steps):
                rx.push_device(dev_ptr, n)
                nrec += _drain(rx, buf)
            rx.sync()
            dt = time.perf_counter() - t0
            tm, k1 = rx.timing(), rx.debug_k1()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return dt / steps, nrec // steps, tm, k1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--periods", type=int, default=512, help="periods of the dump schedule (1 ms of air time each) per push")
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--pp", action="store_true", help="k1_pp instead of k1_fast (VDL2GPU_K1_PP)")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("exact_fo_cost: needs a GPU (a timing taken anywhere else says nothing)")
    env = {"VDL2GPU_K1_PP": "1"} if a.pp else {}
    fos = [f + FD for f in synth.DEFAULT_FO_8CH]
    per = RATE // 1000
    tile = synth.synth_stream(synth.random_scenario(RATE, fos, TILE_PERIODS * per, seed=41, bursts_per_s=4.0, info_max=120), "cs16")
    n = a.periods * per
    raw = np.concatenate([tile] * ((a.periods + TILE_PERIODS - 1) // TILE_PERIODS))[:2 * n]
    dev = torch.from_numpy(raw).to("cuda:0")
    torch.cuda.synchronize()
    secs = {False: [], True: []}
    nrec = {}
    for _ in range(3):                  # alternating: a drift of the box falls on both
        for flag in (False, True):
            s, nrec[flag], _, _ = run(fos, flag, dev.data_ptr(), n, a.steps, a.warmup, env)
            secs[flag].append(s)
    for flag in (False, True):
        _, _, tm, k1 = run(fos, flag, dev.data_ptr(), n, a.steps, a.warmup, dict(env, VDL2GPU_STAGE_EVERY="1"))
        ms = sorted(s * 1e3 for s in secs[flag])
        print(json.dumps({"exact_fo": flag, "fd_hz": FD, "rate": RATE, "push_samples": n, "steps": a.steps,
                          "ms_per_push_median": round(ms[1], 3), "ms_per_push_min": round(ms[0], 3), "ms_per_push_max": round(ms[2], 3),
                          "channelise_ms_per_push": round(tm["channelise_ms"] / max(tm["pushes"], 1), 4),
                          "channelise_fast_ms_per_push": round(tm["channelise_fast_ms"] / max(tm["fast_pushes"], 1), 4),
                          "k1": k1, "bursts_per_push": nrec[flag]}), flush=True)


if __name__ == "__main__":
    main()
