"""What the sample rate costs the channeliser: 8 channels of cs16, device-resident input, one push of --periods periods of the
dump schedule (1 ms each) per step, at the rates off the 25 kHz grid (2.048, 7.68, 15.36, 30.72 MS/s) and, for comparison on the
same box and run, at 2 MS/s (k1_fast), 2 MS/s forced onto k1_pp (VDL2GPU_K1_PP) and 10 MS/s.  Per case three timed runs
(synchronous: push + poll), reported as median, min and max of the rate in GS/s, and the channeliser's own time per push from
vdl2gpu_get_timing in a fourth run with every push staged (VDL2GPU_STAGE_EVERY=1).  With --general the same through the general
kernel alone (VDL2GPU_NO_K1_FAST: the table in LDS up to 7.68 MS/s, in global memory at 15.36 and 30.72 MS/s).

    python scripts/rate_cost.py [--periods 512] [--steps 6] [--warmup 2] [--general]
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
CASES = [("2.048", 2_048_000, {}), ("7.68", 7_680_000, {}), ("15.36", 15_360_000, {}), ("30.72", 30_720_000, {}),
         ("2.0 k1_fast", 2_000_000, {}), ("2.0 k1_pp", 2_000_000, {"VDL2GPU_K1_PP": "1"}), ("10.0", 10_000_000, {})]
TILE_PERIODS = 64


def _fos(rate):
    return [int(f * rate / 2_000_000) // 25000 * 25000 for f in synth.DEFAULT_FO_8CH]


def _drain(rx, buf):
    n_all = 0
    while True:
        n = rx.poll_raw(buf, 16384)
        n_all += n
        if n < 16384:
            return n_all


def run(rate, dev_ptr, n, steps, warmup, env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)          # the library reads its knobs when a handle is created
    try:
        buf = (lib.BurstT * 16384)()
        with Receiver(rate, plan_channels(FC, _fos(rate)), fmt="cs16", max_push=n, max_bursts=1 << 18) as rx:
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
            tm = rx.timing()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return dt / steps, nrec // steps, tm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--periods", type=int, default=512, help="periods of the dump schedule (1 ms of air time each) per push")
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--general", action="store_true", help="the general kernel alone (VDL2GPU_NO_K1_FAST)")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("rate_cost: needs a GPU (a timing taken anywhere else says nothing)")
    for name, rate, env in CASES:
        if a.general and env:
            continue
        env = dict(env, **({"VDL2GPU_NO_K1_FAST": "1"} if a.general else {}))
        per = rate // 1000
        tile = synth.synth_stream(synth.random_scenario(rate, _fos(rate), TILE_PERIODS * per, seed=rate // 1000, bursts_per_s=4.0,
                                                        info_max=120), "cs16")
        n = a.periods * per
        raw = np.concatenate([tile] * ((a.periods + TILE_PERIODS - 1) // TILE_PERIODS))[:2 * n]
        dev = torch.from_numpy(raw).to("cuda:0")
        torch.cuda.synchronize()
        secs, nrec = [], None
        for _ in range(3):
            s, nrec, _ = run(rate, dev.data_ptr(), n, a.steps, a.warmup, env)
            secs.append(s)
        _, _, tm = run(rate, dev.data_ptr(), n, a.steps, a.warmup, dict(env, VDL2GPU_STAGE_EVERY="1"))
        gs = sorted(n / s / 1e9 for s in secs)
        print(json.dumps({"case": name + (" general" if a.general else ""), "rate": rate, "lo_len": lib.load().vdl2gpu_lo_len(rate),
                          "push_samples": n, "steps": a.steps, "GSps_median": round(gs[1], 3), "GSps_min": round(gs[0], 3),
                          "GSps_max": round(gs[2], 3), "ms_per_push_median": round(sorted(secs)[1] * 1e3, 3),
                          "channelise_ms_per_push": round(tm["channelise_ms"] / max(tm["pushes"], 1), 3),
                          "fast_pushes": tm["fast_pushes"], "bursts_per_push": nrec}), flush=True)
        del dev


if __name__ == "__main__":
    main()
