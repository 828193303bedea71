"""What a sample format costs the channeliser and what it saves on the bus: the headline workload (8 ch @ 2 MS/s, bench.py's
recordings and push size) re-quantised per format from the SAME complex stream, for cu8, cs8, cs16, f32, s16, alternating formats
over --rounds rounds, in two legs:

    device   pushes of device-resident samples (the channeliser's own cost; ms per push, synchronous: push + poll)
    host     pushes from page-locked ingest-ring slots (the PCIe-inclusive rate; MS/s and host GB/s, as bench.py's host_ring)

One JSON line per format and leg with the rounds' values, median, min and max.  Formats the library does not know (lib.FMT) are
skipped, so the same script measures the siblings on an older tree.  The real formats (f32, s16) see the real part of the stream:
their burst count differs from the complex formats', compare them with each other.  For k1_fast's own time run one format and
leg under rocprofv3 --kernel-trace --stats:  --fmts s16 --legs device --rounds 1.

    python scripts/fmt_cost.py [--steps 6] [--warmup 3] [--rounds 3] [--tiles 16] [--fmts cu8,cs8,...] [--legs device,host]
"""
import argparse
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

RATE = 2_000_000
ALL = ["cu8", "cs8", "cs16", "f32", "s16"]


def _drain(rx, buf, ready=False):
    n_all = 0
    while True:
        n = rx.poll_ready_raw(buf, 16384) if ready else rx.poll_raw(buf, 16384)
        n_all += n
        if n < 16384:
            return n_all


def _rx(fmt, batch):
    return Receiver(RATE, plan_channels(bench.FC, synth.DEFAULT_FO_8CH), fmt=fmt, max_push=batch, max_bursts=1 << 18)


def device_leg(fmt, raw, batch, steps, warmup):
    import torch
    buf = (lib.BurstT * 16384)()
    dev = torch.from_numpy(raw.view(np.uint8)).to("cuda:0")
    torch.cuda.synchronize()
    with _rx(fmt, batch) as rx:
        for _ in range(warmup):
            rx.push_device(dev.data_ptr(), batch)
            _drain(rx, buf)
        rx.sync()
        nrec = 0
        t0 = time.perf_counter()
        for _ in range(steps):
            rx.push_device(dev.data_ptr(), batch)
            nrec += _drain(rx, buf)
        rx.sync()
        dt = time.perf_counter() - t0
    del dev
    return dt / steps * 1e3, nrec // steps


def host_leg(fmt, raw, batch, steps, warmup):
    buf = (lib.BurstT * 16384)()
    rawb = raw.view(np.uint8).reshape(1, -1)
    with _rx(fmt, batch) as rx:
        rx.ring_init(batch, nslots=3)
        nb = batch * rx.sample_bytes
        for _ in range(max(3, warmup)):                 # every slot holds the recording from here on
            slot = rx.ring_acquire()
            slot[:, :nb] = rawb[:, :nb]
            rx.ring_commit(batch)
        _drain(rx, buf)
        rx.sync()
        t0 = time.perf_counter()
        for _ in range(steps):
            rx.ring_acquire()
            rx.ring_commit(batch)
            _drain(rx, buf, ready=True)
        _drain(rx, buf)
        rx.sync()
        dt = time.perf_counter() - t0
        nb_s = rx.sample_bytes
    return steps * batch / dt / 1e6, steps * batch * nb_s / dt / 1e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--tiles", type=int, default=16, help="4.2 MS tiles per push (bench.py's headline push: 16)")
    ap.add_argument("--fmts", default=",".join(ALL))
    ap.add_argument("--legs", default="device,host")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("fmt_cost: needs a GPU (a timing taken anywhere else says nothing)")
    fmts = [f for f in a.fmts.split(",") if f in lib.FMT]
    skipped = [f for f in a.fmts.split(",") if f not in lib.FMT]
    legs = a.legs.split(",")
    # bench.make_tile's scenarios, kept complex: every format is a quantisation of the same stream
    tiles = [synth.synth_complex(synth.random_scenario(RATE, synth.DEFAULT_FO_8CH, bench.TILE, seed=1234 + 1000 * v, bursts_per_s=4.0,
                                                       info_max=240)) for v in range(4)]
    batch = a.tiles * bench.TILE
    raws = {}
    for f in fmts:
        q = [synth.quantise(t, f) for t in tiles]
        raws[f] = np.concatenate([q[k % len(q)] for k in range(a.tiles)])
    del tiles
    res = {(f, leg): [] for f in fmts for leg in legs}
    bursts = {}
    for _ in range(a.rounds):
        for f in fmts:
            if "device" in legs:
                ms, n = device_leg(f, raws[f], batch, a.steps, a.warmup)
                res[(f, "device")].append(ms)
                assert bursts.setdefault(f, n) == n, "a format is not deterministic"
            if "host" in legs:
                res[(f, "host")].append(host_leg(f, raws[f], batch, a.steps, a.warmup))
    for f in fmts:
        for leg in legs:
            v = res[(f, leg)]
            if leg == "device":
                out = {"unit": "ms_per_push", "values": [round(t, 3) for t in v], "median": round(float(np.median(v)), 3),
                       "min": round(min(v), 3), "max": round(max(v), 3), "MSps_median": round(batch / float(np.median(v)) / 1e3, 1),
                       "bursts_per_push": bursts[f]}
            else:
                r, g = [p[0] for p in v], [p[1] for p in v]
                out = {"unit": "MS/s", "values": [round(t, 1) for t in r], "median": round(float(np.median(r)), 1), "min": round(min(r), 1),
                       "max": round(max(r), 1), "host_GBps_median": round(float(np.median(g)), 2)}
            print(json.dumps({"fmt": f, "leg": leg, "bytes_per_sample": lib.SAMPLE_BYTES[f], "push_samples": batch, "steps": a.steps,
                              **out}), flush=True)
    if skipped:
        print(json.dumps({"skipped": skipped, "why": "not in lib.FMT of this tree"}), flush=True)


if __name__ == "__main__":
    main()
