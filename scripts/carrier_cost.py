"""What VDL2GPU_F_CARRIER costs: the headline workload (8 ch @ 2 MS/s cs16, device-resident samples, bench.py's recordings and push
size) and the busy-30 one (30 bursts/s/channel offered), each without and with the flag, alternating x3.  Prints ms per step and
checks that the burst records are byte-identical between the two modes and that every carrier record holds sums.  For the payload
kernel's own time run it under rocprofv3 --kernel-trace --stats with --mode off / --mode on (one mode per run).

    python scripts/carrier_cost.py [--steps 4] [--warmup 2] [--rounds 3] [--mode both|off|on]
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


def run(dev, batch, carrier, steps, warmup):
    buf = (lib.BurstT * 16384)()
    cv = (lib.CarrierT * 16384)() if carrier else None
    h = hashlib.sha256()
    nrec = nsym = 0
    with Receiver(2_000_000, plan_channels(bench.FC, synth.DEFAULT_FO_8CH), fmt="cs16", max_push=batch, max_bursts=1 << 18,
                  carrier=carrier) as rx:
        def drain(timed):
            nonlocal nrec, nsym
            while True:
                n = rx.poll_carrier_raw(buf, None, None, cv, 16384)
                if timed:
                    h.update(C.string_at(C.addressof(buf), n * C.sizeof(lib.BurstT)))
                    nrec += n
                    if carrier:
                        nsym += sum(cv[i].nsym for i in range(n))
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
    assert not carrier or nsym > 0 or nrec == 0, "carrier records without sums"
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
    modes = {"both": (False, True), "off": (False,), "on": (True,)}[a.mode]
    out = {}
    for name, bps in (("headline_8ch_2MSps_cs16", 4.0), ("busy_30", 30.0)):
        tiles = [bench.make_tile(1234 + 1000 * v, "cs16", 2_000_000, synth.DEFAULT_FO_8CH, bps)[1] for v in range(4)]
        raw = np.concatenate([tiles[k % len(tiles)] for k in range(a.tiles)])
        batch = raw.size // 2
        dev = torch.from_numpy(raw).to("cuda:0")
        ms = {m: [] for m in modes}
        digest = {}
        for _ in range(a.rounds):
            for m in modes:
                t, d, n = run(dev, batch, m, a.steps, a.warmup)
                ms[m].append(t)
                assert digest.setdefault(m, (d, n)) == (d, n), "a mode is not deterministic"
        res = {("carrier" if m else "plain"): {"ms_per_step": [round(x, 2) for x in ms[m]], "median": round(float(np.median(ms[m])), 2),
                                                "min": round(min(ms[m]), 2)} for m in modes}
        if len(modes) == 2:
            res["records_identical"] = digest[False] == digest[True]
            res["bursts_per_step"] = digest[False][1] // a.steps
            res["added_pct_median"] = round(100 * (np.median(ms[True]) / np.median(ms[False]) - 1), 2)
            res["added_pct_min"] = round(100 * (min(ms[True]) / min(ms[False]) - 1), 2)
        out[name] = res
        print(json.dumps({name: res}), flush=True)
        del dev
    if len(modes) == 2 and not all(v["records_identical"] for v in out.values()):
        sys.exit("carrier_cost: the records differ between the modes")


if __name__ == "__main__":
    main()
