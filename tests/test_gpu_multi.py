"""N > 1 on real GPUs.  The driver's box has one GPU: the two-device test skips there, the launcher test
does not (it checks that `bench.py --gpus N` refuses to run N ranks on fewer than N devices instead of silently
running one)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import scenarios as S
from vdlm2dec_amd import shard, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_refuses_more_ranks_than_gpus(built):
    import torch
    n = torch.cuda.device_count() + 1
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--steps", "1", "--warmup", "0"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert "GPU(s) visible" in (r.stderr + r.stdout)


def test_two_receivers_on_two_devices_equal_one(built, oracle):
    """Streams sharded over two devices (one Receiver each, vdlm2dec_amd.shard partition) decode to the same records as
    all streams on one device and as the oracle."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    from vdlm2dec_amd.demod import Receiver, plan_channels
    nstreams = 3
    specs = [S.eight_channels(seed=800 + i, dur=0.05, info=(3, 9, 5, 12, 7, 4, 6, 8)) for i in range(nstreams)]
    raws = [synth.synth_stream(sp, "cs16") for sp in specs]
    fos = specs[0].fo

    def decode(dev, idx):
        if not len(idx):
            return np.zeros(0, shard.REC_DTYPE)
        with Receiver(specs[0].rate, [plan_channels(S.FC, fos)] * len(idx), fmt="cs16", max_push=specs[0].nsamples, device=dev) as rx:
            rx.push(np.stack([raws[i] for i in idx]))
            return shard.pack_bursts(rx.poll(), stream_offset=idx.start)

    parts = [decode(r, shard.shard_streams(nstreams, r, 2)) for r in range(2)]
    both = np.concatenate(parts)
    one = decode(0, range(nstreams))
    assert shard.digest(both) == shard.digest(one)
    nwant = sum(len(oracle.run_oracle(raws[s], "cs16", specs[s].rate, fos, S.FC)) for s in range(nstreams))
    assert len(both) == nwant >= 6


def _bench_line(argv, timeout=900):
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + argv, capture_output=True, text=True, timeout=timeout, env=env)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    import json
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_bench_multi_rank_path_on_one_gpu(built, tmp_path):
    """The WHOLE N > 1 path of bench.py on the one GPU a box has: `--gpus 2 --backend gloo --share-gpu` respawns itself as two
    ranks (python -m torch.distributed.run, 127.0.0.1), each with a real Receiver on cuda:0 over its shard of the streams
    (RCCL refuses two ranks on one device: gloo carries the barrier, the verdicts and the gather -- the same shard.run_sharded
    code).  Every rank's bursts are checked against the oracle inside bench.py (verdicts MIN-reduced); here: the gathered
    records on rank 0 are the records ONE process decodes from the same two streams, their digest of digests is what
    shard.combined_digest() says a two-rank run must produce, and the 512-channel leg (8 streams per rank) ran across both."""
    tiles, steps, warmup = 2, 3, 1
    common = ["--steps", str(steps), "--warmup", str(warmup), "--tiles", str(tiles), "--full", "--no-cpu", "--no-ring"]
    g2 = str(tmp_path / "g2.npy")
    two = _bench_line(["--gpus", "2", "--backend", "gloo", "--share-gpu", "--gather-out", g2] + common)
    assert two["n_gpus"] == 2 and two["value"] and two["parity"]["equal"]
    assert "2 x configs[1]" in two["config"]["workload"] and "1xMI355X" not in two["config"]["workload"]
    assert two["gather"]["ranks_share_one_gpu"] and two["gather"]["backend"] == "gloo" and len(two["gather"]["per_rank"]) == 2
    leg = two["configs"]["config4_512ch"]
    assert leg["parity"]["equal"] and leg["value"] and leg["streams"] == 16 and leg["channels"] == 128
    assert len(leg["gather"]["per_rank"]) == 2 and min(leg["gather"]["per_rank"]) > 0 and leg["gather"]["digest_of_rank_digests"]
    g1 = str(tmp_path / "g1.npy")
    one = _bench_line(["--gpus", "1", "--streams", "2", "--gather-out", g1, "--no-extra"] + common)
    assert one["parity"]["equal"]
    a, b = np.load(g2), np.load(g1)
    # the tiles wholly inside both timed regions (a burst that is open when a run's last push ends comes with the next push)
    tile_dec = 4_200_000 * 21 // 500
    lo, hi = warmup * tiles, (warmup + steps) * tiles - 1
    sel = lambda r: r[(r["trig_dec"] // tile_dec >= lo) & (r["trig_dec"] // tile_dec < hi)]
    a, b = sel(a), sel(b)
    assert len(a) > 50 and shard.digest(a) == shard.digest(b)
    assert set(np.unique(a["stream"])) == {0, 1}
    full = np.load(g2)
    assert shard.combined_digest(full, 2, 2).hex()[:16] == two["gather"]["digest_of_rank_digests"]
