"""bench.py's CPU legs (no GPU): the reference-kind baseline runs the prebuilt real reference, the port-kind one the
oracle; both must see the same traffic."""
import os
import sys

import numpy as np
import pytest

import scenarios as S
from vdlm2dec_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


@pytest.fixture(scope="module")
def tile():
    spec = synth.random_scenario(2_000_000, S.FO8[:3], 1_050_000, seed=3, bursts_per_s=8.0, info_max=120)
    return spec, synth.synth_stream(spec, "cs16")


def test_port_baseline(oracle, tile):
    import bench
    spec, raw = tile
    r = bench.cpu_baseline(raw, "cs16", spec.fo, spec.rate, budget_s=0.5)
    assert r["kind"] == "port" and r["value"] > 1.0 and r["cores"] == 3 and r["unit"] == "MS/s"


def test_reference_baseline(oracle, tile):
    import bench
    if not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "ref_rtl")):
        pytest.skip("the real reference is built only where /root/reference exists")
    spec, raw = tile
    r = bench.cpu_baseline_reference(raw, "cs16", spec.fo, spec.rate, budget_s=0.5)
    assert r is not None and r["kind"] == "reference" and r["value"] > 1.0 and r["cores"] == 4
    assert "oracle/_ref/ref_rtl" in r["sample"]
    assert bench.cpu_baseline_reference(raw, "nosuchformat", spec.fo, spec.rate) is None


def test_share_gpu_needs_gloo():
    """`--share-gpu` (two ranks on cuda:0: the N > 1 path on a one-GPU box) is only accepted with `--backend gloo`: RCCL
    refuses two ranks on one device, and the refusal must come from bench.py's argument check, not from a hang in init."""
    import subprocess
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--share-gpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--backend gloo" in (r.stderr + r.stdout)


def test_dropin_replay_without_a_gpu_reports_an_error_not_a_number(tile, tmp_path):
    """bench.py's `dropin_replay` leg runs oracle/_ref/ref_rtl_gpu; where there is no GPU the shim's vdl2gpu_create() fails
    (there is no CPU fallback) and the leg must say so instead of producing a figure."""
    import bench
    if not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "ref_rtl_gpu")):
        pytest.skip("the drop-in executable is built only where /root/reference exists")
    try:
        import torch
        if torch.cuda.is_available():
            pytest.skip("a GPU is present")
    except ImportError:
        pass
    spec, raw = tile
    path = str(tmp_path / "iq.bin")
    raw.tofile(path)
    fo = ",".join(str(int(x)) for x in spec.fo)
    fr = ",".join(str(int(bench.FC + x)) for x in spec.fo)
    r = bench._dropin_replay(ROOT, str(tmp_path), path, "cs16", spec.rate, fo, fr, raw.size // 2)
    assert r is None or ("error" in r and "value" not in r)


def test_dump_outputs_writes_the_last_step_as_float_arrays(tmp_path):
    """--dump-outputs: the records whose instant lies in the given tiles, in canonical order, one float .npy per field;
    above the size bound a fixed, seeded sample of them (the same one every time)."""
    import bench
    from vdlm2dec_amd import shard
    tile_dec = 1000
    rng = np.random.default_rng(5)
    recs = np.zeros(400, shard.REC_DTYPE)
    recs["stream"] = rng.integers(0, 2, len(recs))
    recs["chn"] = rng.integers(0, 8, len(recs))
    recs["trig_dec"] = rng.permutation(np.arange(len(recs)) * 37)
    recs["end_dec"] = recs["trig_dec"] + 500
    recs["nbrow"] = 3
    recs["df_bits"] = np.float32(-1.5).view(np.uint32)
    recs["data"] = rng.integers(0, 256, recs["data"].shape)
    lo, hi = 5, 9
    want = recs[(recs["trig_dec"] >= lo * tile_dec) & (recs["trig_dec"] < hi * tile_dec)]
    want = want[np.lexsort((want["trig_dec"], want["chn"], want["stream"]))]
    d = tmp_path / "out"
    bench.dump_outputs(str(d), recs, lo, hi, tile_dec)
    got = {p.stem: np.load(p) for p in d.glob("*.npy")}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert got["bursts_total"][0] == len(want) > 50
    assert np.array_equal(got["bursts_trig_dec"], want["trig_dec"]) and np.array_equal(got["bursts_chn"], want["chn"])
    assert np.array_equal(got["bursts_data"], want["data"].astype(np.float32)) and np.all(got["bursts_df"] == -1.5)
    assert sum(p.stat().st_size for p in d.glob("*.npy")) <= bench.DUMP_BYTES
    # a bound below the step's size: a sample, the same one on every call, still in canonical order
    old = bench.DUMP_BYTES
    try:
        bench.DUMP_BYTES = 4096 + 20 * (6 * 8 + 4 + 2040 * 4)
        for k in ("a", "b"):
            bench.dump_outputs(str(tmp_path / k), recs, lo, hi, tile_dec)
    finally:
        bench.DUMP_BYTES = old
    a, b = (np.load(tmp_path / k / "bursts_trig_dec.npy") for k in ("a", "b"))
    assert len(a) == 20 and np.array_equal(a, b) and np.all(np.isin(a, want["trig_dec"]))
    assert np.load(tmp_path / "a" / "bursts_total.npy")[0] == len(want)
