"""Every row of the payload kernel list (K2D_PAYLOAD_KERNELS, vdl2gpu_resolve.h) launched once: sixteen receivers, one per subset of
{levels, soft_rs, carrier, feedback}, on the recording of smoke() -- 2 channels, cu8, 2 MS/s, three bursts of 5, 40 and 120 information
bytes, one push.  In every receiver the bursts are the oracle's, every column that is on equals the same burst's column of the receiver
with all four on bit for bit, and every column that is off is None.  Once on the default path and once with serial=True (k2f_commit or
k2f_commit_fb, and mach_commit_trigger's four passes).  What the all-on receiver's columns must BE is held by the per-feature tests
(test_gpu_levels, test_gpu_soft, test_gpu_carrier, test_gpu_feedback)."""
import dataclasses
import itertools
import struct

import numpy as np
import pytest

from vdlm2dec_amd import synth

pytestmark = pytest.mark.gpu

RATE, FC, FO = 2_000_000, 136_975_000, [-50_000, 250_000]
COLUMNS = (("levels", "level"), ("soft_rs", "soft"), ("carrier", "carrier"), ("feedback", "fb"))     # Receiver keyword, Burst field
_cache = {}


def _recording(oracle):
    """(raw, the oracle's sorted burst keys): computed once"""
    if "rec" not in _cache:
        rng = np.random.default_rng(11)
        bursts, t = [], 0.002
        for i, n in enumerate((5, 40, 120)):
            b = synth.Burst(chan=i % 2, t0=t, info=bytes(rng.integers(0, 256, n, dtype=np.uint8).tolist()),
                            amp=float(rng.uniform(10, 50)), cfo=float(rng.uniform(-300, 300)))
            bursts.append(b)
            t += b.duration() + 0.002
        ns = (int((t + 0.004) * RATE) + 32767) // 32768 * 32768
        raw = synth.synth_stream(synth.StreamSpec(rate=RATE, fo=FO, nsamples=ns, bursts=bursts, seed=2), "cu8")
        want = sorted(b.key() for b in oracle.run_oracle(raw, "cu8", RATE, FO, FC))
        assert len(want) == 3
        _cache["rec"] = (raw, ns, want)
    return _cache["rec"]


def _bits(v):
    """a column's value as something that compares bit for bit"""
    if v is None:
        return None
    if isinstance(v, np.ndarray):
        return (v.dtype.str, v.shape, v.tobytes())
    return tuple(struct.pack("<d", x) if isinstance(x, float) else x for x in dataclasses.astuple(v))


@pytest.mark.parametrize("serial", (False, True), ids=("default", "serial"))
def test_every_set_of_columns(built, oracle, serial):
    from vdlm2dec_amd.demod import Receiver, plan_channels
    raw, ns, want = _recording(oracle)
    got = {}
    for on in itertools.product((False, True), repeat=len(COLUMNS)):
        with Receiver(RATE, plan_channels(FC, FO), fmt="cu8", max_push=ns, serial=serial,
                      **{kw: o for (kw, _), o in zip(COLUMNS, on)}) as rx:
            rx.push(raw)
            got[on] = rx.poll()
    assert len(got) == 16
    full = {(b.chn, b.trig_dec): b for b in got[(True,) * len(COLUMNS)]}
    assert len(full) == 3
    for on, bursts in got.items():
        assert sorted((b.chn, b.nbrow, b.nlbyte, b.data) for b in bursts) == want, on
        for b in bursts:
            ref = full[(b.chn, b.trig_dec)]
            assert b.report is None
            for (_, field), o in zip(COLUMNS, on):
                v = getattr(b, field)
                if o:
                    assert v is not None and _bits(v) == _bits(getattr(ref, field)), (on, field, b.chn, b.trig_dec)
                else:
                    assert v is None, (on, field)
