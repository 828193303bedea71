"""The back stage's list limits, and what happens when each is full: regions, verify stretches, the resolver's visited list, the windows,
merge and serial-stretch log of a local repair, and the dynamic tail of the descriptor pool.  With ordinary inputs none of them is reached
before VDL2_CAND_CAP overflows and takes the channel to the serial machine, so the test library lowers each at run time
(VDL2GPU_TEST_*_CAP, VDL2GPU_TEST_STAGE_DYN: csrc/vdl2gpu_types.h, K2_*_LIM) and counts how often the branch behind it was taken
(development counters 64 .. 70, 75, 76).  Beside them it counts violations of the two invariants the windows of a local repair stand on
(71 .. 74, at CTL_NWIN0; 77 .. 80: how often each check was made): those read zero in every run here.

The rig is the exact identity of tests/test_gpu_planes.py; the planes are geom_craft's `geom` and chain_craft's families, which the oracle
judges once per process.  Every case runs twice -- hook set, hook unset -- and both give the oracle's records; the escape counter is
positive in the first and zero in the second.  One case per limit runs with frames, levels, reliability maps and carrier sums: the
side columns are verified once per plane against their CPU models (levels_ref, soft_ref / geom_craft.soft_maps, carrier_ref) and every
later run must reproduce those bit for bit.

Also here: the repair schedules of production handles (one round; three rounds with the middle k2s_merge + k2c_resolve round) on the
crafted chain and geometry planes, which tests/test_gpu_planes.PATHS runs with none and with two rounds only."""
import types

import numpy as np
import pytest

import carrier_ref as CR
import chain_craft as CC
import geom_craft as G
import plane_craft as PC
import test_gpu_carrier as TCAR
import test_gpu_chain as TC
import test_gpu_geometry as TG
import test_gpu_levels as TL
import test_gpu_rates as TR
from test_gpu_chain import PART, _env, _push_parts
from test_gpu_planes import _bits, _rx
from vdlm2dec_amd import lib

pytestmark = pytest.mark.gpu

NDBG = lib.DBG_WORDS_TEST       # VDL2_DBG_WORDS of the test library
REPAIRED = lib.DBG["REPAIRED"]  # channel-pushes that went through a repair round (k2_begin_repair)
ESC = {"REG_CAP": lib.DBG["ESC_REG"], "SEG_CAP": lib.DBG["ESC_SEG"], "VIS_CAP": lib.DBG["ESC_VIS"], "WIN_CAP": lib.DBG["ESC_WIN"],
       "MERGE_CAP": lib.DBG["ESC_MERGE"], "SLOG_CAP": lib.DBG["ESC_SLOG"], "STAGE_DYN": lib.DBG["ESC_STAGE"]}
# (b) k2b_clusters, (b) k2d_run's descriptors, (b) k2d_run's records, (a) k2p_patch
INVARIANTS = tuple(lib.DBG[k] for k in ("INV_B_CLUSTER", "INV_B_DECODE", "INV_B_RECORD", "INV_A"))
MERGE_SORT = lib.DBG["ESC_MERGE_SORT"]          # the merge escapes of k2s_merge alone
ABANDONED = lib.DBG["ESC_PATCH_ABANDON"]        # k2p_patch gave up a repair it had begun
CHECKED = tuple(lib.DBG[k] for k in ("CHK_B_CLUSTER", "CHK_B_DECODE", "CHK_B_RECORD", "CHK_A"))   # how often the checks behind INVARIANTS were made
HOOKS = tuple("VDL2GPU_TEST_" + k for k in ESC)
SIDE = dict(frames=True, levels=True, soft_rs=True, carrier=True)

_runs, _side = {}, {}


def _judge(plane):
    return G.judge("geom") if plane == "geom" else CC.judge(plane)


class Run(types.SimpleNamespace):
    pass


def _run(monkeypatch, plane, base, rounds, env, side, keep=True):
    """the plane, in parts, through the test library with `env` set; counters read (and reset) behind every part.  keep: the run is the
    other half of several cases (the one without the case's hook)."""
    key = (plane, base, rounds, tuple(sorted(env.items())), side)
    if key in _runs:
        return _runs[key]
    kw = _env(monkeypatch, base)
    monkeypatch.setenv("VDL2GPU_REPAIR_ROUNDS", str(rounds))
    monkeypatch.setenv("VDL2GPU_DEBUG_COUNTERS", "1")
    for name in HOOKS + ("VDL2GPU_PRIM_DROP",):
        monkeypatch.delenv(name, raising=False)
    for name, v in env.items():
        monkeypatch.setenv(name, str(v))
    j = _judge(plane)
    raw = j.plane.raw()
    with _rx(min(raw.size // 2, PART), kw, testhooks=True, **(SIDE if side else {})) as rx:
        dec, parts = [], []
        for g in _push_parts(rx, raw):
            dec.append(g)
            parts.append(np.array(rx.debug_counters(NDBG, reset=True), dtype=np.uint64))
        got = rx.poll()
        frames = rx.poll_frames() if side else None
        parts.append(np.array(rx.debug_counters(NDBG, reset=True), dtype=np.uint64))     # (what the last part's tail counted behind the read)
        st = rx.stats()
    behind = parts.pop()
    parts[-1] = parts[-1] + behind
    dec = np.concatenate(dec)
    assert len(dec) == len(j.plane.plane) and np.array_equal(_bits(dec), _bits(j.plane.plane))      # the identity, on the GPU
    r = Run(j=j, got=got, frames=frames, st=st, parts=parts, cnt=np.sum(parts, axis=0), dec=dec, plane=plane)
    if keep:
        _runs[key] = r
    return r


def _columns(b):
    return (repr(b.level), b.soft.tobytes(), repr(b.carrier))


def _check_side(r):
    """levels, reliability maps and carrier sums: against the CPU models the first time a plane comes by, against that run afterwards"""
    if r.plane not in _side:
        whole = types.SimpleNamespace(debug_dec=lambda stream, ch, wide=r.dec.astype(np.complex128): wide)
        TL._check_exact(whole, r.got, types.SimpleNamespace(rate=PC.RATE), "cf32")
        if r.plane == "geom":
            TG._check_soft("geom", r.got)
        else:
            TC._check_soft(r.j, r.got)
        model = {(0, 0, b.trig_dec): (b, sums) for b, sums in CR.tap_sums(r.j.dec, r.j.triggers, r.j.blocks)}
        TCAR._check(r.got, model, least=100)
        _side[r.plane] = {b.trig_dec: _columns(b) for b in r.got}
    want = _side[r.plane]
    assert len(r.got) == len(want)
    for b in r.got:
        assert _columns(b) == want[b.trig_dec], b.trig_dec


def _check(oracle, r, tag):
    """(i) the oracle's records (and frames, and the side columns); (ii) every burst counted, none lost; (iv) the invariants hold"""
    print(f"\n{tag}: counters 64..80 {r.cnt[64:81].tolist()}, by part (escapes) {[p[64:71].tolist() + [int(p[MERGE_SORT])] for p in r.parts]}, "
          f"repaired {int(r.cnt[REPAIRED])}, repairs {r.st['repairs']}, serial_redos {r.st['serial_redos']}, overflowed {r.st['overflowed']}, "
          f"bursts {r.st['bursts']} / {len(r.j.blocks)}, records {len(r.got)}")
    TR._check_bursts(oracle, r.got, r.j.blocks, PC.SDRCLK, r.frames)
    assert r.st["bursts"] == len(r.j.blocks) and r.st["overflowed"] == 0
    assert [int(r.cnt[k]) for k in INVARIANTS] == [0, 0, 0, 0]
    if r.frames is not None:
        _check_side(r)


def _records(r):
    return sorted((b.chn, b.trig_dec, b.end_dec, b.nbrow, b.nlbyte, b.data, int(np.float32(b.df).view(np.uint32))) for b in r.got)


# hook, value, plane, decode path (tests/test_gpu_planes.PATHS: what the handle is made with), VDL2GPU_REPAIR_ROUNDS, further environment,
# with the side columns, reached.  The values: the largest of 1 2 3 4 6 8 12 16 24 32 48 ... at which every part pushed of the plane still
# took the branch on an MI355X, or 1; behind each row the limit's escape counter over the whole plane (parts), as measured there.
PD = {"VDL2GPU_PRIM_DROP": 1}          # every cluster is replayed by the resolver: a serial stretch and a dynamic descriptor per burst
PD_REG = dict(PD, VDL2GPU_TEST_REG_CAP=4)   # ... and all but four regions dropped: the verify pass finds events for a local repair


def _cut(n):
    """every region but n, evenly spread over the part (k2r_regions, test build): bursts the region scan covered and bursts it did not
    alternate, so that a repaired chain rejoins the old one and the next event opens another window"""
    return {"VDL2GPU_TEST_REG_CAP": n}


NR = "noregion-r0"
ROWS = [
    ("REG_CAP", 8, "geom", "default", 0, {}, True, True),       # 8 (8 parts, one k2r_regions each); 12: the last part has fewer regions
    ("REG_CAP", 8, "geom", "default", 1, {}, False, True),
    ("REG_CAP", 8, "geom", "default", 2, {}, False, True),
    ("SEG_CAP", 1, "geom", "default", 1, {}, True, True),       # 154; at 2 the last part lists no third stretch
    ("SEG_CAP", 1, "geom", "default", 2, {}, False, True),
    ("SEG_CAP", 32, "train", "default", 1, {}, False, True),    # 6 (one part); none at 48
    ("SEG_CAP", 32, "train", "default", 2, {}, False, True),
    ("VIS_CAP", 32, "train", "default", 1, {}, True, True),     # 4; none at 48
    ("VIS_CAP", 32, "train", "default", 2, {}, False, True),
    # WIN_CAP cannot be reached while the region scan is dropped (test_a_full_list_is_exact_only_slower says why): the default path
    # with the regions cut.  Two parts of geom's eight get to a second window (2), train's one part does (1); a third window: geom with
    # sixteen regions (1), collide with thirty-two (1).  No value makes every part of geom overflow: most have one event.
    ("WIN_CAP", 1, "geom", "default", 1, _cut(8), True, True),
    ("WIN_CAP", 1, "geom", "default", 2, _cut(8), False, True),
    ("WIN_CAP", 1, "geom", "default", 3, _cut(8), False, True),
    ("WIN_CAP", 1, "train", "default", 1, _cut(8), False, True),
    ("WIN_CAP", 1, "train", "default", 2, _cut(8), False, True),
    ("WIN_CAP", 1, "train", "default", 3, _cut(8), False, True),
    ("WIN_CAP", 2, "geom", "default", 1, _cut(16), False, True),
    ("WIN_CAP", 2, "geom", "default", 2, _cut(16), False, True),
    ("WIN_CAP", 2, "geom", "default", 3, _cut(16), False, True),
    ("WIN_CAP", 2, "collide", "default", 1, _cut(32), False, True),
    ("WIN_CAP", 2, "collide", "default", 2, _cut(32), False, True),
    ("WIN_CAP", 2, "collide", "default", 3, _cut(32), False, True),
    ("MERGE_CAP", 4, "geom", NR, 1, {}, True, True),            # 12; at 6 the last part's verify pass lists fewer
    ("MERGE_CAP", 4, "geom", NR, 3, {}, False, True),
    # SLOG_CAP is not reached either with the region scan dropped (same docstring); with the regions cut to four it is
    ("SLOG_CAP", 1, "train", NR, 1, PD, False, False),
    ("SLOG_CAP", 1, "train", NR, 2, PD, False, False),
    ("SLOG_CAP", 1, "collide", NR, 1, PD, False, False),
    ("SLOG_CAP", 1, "collide", NR, 2, PD, False, False),
    ("SLOG_CAP", 1, "train", "default", 1, PD_REG, True, True),     # k2c_resolve's full log, k2p_patch's refusal
    ("SLOG_CAP", 1, "train", "default", 2, PD_REG, False, True),
    ("SLOG_CAP", 1, "collide", "default", 1, PD_REG, False, True),
    ("SLOG_CAP", 1, "collide", "default", 2, PD_REG, False, True),
    ("STAGE_DYN", 2, "geom", "default", 1, PD, True, True),         # 20; at 3 the last part's chain has three bursts
]


def _also(hook, rounds, r):
    """what a row asserts beside (i) .. (iv)"""
    st = r.st
    if hook == "REG_CAP":
        assert st["repairs"] + st["serial_redos"] > 0, st     # the verify pass found what the missing regions would have
    if hook == "SEG_CAP":
        # a pass that cannot vouch for the channel must not be repaired locally: one round leaves it to K2f, a complete round (which lists
        # no stretches: its tables hold every class) settles it
        assert (st["serial_redos"] > 0) if rounds == 1 else (st["serial_redos"] == 0), st
    if hook == "VIS_CAP":
        # ... and what a complete round cannot settle: its chain visits the same clusters, the list is as full as before -- K2f redoes
        # the channel whatever the rounds
        assert st["serial_redos"] > 0, st
    if hook == "WIN_CAP":
        # k2p_patch gave up a repair it had BEGUN (k2_begin_repair had set redo, the mask and CTL_NWIN0): its unwinding left the channel
        # failed and nothing of a selection -- one round: K2f redoes it; more: a further round resolves it again
        assert r.cnt[ABANDONED] > 0 and r.cnt[CHECKED[3]] > 0       # (... and the walk of invariant (a) had bursts inside windows to look at)
        assert (st["serial_redos"] > 0) if rounds == 1 else (st["serial_redos"] == 0 and st["repairs"] > 0), st
    if hook == "MERGE_CAP" and rounds == 3:
        assert r.cnt[MERGE_SORT] > 0      # the middle round's k2s_merge refused as well: the resolver took the channel serially
    if hook == "STAGE_DYN":
        assert st["serial_redos"] > 0, st


@pytest.mark.timeout(180)
@pytest.mark.parametrize("hook,value,plane,base,rounds,more,side,reached", ROWS,
                         ids=[f"{h}={v}-{pl}-{'noregion' if b != 'default' else 'default'}{'-regcap' if 'VDL2GPU_TEST_REG_CAP' in m else ''}-r{rr}"
                              for h, v, pl, b, rr, m, _, _ in ROWS])
def test_a_full_list_is_exact_only_slower(built, oracle, monkeypatch, hook, value, plane, base, rounds, more, side, reached):
    """WIN_CAP and SLOG_CAP cannot be reached with the region scan dropped (VDL2GPU_F_TEST_NOREGION).  A push's tables then hold
    candidates of the probe's class alone.  The first pass's chain meets candidates while it is in that class; the first burst that
    leaves the detector in another class sends it idling to the end of the push, for no candidate of that class exists.  So every
    event the verify pass finds lies in that one last stretch, behind every candidate the chain met (K2Params.onchain): a repaired chain
    never rejoins, a local repair has ONE window, to the end of the data, whatever the plane -- and the first pass has at most one serial
    stretch for the log (on the chain planes k2p_patch refuses anyway: more than K2S_MERGE new candidates).  A second window needs an
    event between two bursts the region scan covered.  The WIN_CAP rows therefore run the default path with the regions cut
    (VDL2GPU_TEST_REG_CAP, which in the test build keeps the same regions in every run, evenly spread over the part); the SLOG_CAP rows
    with the region scan dropped stay, with their counter pinned at zero, beside those with the regions cut to four, which reach it.
    The WIN_CAP rows are also the ones that reach k2p_patch's unwinding (counter 76): every other limit either fails the channel in
    k2c_resolve, so that k2p_patch leaves at its entry, or refuses there before k2_begin_repair.

    STAGE_DYN: a burst of a serial stretch that found the descriptor pool (or the selection list) full under k2c_resolve was counted
    in n_burst but neither decoded nor added to `overflowed` -- the resolver never looked at MachOut.badslot, and nothing reads
    CTL_STAGE_OVF (on an MI355X: 8 records for the oracle's 135, `overflowed` 0).  It fails the channel now, as k2b_clusters and
    k2p_patch always did, and K2f redoes it: the row asserts the oracle's records and a serial redo.  (The selection list's own limit,
    VDL2_SEL_CAP, has no hook: that half of the fix stands on reading alone.)"""
    plain = _run(monkeypatch, plane, base, rounds, more, side)
    _check(oracle, plain, f"{plane} {base} r{rounds} {more} without a hook")
    assert plain.cnt[ESC[hook]] == 0 and (hook != "MERGE_CAP" or plain.cnt[MERGE_SORT] == 0)
    r = _run(monkeypatch, plane, base, rounds, dict(more, **{"VDL2GPU_TEST_" + hook: value}), side, keep=False)
    _check(oracle, r, f"{plane} {base} r{rounds} {more} {hook}={value}")
    assert (r.cnt[ESC[hook]] > 0) if reached else (r.cnt[ESC[hook]] == 0)       # (iii) the branch was taken ...
    assert _records(r) == _records(plain)           # ... and changed nothing
    _also(hook, rounds, r)


@pytest.mark.timeout(180)
@pytest.mark.parametrize("rounds", (1, 3))
@pytest.mark.parametrize("plane", CC.FAMILIES + ("geom",))
def test_production_repair_schedules_on_the_crafted_planes(built, oracle, monkeypatch, plane, rounds):
    """one round is what every product handle schedules -- a local repair, then a serial redo of whatever it leaves failed --, three have
    the middle k2s_merge + k2c_resolve round; with the region scan dropped the verify pass finds the triggers and the rounds run"""
    r = _run(monkeypatch, plane, "noregion-r0", rounds, {}, False)
    _check(oracle, r, f"{plane} noregion r{rounds}")
    if rounds == 1:
        assert r.cnt[REPAIRED] > 0      # without it the run says nothing about k2p_patch
    # the invariant counters' zeros are zeros of checks that were made: every cluster's first descriptor (k2b_clusters) on every plane;
    # on geom, whose local repairs succeed, also K2d's descriptors and the records its second pass tags.  (Invariant (a)'s walk finds
    # no burst inside a window here -- without the region scan the one window lies behind everything the first pass selected --: the
    # WIN_CAP rows assert that one.)
    assert r.cnt[CHECKED[0]] > 0
    if plane == "geom":
        assert r.cnt[CHECKED[1]] > 0 and r.cnt[CHECKED[2]] > 0
