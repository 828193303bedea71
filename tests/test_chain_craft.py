"""The planes of tests/chain_craft.py against the oracle, on the CPU: the COVERAGE CONDITIONS that keep tests/test_gpu_chain.py from
passing on inputs that miss the region they aim at -- a follower triggered while the detector still fits a partly stale ring, on both
sides of the 68 evaluations after which it is history-free again.  Held against the oracle's own triggers and blocks, never the GPU.

"count" is (a trigger's dec_index - the previous block's end_dec) / 2 in the oracle's stamps (chain_craft.count).
Run with -s for the counts each family reaches (DESIGN.md section 2 quotes them)."""
import collections

import numpy as np
import pytest

import chain_craft as CC
import plane_craft as PC


@pytest.fixture(scope="module")
def J(oracle):
    return CC.judge


@pytest.mark.parametrize("name", CC.FAMILIES)
def test_the_plane_is_the_identity_and_the_groups_stand_alone(J, name):
    j = J(name)
    assert len(j.dec) == len(j.plane.plane) < 1_000_000
    assert np.array_equal(j.dec.view(np.uint32), j.plane.plane.view(np.uint32))
    assert np.isfinite(j.plane.plane.view(np.float32)).all()
    gs = CC.groups_of(j.plane)
    # every group's head is met by an idle, history-free detector: whatever a group did to the receiver is over before the next one
    for g in gs:
        t = j.sync_trigger(g[0])
        assert CC.block_of(j, g[0]) is not None, (g[0].label, g[0].group)
        c = CC.count(j, t)
        assert c is None or c >= CC.STEADY + PC.GAP // 4, (g[0].label, c)
        assert all(x.tail == 0 for x in g[:-1])         # no tail symbols inside a group
    assert CC.unsettled(j) == {}                        # RESERVE holds every header a stale sync word got accepted (a stale table fails here)
    assert len({b.trig_dec for b in j.blocks}) == len(j.blocks)


@pytest.mark.parametrize("name", CC.FAMILIES)
def test_two_runs_of_the_builder_give_the_same_blocks(J, name):
    j = J(name)
    again = CC.run_oracle(CC.layout(name, CC.family_groups(name), CC.NOISE, 100 + CC.FAMILIES.index(name), CC.RESERVE.get(name, {})))
    assert np.array_equal(again.plane.plane.view(np.uint32), j.plane.plane.view(np.uint32))
    assert [(b.trig_dec, b.end_dec, b.key()) for b in again.blocks] == [(b.trig_dec, b.end_dec, b.key()) for b in j.blocks]


def _pairs(j, sweep):
    """[(A, B, B's block or None, B's count or None, the sub-phase B was met in)] of the sweep's groups.  A trigger on B's sync word
    whose header decodes to another length than B's (a few do, met on a stale ring) is not B taken: it counts as lost."""
    out = []
    for g in CC.groups_of(j.plane):
        if g[0].sweep != sweep:
            continue
        a, b = g
        blk = CC.block_of(j, b)
        if blk is not None and (blk.nbrow, blk.nlbyte) != (1, len(b.payload)):
            blk = None
        t = j.sync_trigger(b)
        out.append((a, b, blk, CC.count(j, t) if blk else None, CC.met_in(j, t) if blk else None))
    return out


def test_claim_meets_b_on_both_sides_of_steady(J):
    j = J("claim")
    rows = _pairs(j, "long")
    assert len(rows) == len(CC.CLAIM_SWEEP) == 288
    cnt = collections.Counter(c for *_, blk, c, _ in rows if blk)
    lost = sum(blk is None for *_, blk, _, _ in rows)
    below = {r for *_, blk, c, r in rows if blk and c < CC.STEADY}
    above = {r for *_, blk, c, r in rows if blk and c >= CC.STEADY}
    stale = [t for t in j.triggers if (CC.count(j, t) or 99) <= 3]
    print(f"\nclaim: B taken at counts {sorted(cnt.items())}, lost in {lost}; sub-phases below 68 {sorted(below)}, from 68 {sorted(above)}; "
          f"{len(stale)} stale-word triggers at a count <= 3, {sum(t['accepted'] == 1 for t in stale)} of them accepted")
    for c in range(62, 76):
        assert cnt[c] >= 4, (c, cnt[c])             # every count from 62 to 75, four cases or more each
    assert lost >= 10                               # B's sync word inside the time A claims
    assert below == above == {0, 1, 2, 3}           # B met from each of the four sub-phases, both sides of 68
    for a, b, blk, _, _ in rows:                    # A's block is the length it CLAIMS, B's the one it sent
        ba = CC.block_of(j, a)
        assert (ba.nbrow, ba.nlbyte) == (1, CC.CLAIM_BITS // 8)
        assert blk is None or (blk.nbrow, blk.nlbyte) == (1, 14)
    short = _pairs(j, "short")
    assert len(short) == len(CC.SHORT_SWEEP)
    for a, b, blk, c, _ in short:                   # the other half: the receiver is back to idle inside A's own payload, B follows A's true end
        ba = CC.block_of(j, a)
        assert (ba.nbrow, ba.nlbyte) == (1, CC.SHORT_BITS // 8) and a.claimed() < a.sent() - CC.STEADY // 4
        assert blk is not None and c >= CC.STEADY and ba.end_dec < b.t0 < blk.trig_dec, (b.label, c)
    assert {r for *_, r in short} == {0, 1, 2, 3}


def test_collide_meets_b_on_both_sides_of_steady(J):
    j = J("collide")
    rows = _pairs(j, "collide")
    assert len(rows) == len(CC.COLLIDE_SWEEP) == 320
    cnt = collections.Counter(c for *_, blk, c, _ in rows if blk)
    print(f"\ncollide: B taken at counts {sorted(cnt.items())}, lost in {sum(blk is None for *_, blk, _, _ in rows)}")
    assert sum(n for c, n in cnt.items() if c <= CC.STEADY - 1) >= 20
    assert sum(n for c, n in cnt.items() if c >= CC.STEADY) >= 20
    for a, b, blk, c, _ in rows:                    # B's ramp and sync word really lie on A's last symbols where it is met early
        if blk and c < CC.STEADY:
            assert b.t0 < a.t0 + PC.SPS * (a.sent() - 1)


def test_trains_run_past_the_cluster_limit(J):
    j = J("train")
    whole = collections.defaultdict(list)
    nxt = None
    for g in CC.groups_of(j.plane):
        train = [c for c in g if c.role != "next"]
        blks = [CC.block_of(j, c) for c in train]
        cs = [CC.count(j, j.sync_trigger(c)) for c, b in zip(train[1:], blks[1:]) if b]
        if all(blks) and len(cs) == len(train) - 1 and all(1 <= c < CC.STEADY for c in cs):
            whole[len(train)].append(g[0].param)
            assert [(b.nbrow, b.nlbyte) for b in blks] == [(1, 12 + k) for k in range(len(train))]       # each burst its own length
        if g[-1].role == "next" and all(blks):
            b = CC.block_of(j, g[-1])
            nxt = CC.count(j, j.sync_trigger(g[-1])) if b else None
    print(f"\ntrain: overlaps at which every burst is taken and every follower met below 68, per length: {dict(whole)}; the burst behind a train at {nxt}")
    for n in CC.TRAIN_LENGTHS:
        assert whole[n], n
    assert len({ov for n in CC.TRAIN_LENGTHS if n > CC.MAXB for ov in whole[n]}) >= 3     # three overlaps carry trains past VDL2_CL_MAXB
    assert nxt is not None and 68 <= nxt <= 72


def test_swallowed_bursts_give_no_block(J):
    j = J("swallow")
    rows = collections.Counter()
    for g in CC.groups_of(j.plane):
        a = CC.block_of(j, g[0])
        assert a is not None and a.nbrow in (2, 8) and a.nbrow == g[0].length_bits // 1992 + 1
        for c in g[1:]:
            b = CC.block_of(j, c)
            if c.role.startswith("in"):
                assert a.trig_dec < c.t0 and c.t0 + PC.SPS * c.sent() < a.end_dec       # wholly inside the claimed time ...
                assert b is None and j.sync_trigger(c) is None, (c.label, c.role)        # ... the receiver was busy: no trigger, no block
            if c.role == "across":
                assert c.t0 < a.end_dec < c.t0 + PC.SPS * c.sent()
                rows[(a.nbrow, "across", b is not None)] += 1
            if c.role == "behind":
                assert b is not None and (b.nbrow, b.nlbyte) == (1, 13), (c.label, c.role)
        assert not [b for b in j.blocks if a.trig_dec < b.trig_dec < a.end_dec]          # nothing at all from inside it
    print(f"\nswallow: {dict(rows)}")
    assert {k[0] for k in rows} == {2, 8}
    assert {k[2] for k in rows} == {True, False}    # the burst across the claimed end: taken at some offsets, lost at others


def test_stale_tables_are_what_the_oracle_finds(J):
    j = J("stale")
    rej, acc = CC.stale_found(j)
    assert rej == CC.STALE_REJECTED and acc == CC.STALE_ACCEPTED
    early = [t for t in j.triggers if (CC.count(j, t) or 99) <= 3]
    refused = [t for t in early if t["accepted"] == 0]
    print(f"\nstale: {len(early)} triggers at a count <= 3, {len(refused)} refused, {len(acc)} accepted with lengths {sorted({a[2] for a in acc})}")
    assert len(refused) >= 10 and len(rej) >= 10
    assert acc                                      # (the search found accepted ones; see the comment at STALE_ACCEPTED)
    gs = {g[0].label: g for g in CC.groups_of(j.plane)}
    for n, s, bits in acc:                          # the one burst inside the time an accepted stale header claims is lost
        a, b = gs[f"{n}/{s}"]
        blk = CC.block_of(j, a)
        st = [b2 for b2 in j.blocks if 0 < b2.trig_dec - blk.end_dec <= 6]
        assert len(st) == 1 and st[0].trig_dec < b.t0 and b.t0 + PC.SPS * b.sent() < st[0].end_dec
        assert CC.block_of(j, b) is None
    for n, s in rej:                                # the real burst behind a refused stale header is taken
        a, b = gs[f"{n}/{s}"]
        assert CC.block_of(j, b) is not None


@pytest.mark.parametrize("name", ("train", "claim"))
def test_block_cuts_fall_where_the_state_is_carried(J, name):
    j = J(name)
    blocks = CC.cutting_blocks(j)       # asserts that it found each kind of cut
    n_in = 2 * len(j.plane.plane)
    assert 1 <= len(blocks) <= 3
    assert all(b % 2 == 1 and 2 * CC.SERIAL_BELOW < b < n_in for b in blocks)
