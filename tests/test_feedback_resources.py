"""What the compiler made of the kernels VDL2GPU_F_FEEDBACK adds -- the eight k2d_payload*_fb, k2f_commit_fb, k4_frames_fb,
k4_frames_rep_fb and k_export_feedback: listed, no vector spills, the occupancy of their siblings -- and of every kernel that existed
before: the line profiles/r21_kernel_resources.txt recorded for the parent, figure for figure."""
import os

from test_build_resources import resources  # noqa: F401  (the fixture: kernel_resources.txt as build_hip() wrote it)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REC = os.path.join(ROOT, "profiles", "r21_kernel_resources.txt")

K2D = ["k2d_payload", "k2d_payload_lev", "k2d_payload_soft", "k2d_payload_lev_soft",
       "k2d_payload_car", "k2d_payload_lev_car", "k2d_payload_soft_car", "k2d_payload_lev_soft_car"]


def _z(name):
    return f"_Z{len(name)}{name}"


def _recorded():
    """({name: line} of the parent's section, {name: line} of the added section)"""
    parent, added, cur = {}, {}, None
    for ln in open(REC):
        if ln.startswith("# ---- parent"):
            cur = parent
        elif ln.startswith("# ---- added"):
            cur = added
        elif not ln.startswith("#") and ln.strip():
            cur[ln.split(" ", 1)[0]] = ln.rstrip("\n")
    return parent, added


def _line(name, fields):
    return name + " " + " ".join(f"{a}={b}" for a, b in sorted(fields.items()))


def _one(resources, prefix):  # noqa: F811
    hit = [k for k in resources if k.startswith(prefix + "8K")]
    assert len(hit) == 1, (prefix, hit)
    return resources[hit[0]]


def test_new_payload_kernels_do_not_spill_and_keep_four_waves(resources):  # noqa: F811
    for k in K2D:
        r, sib = _one(resources, _z(k + "_fb")), _one(resources, _z(k))
        assert r["VGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] == 0, k
        assert r["Occupancy [waves/SIMD]"] >= 4, k          # amdgpu_waves_per_eu(4, 8), like k2d_payload_lev .. k2d_payload_lev_soft_car
        # the indices go where the phases were: no LDS beyond the sibling without the pass, but for one word (S)
        assert 0 <= r["LDS Size [bytes/block]"] - sib["LDS Size [bytes/block]"] <= 8, k


def test_new_block_kernels_do_not_spill_and_keep_four_waves(resources):  # noqa: F811
    for k in ("k4_frames_fb", "k4_frames_rep_fb"):
        r = _one(resources, _z(k))
        assert r["VGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] == 0, k
        assert r["Occupancy [waves/SIMD]"] >= 4, k
    assert _one(resources, _z("k4_frames_fb"))["LDS Size [bytes/block]"] == _one(resources, _z("k4_frames"))["LDS Size [bytes/block]"]
    assert _one(resources, _z("k4_frames_rep_fb"))["LDS Size [bytes/block]"] == _one(resources, _z("k4_frames_rep"))["LDS Size [bytes/block]"]


def test_serial_commit_with_feedback_uses_no_scratch(resources):  # noqa: F811
    r, sib = _one(resources, _z("k2f_commit_fb")), _one(resources, _z("k2f_commit"))
    assert r["VGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] == 0
    assert r["Occupancy [waves/SIMD]"] >= sib["Occupancy [waves/SIMD]"]
    assert r["LDS Size [bytes/block]"] == sib["LDS Size [bytes/block]"]         # the indices borrow the cluster mode's sample tile
    e = [v for k, v in resources.items() if k.startswith("_Z17k_export_feedback")]
    assert len(e) == 1 and e[0]["VGPRs Spill"] == 0 and e[0]["ScratchSize [bytes/lane]"] == 0


def test_every_kernel_that_existed_keeps_its_line(resources):  # noqa: F811
    parent, added = _recorded()
    assert len(parent) == 75 and len(added) == 12
    for name, want in parent.items():
        assert name in resources, name
        assert _line(name, resources[name]) == want, name
    # and the build has nothing the record does not know
    assert set(resources) == set(parent) | set(added)
