"""CPU checks of the view selection (include/pft_view.h): the NumPy model (tests/view_model.py) against the answers worked
out by hand and the claims of tests/view_cases.py, the two finiteness rules, the decimation rule, and the property the
feature exists for on the scene's box: the selected subset of a full-surface model matches a frame better than the full
model, and holds the faces that face the camera."""
import numpy as np
import pytest

import view_cases as wc
import view_model as wm
import visibility_model as vm

F = np.float32


def run(c, **kw):
    return wm.select(c["cam"], c["xyz"], c["T"], c["K"], **kw)


def check_consistent(o):
    kept = o["kept_index"]
    assert np.all(np.diff(kept.astype(np.int64)) > 0)
    assert kept.tolist() == np.flatnonzero(o["state"] == wm.KEPT).tolist()
    assert o["n_kept"] == len(kept) == o["n_state"][wm.KEPT]
    assert o["n_visible"] == o["n_state"][wm.KEPT] + o["n_state"][wm.DECIMATED]
    assert sum(o["n_state"]) == o["n_model"]
    assert not o["self_gap"][np.isin(o["state"], (wm.OUT_OF_VIEW, wm.NONFINITE))].any()


@pytest.mark.parametrize("name", sorted(wc.HAND_MADE))
def test_model_answers_worked_out_by_hand(name):
    c = wc.HAND_MADE[name]()
    o = run(c)
    assert o["state"].tolist() == c["state"]
    if "gap" in c:
        assert o["self_gap"].tolist() == [F(g) for g in c["gap"]]
    if "claim" in c:
        assert c["claim"](o)
    check_consistent(o)


def test_strict_gate_is_one_ulp_wide():
    o = run(wc.strict_gate())
    m = F(wc.MARGIN)
    assert o["self_gap"][1] == m and o["state"][1] == wm.KEPT
    assert o["self_gap"][3] == m + F(2.0 ** -22) and o["state"][3] == wm.SELF_OCCLUDED  # (one ulp of the depth 2 + margin)


def test_what_the_two_finiteness_rules_keep_out():
    """A q = (0, 0, +inf) is in_view (x / z = 0), its footprint splats +inf, and its gap is fmaxf(inf - inf, 0) = 0: the
    classification alone would select it.  Such a q comes from a finite record by overflow, and the finiteness clause of
    rule 2 is what keeps it out.  The record (0, 0, +inf) itself never gets that far through xform -- a zero entry of T
    times inf is NaN, so qx is NaN and rule 2 takes it without rule 1 as well; rule 1 gives it its own state, before any
    arithmetic is done on it"""
    cam = wc.small()
    ok, _, _ = vm.project(cam, [[0, 0, np.inf]])
    assert ok[0]
    assert np.isinf(vm.depth_image(cam, [[0, 0, np.inf]])).all()
    with np.errstate(all="ignore"):
        assert np.fmax(F(np.inf) - F(np.inf), F(0)) == 0
    c = wc.overflowing_q()
    assert run(c)["state"].tolist() == [wm.OUT_OF_VIEW, wm.OUT_OF_VIEW, wm.KEPT]
    o = run(c, q_finite=False)
    assert o["state"][0] == wm.KEPT and 0 in o["kept_index"]  # selected: a reference point at infinity
    c = wc.nonfinite_records()
    assert np.isinf(c["xyz"][7, 2]) and not c["xyz"][7, :2].any()
    assert run(c)["state"][7] == wm.NONFINITE
    o = run(c, rule1=False)
    assert np.isnan(vm.xform(c["T"], c["xyz"][7:8])[0, 0])
    assert o["state"][:9].tolist() == [wm.OUT_OF_VIEW] * 9 and o["kept_index"].tolist() == [9]
    assert run(c, rule1=False, q_finite=False)["kept_index"].tolist() == [9]  # (a NaN fails in_view)


@pytest.mark.parametrize("K", wc.DECIMATION_K)
def test_decimation_keeps_exactly_k_ascending(K):
    o = run(wc.decimation(K))
    n = wc.DECIMATION_N
    assert o["n_visible"] == n
    assert o["n_kept"] == min(K, n)
    check_consistent(o)
    if K < n:  # the kept ranks are the r at which floor(r K / n) steps: spread over the whole range
        assert o["kept_index"].tolist() == [r for r in range(n) if (r + 1) * K // n > r * K // n]
        assert o["kept_index"][-1] == n - 1


def test_decimation_by_hand():
    assert run(wc.decimation(5))["kept_index"].tolist() == [2, 4, 7, 9, 11]
    assert run(wc.decimation(1))["kept_index"].tolist() == [11]
    assert run(wc.decimation(11))["kept_index"].tolist() == list(range(1, 12))


@pytest.mark.parametrize("N", wc.SIZES)
def test_sizes(N):
    o = run(wc.shell(N))
    assert o["n_model"] == N
    check_consistent(o)


def test_big_shell_is_half_visible_and_decimated_across_tiles():
    c, o = wc.expected("big")
    assert o["n_model"] == wc.BIG
    assert 0.3 < o["n_visible"] / wc.BIG < 0.6
    assert o["n_kept"] == 50001 and o["n_state"][wm.NONFINITE] > 0
    check_consistent(o)


# ---- the property on the scene's box ---------------------------------------------------------------------------------------
ROLLS = (0.2, 0.5, 0.8, 1.1, 1.4)


@pytest.fixture(scope="module")
def lattice():
    from pcl_tracking_amd import scene

    xyz, fid = scene._box_surface_lattice(scene.MODEL_DIMS, 0.01)
    return xyz.astype(F), fid


def share_within(points, frame, d=0.02):
    """the share of `points` with a frame point within d"""
    lo, hi = points.min(0) - d, points.max(0) + d
    near = frame[np.all((frame >= lo) & (frame <= hi), 1)].astype(np.float64)
    if not len(near):
        return 0.0
    hit = 0
    for a in range(0, len(points), 512):
        p = points[a:a + 512].astype(np.float64)
        d2 = ((p[:, None, :] - near[None, :, :]) ** 2).sum(2)
        hit += int((d2.min(1) <= d * d).sum())
    return hit / len(points)


@pytest.mark.parametrize("roll", ROLLS)
def test_selected_subset_matches_the_frame_better_than_the_full_lattice(lattice, roll):
    from pcl_tracking_amd import scene

    xyz, fid = lattice
    pose = list(scene.GT_POSE)
    pose[3] = roll
    T = scene.pose_matrix(*pose)[:3].astype(F)
    o = wm.select(vm.camera(), xyz, T)
    frame = scene.make_scene(50000, obj_pose=tuple(pose))
    frame = np.stack([frame["x"], frame["y"], frame["z"]], 1)
    moved = vm.xform(T, xyz)
    full = share_within(moved, frame)
    sel = share_within(moved[o["kept_index"]], frame)
    print("roll %.1f: selected %d of %d, share within 2 cm %.3f (selected) %.3f (full)" % (roll, o["n_kept"], len(xyz), sel, full))
    assert sel > full
    faces = scene._visible_faces(scene.MODEL_DIMS, tuple(pose))
    on_visible = np.isin(fid, faces)
    recall = float((o["state"][on_visible] == wm.KEPT).mean())
    print("roll %.1f: recall on the faces that face the camera %.3f" % (roll, recall))
    if roll in (0.2, 0.8):  # (at the other rolls the default 160 x 90 camera drops steep faces: DESIGN.md section 3.17)
        assert recall == 1.0
