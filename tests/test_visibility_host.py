"""CPU checks of the visibility (include/pft_visibility.h): the NumPy model (tests/visibility_model.py) against answers
worked out by hand, the library's host projection against the model bit by bit at the edges of the definition, the strict
gates, the defaults, and every scenario of tests/test_gpu_visibility.py run through the model alone, so that each case
shows the states it claims."""
import ctypes as C

import numpy as np
import pytest

import visibility_cases as vc
import visibility_model as vm

F = np.float32


@pytest.fixture(scope="module")
def lib():
    from pcl_tracking_amd import build

    build.build()
    from pcl_tracking_amd import _lib

    _lib.load()
    return _lib


def run(case, **kw):
    return vm.visibility(case["cam"], case["ref"], case["T"], case["frame"], **kw)


# ---- the model against answers worked out by hand ------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(vc.HAND_MADE))
def test_model_answers_worked_out_by_hand(name):
    case = vc.HAND_MADE[name]()
    o = run(case)
    assert o["state"].tolist() == case["state"]
    assert o["scene_gap"].tolist() == [F(g) for g in case["scene_gap"]]
    assert o["self_gap"].tolist() == [F(g) for g in case["self_gap"]]
    for k, s in (("n_visible", vm.VISIBLE), ("n_occluded", vm.OCCLUDED), ("n_self", vm.SELF_OCCLUDED), ("n_out", vm.OUT_OF_VIEW)):
        assert o[k] == case["state"].count(s)


def test_footprint_is_clipped_at_the_image_border():
    cam = vc.small(splat=4)
    Z = vm.depth_image(cam, vc.pts([vc.at_pixel(cam, 0, 0, 1.0), vc.at_pixel(cam, 15, 11, 2.0)]))
    want = np.full((12, 16), np.inf, F)
    want[:5, :5] = 1.0
    want[7:, 11:] = 2.0
    np.testing.assert_array_equal(Z, want)


def test_strict_gates_gap_equal_to_the_margin_is_not_occluded():
    case = vc.strict_gates()
    o = run(case)
    m = F(vc.MARGIN)
    assert o["scene_gap"][0] == m and o["state"][0] == vm.VISIBLE
    assert o["self_gap"][3] == m and o["state"][3] == vm.VISIBLE
    assert o["scene_gap"][1] > m and o["state"][1] == vm.OCCLUDED
    assert o["self_gap"][5] > m and o["state"][5] == vm.SELF_OCCLUDED


def test_the_rule():
    thr = (0.25, 0.5, 2)
    assert vm.rule(100, 80, 100, True, thr, 0) == (False, False, 0, False)
    assert vm.rule(100, 49, 100, True, thr, 0) == (False, True, 1, False)
    assert vm.rule(100, 49, 100, True, thr, 1) == (False, True, 2, True)
    assert vm.rule(24, 0, 100, True, thr, 1) == (True, False, 1, False)   # hidden: the streak is held
    assert vm.rule(25, 13, 100, True, thr, 1) == (False, False, 0, False)  # 25 is not below 0.25 * 100; 13 not below 12.5
    assert vm.rule(100, 0, 100, False, thr, 1) == (False, False, 1, False)  # no match: held
    assert vm.rule(0, 0, 100, True, vm.DEFAULT_THRESHOLD, 0) == (True, False, 0, False)
    assert vm.rule(100, 0, 100, True, vm.DEFAULT_THRESHOLD, 0) == (False, False, 0, False)  # the defaults never fire


# ---- the library's host projection against the model ----------------------------------------------------------------------
def lib_project(lib, cam, xyz):
    c = lib.VisibilityConfig(cam["width"], cam["height"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["z_near"],
                             cam["splat"], cam["occlusion_margin"], cam["self_margin"])
    p = np.asarray(xyz, F)
    uv = np.array([-7, -7], np.int32)
    ok = lib.load().pft_visibility_project(C.byref(c), p.ctypes.data_as(C.c_void_p), uv.ctypes.data_as(C.c_void_p))
    return ok, uv.tolist()


def test_defaults(lib):
    c = lib.VisibilityConfig()
    lib.load().pft_visibility_config_default(C.byref(c))
    got = {f: getattr(c, f) for f, _ in c._fields_}
    floats = ("fx", "fy", "cx", "cy", "z_near")  # float fields: the default is the float nearest the decimal
    assert got == {k: float(F(v)) if k in floats else v for k, v in vm.DEFAULT_CAMERA.items()}
    assert (c.occlusion_margin, c.self_margin, c.splat, c.width, c.height) == (0.03, 0.03, 1, 160, 90)
    assert C.sizeof(lib.VisibilityConfig) == 48 and C.sizeof(lib.VisibilityStatsStruct) == 104


def test_projection_bits(lib):
    cam = vc.small(width=64, height=48, fx=64.0, fy=64.0, cx=32.0, cy=24.0)
    e = 2.0 ** -24
    edge = [
        ([0.25, 0.0, 1.0], (1, [48, 24])),        # uf == 48.0 exactly: pixel 48
        ([0.25 - e, 0.0, 1.0], (1, [47, 24])),    # uf = 48 - 2^-18, the float just below 48: pixel 47
        ([0.25 - e / 4, 0.0, 1.0], (1, [48, 24])),  # the x just below 0.25: 64 x = 16 - 2^-20, and 48 - 2^-20 rounds to 48.0
        ([0.5, 0.0, 1.0], (0, None)),             # uf == W: out
        ([0.5 - 2 * e, 0.0, 1.0], (1, [63, 24])),  # uf = 64 - 2^-17, representable
        ([0.5 - e / 2, 0.0, 1.0], (0, None)),     # the x just below 0.5: 64 - 2^-19 is a tie and rounds to even, 64.0: out
        ([-0.5, 0.0, 1.0], (1, [0, 24])),         # uf == 0: in
        ([np.nextafter(F(-0.5), F(-1)), 0.0, 1.0], (0, None)),
        ([0.0, 0.375, 1.0], (0, None)),           # vf == H: out
        ([0.0, 0.0, cam["z_near"]], (0, None)),   # z == z_near: not in front
        ([0.0, 0.0, np.nextafter(F(cam["z_near"]), F(1))], (1, [32, 24])),
        ([0.0, 0.0, 0.0], (0, None)), ([0.0, 0.0, -0.0], (0, None)), ([0.1, 0.1, -1.0], (0, None)),
        ([np.nan, 0.0, 1.0], (0, None)), ([0.0, np.nan, 1.0], (0, None)), ([0.0, 0.0, np.nan], (0, None)),
        ([np.inf, 0.0, 1.0], (0, None)), ([-np.inf, 0.0, 1.0], (0, None)), ([0.0, np.inf, 1.0], (0, None)),
        ([0.0, 0.0, np.inf], (1, [32, 24])),      # x / inf = 0: the principal point
        ([np.inf, 0.0, np.inf], (0, None)),       # inf / inf = NaN
        ([0.0, 0.0, -np.inf], (0, None)),
    ]
    for xyz, (want_ok, want_uv) in edge:
        ok, uv = lib_project(lib, cam, xyz)
        m_ok, m_u, m_v = vm.project(cam, [xyz])
        assert ok == want_ok == int(m_ok[0]), xyz
        if ok:
            assert uv == want_uv == [int(m_u[0]), int(m_v[0])], xyz
        else:
            assert uv == [-7, -7], xyz  # written only when in view
    # and bit for bit on random points around the borders of the default camera
    rng = np.random.default_rng(1)
    cam = vm.camera()
    z = rng.uniform(0.03, 2.0, 4000).astype(F)
    p = np.stack([rng.uniform(-1.0, 1.0, 4000).astype(F) * z, rng.uniform(-0.6, 0.6, 4000).astype(F) * z, z], 1)
    m_ok, m_u, m_v = vm.project(cam, p)
    assert 0.2 < m_ok.mean() < 0.95
    for i in range(len(p)):
        ok, uv = lib_project(lib, cam, p[i])
        assert ok == int(m_ok[i])
        if ok:
            assert uv == [int(m_u[i]), int(m_v[i])]


# ---- the GPU file's scenarios by the model alone --------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(vc.ADVERSARIAL))
def test_adversarial_cases_show_what_they_claim(name):
    case = vc.ADVERSARIAL[name]()
    assert 1 <= len(case["ref"]) <= 300 and 1 <= len(case["frame"]) <= 2000
    o = run(case)
    assert case["claim"](o), {k: o[k] for k in ("n_visible", "n_occluded", "n_self", "n_out")}
    assert o["n_visible"] + o["n_occluded"] + o["n_self"] + o["n_out"] == o["n_reference"]


def tracked(kind, **kw):
    ref = vc.cloud_xyz(vc.patch_model())
    return vm.visibility(vm.camera(), ref, vc.patch_trans()[:3], vc.cloud_xyz(vc.patch_frame(kind)), **kw)


def test_half_covered_patch_has_both_states():
    o = tracked("half")
    assert o["n_visible"] >= 100 and o["n_occluded"] >= 100 and o["n_self"] == 0 and o["n_out"] == 0
    covered = o["state"] == vm.OCCLUDED
    assert np.all(np.abs(o["scene_gap"][covered] - 0.2) < 0.05)  # the plate is 0.2 m in front
    assert not tracked("full")["n_occluded"] and tracked("hidden")["n_visible"] == 0


def test_rule_sequence_crosses_its_thresholds():
    """the frames of the GPU rule test at the nominal pose: a matched point is one with a frame point within 1 cm"""
    ref = vc.cloud_xyz(vc.patch_model())
    q = vm.xform(vc.patch_trans()[:3], ref)
    streak, seen = 0, []
    for kind in vc.RULE_SEQUENCE:
        fr = vc.cloud_xyz(vc.patch_frame(kind))
        near = np.array([np.min(np.linalg.norm(fr - p, axis=1)) < 0.01 for p in q])
        o = tracked(kind, match_idx=np.where(near, 0, -1), threshold=vc.RULE_THRESHOLD, prev_streak=streak)
        streak = o["streak"]
        seen.append((o["hidden"], o["below"], o["streak"], o["lost"]))
    assert seen == [(False, False, 0, False), (False, True, 1, False), (True, False, 1, False), (False, True, 2, True),
                    (False, False, 0, False), (False, True, 1, False)]
