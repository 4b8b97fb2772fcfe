"""CPU checks of scene subtraction: the NumPy model (tests/subtract_model.py) against answers worked out by hand, the
scenarios of tests/test_gpu_subtract.py by the model alone (each case has to test what it claims), and what the C ABI
(include/pft_subtract.h) answers without a GPU."""
import ctypes as C

import numpy as np
import pytest

import segment_model as sg
import subtract_cases as sc
import subtract_model as sm

F = np.float32
I = sc.matrix()


def test_model_known_answers():
    model = np.array([[0, 0, 0], [1, 0, 0]], F)
    T = sc.matrix((0.5, 0.0, 0.0))  # moved: (0.5, 0, 0), (1.5, 0, 0)
    frame = np.array([[0.5, 0.1, 0], [1.5, 0, 0.2], [1.0, 0, 0], [0.5, 0, 0], [9, 9, 9]], F)
    r = sm.subtract(frame, {7: (model, T)}, 0.25)
    np.testing.assert_array_equal(r["owner"], [7, 7, -1, 7, -1])
    np.testing.assert_array_equal(r["d2"], np.array([F(0.1) * F(0.1), F(0.2) * F(0.2), np.inf, 0.0, np.inf], F))
    np.testing.assert_array_equal(r["residual_idx"], [2, 4])
    assert (r["n_in"], r["n_explained"], r["n_residual"]) == (5, 3, 2)
    assert r["support"][7] == 3 and r["support"].sum() == 3
    # a rotation: 90 degrees about z takes (1, 0, 0) to (0, 1, 0)
    Rz = np.array([[0, -1, 0, 0], [1, 0, 0, 0], [0, 0, 1, 0]], F)
    np.testing.assert_array_equal(sm.xform(Rz, np.array([[1, 0, 0]], F)), [[0, 1, 0]])
    # the smallest distance wins, whatever the slot order
    r = sm.subtract(np.array([[0.1, 0, 0]], F), {0: (np.array([[0.3, 0, 0]], F), I), 1: (np.array([[0, 0, 0]], F), I)}, 0.25)
    assert r["owner"][0] == 1 and r["d2"][0] == F(0.1) * F(0.1)
    # no slot, an empty slot, an empty frame
    assert sm.subtract(frame, {}, 0.25)["n_residual"] == 5
    assert sm.subtract(frame, {3: (np.zeros((0, 3), F), I)}, 0.25)["n_residual"] == 5
    assert sm.subtract(np.zeros((0, 3), F), {3: (model, I)}, 0.25)["n_in"] == 0


def test_model_summation_order():
    """xform is ((T0 x + T1 y) + T2 z) + T3 and d2 is (dx dx + dy dy) + dz dz, every step rounded to float"""
    T = np.array([[F(1e8), F(1.0), F(-1e8), F(0.5)], [0, 1, 0, 0], [0, 0, 1, 0]], F)
    got = sm.xform(T, np.array([[1.0, 0.25, 1.0]], F))[0, 0]
    assert got == F(F(F(F(1e8) + F(0.25)) + F(-1e8)) + F(0.5)) == F(0.5)  # 0.25 is lost in the first sum
    x = np.array([[F(4096.0), F(2.0 ** -6), F(2.0 ** -6)]], F)
    d = sm.sq_dist(x, np.zeros((1, 3), F))[0, 0]
    assert d == F(F(F(4096.0 * 4096.0) + F(2.0 ** -12)) + F(2.0 ** -12)) == F(4096.0 * 4096.0)


def test_tie_goes_to_the_lowest_slot():
    p = np.array([[0.5, 0.5, 0.5]], F)
    frame = np.array([[0.5, 0.5, 0.6]], F)
    r = sm.subtract(frame, {9: (p, I), 4: (p, I), 30: (p, I)}, 0.25)
    assert r["owner"][0] == 4 and r["ties"][0]
    np.testing.assert_array_equal(np.flatnonzero(r["support"]), [4])
    # mirror images: equal d2 from two different points
    r = sm.subtract(np.array([[0, 0, 0]], F), {2: (np.array([[0.125, 0, 0]], F), I), 1: (np.array([[-0.125, 0, 0]], F), I)}, 0.25)
    assert r["owner"][0] == 1 and r["ties"][0]


def test_strict_gate_at_a_representable_boundary():
    model = np.zeros((1, 3), F)
    at = F(0.25)
    below = np.nextafter(at, F(0))
    frame = np.array([[at, 0, 0], [below, 0, 0], [0, -at, 0], [0, 0, -below]], F)
    r = sm.subtract(frame, {0: (model, I)}, 0.25)
    assert F(at * at) == F(0.0625)  # d2 == r^2 exactly: not explained
    np.testing.assert_array_equal(r["owner"], [-1, 0, -1, 0])
    np.testing.assert_array_equal(r["d2"], np.array([np.inf, below * below, np.inf, below * below], F))


def test_non_finite_points():
    model = np.zeros((1, 3), F)
    frame = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [0.01, 0, 0], [np.nan, np.nan, np.nan]], F)
    r = sm.subtract(frame, {0: (model, I)}, 0.25)
    np.testing.assert_array_equal(r["owner"], [-1, -1, -1, 0, -1])
    np.testing.assert_array_equal(r["residual_idx"], [0, 1, 2, 4])
    # a moved model point that is not finite explains nothing: here the matrix overflows the first point only
    big = np.array([[3e38, 0, 0], [0.01, 0, 0]], F)
    T = np.array([[4, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], F)
    assert not np.isfinite(sm.xform(T, big)[0]).all()
    r = sm.subtract(np.array([[0.04, 0, 0], [np.inf, 0, 0]], F), {0: (big, T)}, 0.25)
    np.testing.assert_array_equal(r["owner"], [0, -1])


def test_the_scenarios_hold_on_the_cpu():
    # 1. neighbour cells: along every one of the 26 directions the lengths chosen fall on both sides of the gate
    for where in sc.OFFSETS:
        for rotated in (False, True):
            c = sc.neighbour_case(where, rotated)
            r = sm.subtract(c["frame"], {0: (c["model"], c["T"])}, sc.R)
            for di, d in enumerate(sc.DIRECTIONS):
                if d == (0, 0, 0):
                    assert (r["owner"][c["direction"] == di] == 0).all()
                    continue
                sel = (c["direction"] == di) & c["outward"]
                assert (r["owner"][sel] == 0).any() and (r["owner"][sel] < 0).any(), (where, rotated, d)
    # 2. the degenerate slots each explain something, the empty one nothing
    c = sc.degenerate_case()
    r = sm.subtract(c["frame"], c["slots"], sc.R)
    assert all(r["support"][s] > 0 for s in (0, 5, 9)) and r["support"][12] == 0 and r["n_residual"] > 0
    # 3. ties between slots happen
    c = sc.many_slots_case()
    r = sm.subtract(c["frame"], c["slots"], sc.R)
    assert r["ties"].sum() >= 1 and (r["support"] > 0).sum() >= 60 and r["n_residual"] > 0
    # 4. a frame around one slot: both classes
    c = sc.sized_frame(1025)
    r = sm.subtract(c["frame"], c["slots"], sc.R)
    assert 0 < r["n_explained"] < 1025
    # 7. end to end: the full frame's clustering has a cluster on the tracked object, the residual's clustering has not
    w = sc.small_world()
    from pcl_tracking_amd import scene

    # (and the residual's clustering is not empty: the second object, which nothing tracks, is in both)
    frame = sc.small_frame(1, second=True)
    xyz = sm.xyz_of(frame)
    on_object = np.linalg.norm(xyz.astype(np.float64) - w["gt"], axis=1) < 0.3
    full = sg.clusters(xyz, **sc.SEGMENT)
    assert any(on_object[c].mean() > 0.9 for c in full) and len(full) >= 2
    r = sm.subtract(xyz, {0: (sm.xyz_of(scene.make_model(300)), w["trans"][:3])}, sc.R)
    res = sg.clusters(xyz[r["residual_idx"]], **sc.SEGMENT)
    assert len(res) >= 1 and not any(on_object[r["residual_idx"][c]].mean() > 0.5 for c in res)
    assert r["n_explained"] > 1000


# ---- the C ABI without a GPU ----
@pytest.fixture(scope="module")
def lib():
    from pcl_tracking_amd import _lib

    return _lib


def test_abi_defaults(lib):
    L = lib.load()
    c = lib.SubtractConfig()
    L.pft_subtract_default_config(C.byref(c))
    assert c.abi_version == lib.PFT_ABI_VERSION and c.device_id == 0 and c.cloud == lib.SUBTRACT_REFERENCE_CLOUD
    assert c.radius == F(0.02)  # the cluster tolerance of the model-creation nodes
    assert C.sizeof(lib.SubtractConfig) == 16
    hdr = open(__import__("os").path.join(__import__("os").path.dirname(__file__), "..", "include", "pft_subtract.h")).read()
    assert "PFT_SUBTRACT_MAX_OBJECTS = %d" % lib.SUBTRACT_MAX_OBJECTS in hdr
    assert lib.SUBTRACT_MAX_OBJECTS == sm.MAX_OBJECTS == 64


def test_abi_refusals_without_a_handle(lib):
    L = lib.load()
    h = C.c_void_p()
    c = lib.SubtractConfig()
    L.pft_subtract_default_config(C.byref(c))
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        c.radius = bad
        assert L.pft_subtract_create(C.byref(c), C.byref(h)) == 1 and not h.value
    c.radius = 0.02
    c.cloud = 2
    assert L.pft_subtract_create(C.byref(c), C.byref(h)) == 1 and not h.value
    c.cloud = 0
    c.abi_version = lib.PFT_ABI_VERSION + 1
    assert L.pft_subtract_create(C.byref(c), C.byref(h)) == 1 and not h.value
    assert L.pft_subtract_create(None, C.byref(h)) == 1
    # a null handle is an invalid argument everywhere, and destroy takes it
    n = C.c_size_t()
    m = (C.c_float * 12)()
    assert L.pft_subtract_apply(None, None, 0) == 1
    assert L.pft_subtract_counts(None, C.byref(n), None, None) == 1
    assert L.pft_subtract_set_object(None, 0, None, 0, m) == 1
    assert L.pft_subtract_bind_tracker(None, 0, None) == 1
    assert L.pft_subtract_get_object(None, 0, m, None, 0, C.byref(n)) == 1
    assert L.pft_subtract_clear(None) == 1
    L.pft_subtract_destroy(None)
    assert L.pft_subtract_last_error_string(None) == b"null handle"


def test_no_gpu_means_loud_failure(lib):
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from pcl_tracking_amd import subtract

    with pytest.raises(lib.PftError) as e:
        subtract.SceneSubtraction()
    assert e.value.status == 4  # PFT_ERR_NO_DEVICE: there is no CPU path
