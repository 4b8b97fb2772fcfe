"""CPU checks of the population statistics (pft_spread): the ABI struct, the new symbols, the
mirrors, the C++ driver's flag, known answers of the NumPy restatement (tests/spread_model.py), and the one-lane
finalisation header (csrc/pft_spread_final.h) compiled into a stand-alone program and compared with the model byte for byte.
The device is compared with the model in tests/test_gpu_spread.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import match_model as mm
import spread_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "spread_final_tool.cpp")
NEW_SYMBOLS = ("pft_set_spread_threshold", "pft_get_spread_threshold", "pft_spread", "pft_get_spread")
MIRROR_CALLS = ("setSpreadThreshold", "computeSpread", "getSpread", "isUncertain")
# (field, bytes)
FIELDS = [("sum_w", 8), ("sum_w2", 8), ("s", 48), ("S", 168), ("n_eff", 8), ("mean", 48), ("cov", 288), ("rpy_sigma", 24),
          ("pos_sigma", 12), ("pos_axes", 36), ("w_max", 4), ("n", 4), ("n_zero", 4), ("i_max", 4), ("solve_info", 4),
          ("evaluated", 4), ("uncertain", 4), ("streak", 4), ("flagged", 4), ("calls", 4)]
PARTICLE = np.dtype([("x", "f4"), ("y", "f4"), ("z", "f4"), ("w", "f4"), ("roll", "f4"), ("pitch", "f4"), ("yaw", "f4"),
                     ("weight", "f4")])
CASE = np.dtype([("sums", "f8", 29), ("max_pos_sigma", "f8"), ("min_n_eff", "f8"), ("pivot", "f4", 6), ("w_max", "f4"),
                 ("n", "u4"), ("n_zero", "u4"), ("i_max", "u4"), ("after", "u4"), ("prev_streak", "u4")])


def population(poses, weights):
    p = np.zeros(len(weights), PARTICLE)
    poses = np.asarray(poses, np.float32).reshape(len(weights), 6)
    for a, k in enumerate(sm.POSE):
        p[k] = poses[:, a]
    p["w"] = 1.0
    p["weight"] = np.asarray(weights, np.float32)
    return p


def pose(v):
    r = np.zeros(1, PARTICLE)[0]
    for a, k in enumerate(sm.POSE):
        r[k] = v[a]
    return r


# ---- the ABI ----------------------------------------------------------------------------------------------------------
def test_spread_struct_layout(tmp_path):
    """pft_population_stats: 688 bytes, fields in order without gaps, the same in C (compiled here) and in ctypes"""
    from pcl_tracking_amd import _lib

    off, want = 0, {}
    for name, n in FIELDS:
        want[name] = off
        off += n
    assert off == 688 and want["n_eff"] == 232 and want["cov"] == 288 and want["pos_sigma"] == 600 and want["calls"] == 684
    assert C.sizeof(_lib.PopulationStatsStruct) == 688
    for name, _ in FIELDS:
        assert getattr(_lib.PopulationStatsStruct, name).offset == want[name], name
    src = tmp_path / "layout.c"
    src.write_text("#include <stddef.h>\n#include <stdio.h>\n#include \"pft.h\"\nint main(void) {\n"
                   "  printf(\"size %zu\\n\", sizeof(pft_population_stats));\n" +
                   "".join("  printf(\"%s %%zu\\n\", offsetof(pft_population_stats, %s));\n" % (f, f) for f, _ in FIELDS) +
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["size"]) == 688
    for name, _ in FIELDS:
        assert int(got[name]) == want[name], name


def test_spread_symbols_are_declared_exported_and_bound():
    from pcl_tracking_amd import _lib

    header = open(os.path.join(ROOT, "include", "pft.h")).read()
    L = _lib.load()
    bound = {n: (res, args) for n, res, args in _lib.SYMBOLS}
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert hasattr(L, name), name
        assert name in bound and bound[name][0] is C.c_int, name
    assert "PFT_ABI_VERSION 5" in header, "pft_config and the ABI version stay as they are"
    assert "} pft_population_stats;" in header


def test_spread_thresholds_are_validated_without_a_handle():
    from pcl_tracking_amd import tracker
    from pcl_tracking_amd._lib import PftError

    t = tracker.ParticleFilterTracker()
    assert t.getSpreadThreshold() == (float("inf"), 0.0, 1)  # never fires
    t.setSpreadThreshold(0.05, 20.0, 3)
    assert t.getSpreadThreshold() == (0.05, 20.0, 3)
    for bad in ((-0.1, 0.0, 1), (0.1, -1.0, 1), (0.1, 0.0, 0), (float("nan"), 0.0, 1), (0.1, float("nan"), 1)):
        with pytest.raises(PftError) as e:
            t.setSpreadThreshold(*bad)
        assert e.value.status == 1
    assert t.getSpreadThreshold() == (0.05, 20.0, 3)
    for call in ("computeSpread", "getSpread", "isUncertain"):
        with pytest.raises(PftError) as e:
            getattr(t, call)()
        assert e.value.status == 7


def test_python_and_cpp_mirrors_have_the_spread_calls():
    from pcl_tracking_amd import tracker

    for m in MIRROR_CALLS:
        assert callable(getattr(tracker.ParticleFilterTracker, m)), m
    hpp = open(os.path.join(ROOT, "pcl_tracking_amd", "include", "pft", "particle_filter_tracker.hpp")).read()
    for m in MIRROR_CALLS:
        assert re.search(r"\b%s\(" % m, hpp), m
    app = open(os.path.join(ROOT, "pcl_tracking_amd", "examples", "tracking_app.hpp")).read()
    assert "reportSpread(" in app


def test_population_stats_from_struct():
    from pcl_tracking_amd import _lib, tracker

    r = _lib.PopulationStatsStruct()
    for k in range(36):
        r.cov[k] = float(k)
    for k in range(9):
        r.pos_axes[k] = float(k)
    r.n_eff, r.n, r.n_zero, r.i_max, r.flagged, r.evaluated = 12.5, 64, 3, 7, 1, 1
    p = tracker.PopulationStats.from_struct(r)
    assert p.cov.shape == (6, 6) and p.cov[5, 4] == 34.0 and p.pos_axes.shape == (3, 3) and p.pos_axes[2, 1] == 7.0
    assert p.cov.dtype == np.float64 and p.pos_sigma.dtype == np.float32 and p.S.shape == (21,) and p.s.shape == (6,)
    assert (p.n_eff, p.n, p.n_zero, p.i_max, p.flagged, p.evaluated, p.uncertain) == (12.5, 64, 3, 7, True, True, False)


def test_cpp_driver_compiles_with_the_spread_flag():
    from pcl_tracking_amd import build

    exe = build.build_example()
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "--spread[=max_pos_sigma[,min_n_eff[,after]]]" in r.stderr
    for bad in (["--spread=-1"], ["--spread=0.1,-2"], ["--spread=0.1,2,0"], ["--spread=x"]):
        r = subprocess.run([exe, "m.bin", "--frames", "f.bin"] + bad, capture_output=True, text=True)
        assert r.returncode == 2 and "max_pos_sigma" in r.stderr, bad
    src = open(os.path.join(ROOT, "pcl_tracking_amd", "examples", "auto_tracking_amd.cpp")).read()
    assert "computeSpread()" in src and "reportSpread(" in src


def test_spread_source_is_part_of_the_build():
    from pcl_tracking_amd import build

    assert "pft_spread.hip" in build.SOURCES and "pft_spread_final.h" in build.HEADERS
    assert os.path.exists(os.path.join(build.CSRC, "pft_spread.hip"))
    internal = open(os.path.join(build.CSRC, "pft_internal.h")).read()
    assert re.search(r"\bvoid pftk_spread\(", internal)


# ---- the model's known answers ------------------------------------------------------------------------------------------
def test_two_particles_by_hand():
    """weights 0.25 / 0.75 at x = 1 and x = 3 (y = -2 and 2, yaw = 0.5 and -0.5) around the pivot (2, 0, 0, 0, 0, 0): every
    value is a small dyadic number, so the expected results are exact"""
    p = population([[1, -2, 0, 0, 0, 0.5], [3, 2, 0, 0, 0, -0.5]], [0.25, 0.75])
    r = sm.stats(p, pose([2, 0, 0, 0, 0, 0]))
    assert (r["n"], r["n_zero"], r["i_max"], float(r["w_max"])) == (2, 0, 1, 0.75)
    assert r["sum_w"] == 1.0 and r["sum_w2"] == 0.625 and r["n_eff"] == 1.6
    # d = (-1, -2, ., ., ., 0.5) and (1, 2, ., ., ., -0.5):  s = 0.25 d0 + 0.75 d1
    assert r["s"].tolist() == [0.5, 1.0, 0.0, 0.0, 0.0, -0.25]
    assert r["mean"].tolist() == [2.5, 1.0, 0.0, 0.0, 0.0, -0.25]
    # S_kl = d_k d_l for both particles (their offsets are opposite), so cov = d_k d_l - m_k m_l
    cov = np.zeros((6, 6))
    d, m = np.array([1.0, 2.0, 0, 0, 0, -0.5]), np.array([0.5, 1.0, 0, 0, 0, -0.25])
    cov = np.outer(d, d) - np.outer(m, m)
    assert r["cov"].tolist() == cov.tolist() and r["cov"][0, 0] == 0.75 and r["cov"][0, 1] == 1.5 and r["cov"][5, 5] == 0.1875
    assert r["S"][sm.tri(0, 1)] == 2.0 and r["S"][sm.tri(1, 5)] == -1.0
    assert r["rpy_sigma"].tolist() == [0.0, 0.0, np.sqrt(0.1875)]
    # the position block is rank one along (1, 2, 0) / sqrt(5) with variance 0.75 + 3 = 3.75
    assert r["solve_info"] == 0 and abs(float(r["pos_sigma"][2]) - np.sqrt(3.75)) < 1e-6
    assert float(r["pos_sigma"][0]) < 1e-3 and float(r["pos_sigma"][1]) < 1e-3
    ax = r["pos_axes"][:, 2].astype(np.float64)
    assert abs(abs(ax @ np.array([1.0, 2.0, 0.0]) / np.sqrt(5.0)) - 1.0) < 1e-6
    assert (r["evaluated"], r["uncertain"], r["streak"], r["flagged"]) == (1, 0, 0, 0)


def test_single_mass_population():
    rng = np.random.default_rng(5)
    poses = rng.normal(0.0, 0.1, (9, 6))
    w = np.zeros(9)
    w[6] = 1.0
    r = sm.stats(population(poses, w), pose(rng.normal(0.0, 0.1, 6)))
    assert r["n_eff"] == 1.0 and r["n_zero"] == 8 and r["i_max"] == 6 and float(r["w_max"]) == 1.0
    assert not r["cov"].any() and not r["pos_sigma"].any() and not r["rpy_sigma"].any()
    assert np.allclose(r["mean"], poses[6].astype(np.float32), rtol=0, atol=1e-12)  # pivot + (p - pivot)


def test_uniform_population():
    rng = np.random.default_rng(6)
    for n in (1, 2, 64, 256):  # 1 / n is exact in float
        r = sm.stats(population(rng.normal(0.0, 0.05, (n, 6)), np.full(n, 1.0 / n)), pose(np.zeros(6)))
        assert r["n_eff"] == float(n) and r["sum_w"] == 1.0 and r["n_zero"] == 0 and r["i_max"] == 0
    n = 400  # 1 / 400 is not: n_eff = (n w)^2 / (n w^2) within rounding
    r = sm.stats(population(rng.normal(0.0, 0.05, (n, 6)), np.full(n, 1.0 / n)), pose(np.zeros(6)))
    assert abs(r["n_eff"] - n) < 1e-9 * n and r["i_max"] == 0
    assert abs(float(r["pos_sigma"][2]) - 0.05) < 0.02


def test_all_weights_zero():
    rng = np.random.default_rng(7)
    r = sm.stats(population(rng.normal(0.0, 0.1, (33, 6)), np.zeros(33)), pose(np.zeros(6)), max_pos_sigma=0.5, min_n_eff=2.0)
    assert r["evaluated"] == 1 and r["n_zero"] == 33 and r["n"] == 33 and r["i_max"] == 0 and float(r["w_max"]) == 0.0
    assert r["sum_w"] == 0.0 and r["n_eff"] == 0.0 and r["solve_info"] == 0
    for f in ("mean", "cov", "rpy_sigma", "pos_sigma", "pos_axes"):
        assert not np.asarray(r[f]).any(), f
    assert (r["uncertain"], r["streak"], r["flagged"]) == (1, 1, 1)  # n_eff 0 < 2
    # the sign of a zero sum follows the tree: one particle left of the pivot gives -0.0, the padding of three gives +0.0
    one = sm.stats(population([[-1, 0, 0, 0, 0, 0]], [0.0]), pose(np.zeros(6)))
    assert np.signbit(one["s"][0]) and not np.signbit(one["s"][1])
    three = sm.stats(population([[-1, 0, 0, 0, 0, 0]] * 3, [0.0] * 3), pose(np.zeros(6)))
    assert not np.signbit(three["s"][0])


def test_equal_maxima_take_the_lowest_index():
    p = population(np.zeros((6, 6)), [0.1, 0.3, 0.2, 0.3, 0.1, 0.0])
    n, n_zero, w_max, i_max = sm.integers(p)
    assert (n, n_zero, i_max) == (6, 1, 1) and w_max == np.float32(0.3)
    assert sm.integers(p[:0]) == (0, 0, np.float32(0), 0)


def test_pivot_keeps_large_coordinates_exact():
    """coordinates of 10^3 m: around the representative state the offsets are small and the covariance is what the same
    cloud gives at the origin"""
    rng = np.random.default_rng(8)
    off = (rng.integers(-64, 65, (40, 6)) / 1024.0)  # dyadic offsets: exact in float at 1024 as well
    w = np.full(40, 1.0 / 64)
    near = sm.stats(population(off, w), pose(np.zeros(6)))
    far_poses = off.copy()
    far_poses[:, :3] += 1024.0
    far = sm.stats(population(far_poses, w), pose([1024.0, 1024.0, 1024.0, 0, 0, 0]))
    assert sm.bits(far["cov"]).tolist() == sm.bits(near["cov"]).tolist()
    assert sm.bits(far["pos_sigma"]).tolist() == sm.bits(near["pos_sigma"]).tolist()
    assert np.isfinite(far["cov"]).all() and far["cov"][0, 0] > 0.0


def test_sums_are_the_adjacent_pair_tree():
    rng = np.random.default_rng(9)
    p = population(rng.normal(0.0, 0.1, (37, 6)), rng.uniform(0.0, 1.0, 37))
    s = sm.sums(p, [np.float32(0)] * 6)
    w = p["weight"].astype(np.float64)
    assert s[0] == mm.tree_sum(w) and s[1] == mm.tree_sum(w * w)
    x, y = p["x"].astype(np.float64), p["y"].astype(np.float64)
    assert s[8 + sm.tri(0, 1)] == mm.tree_sum((w * x) * y)
    assert len(sm.SUM_NAMES) == sm.N_SUMS == 29 and sm.tri(5, 5) == 20 and sm.tri(0, 5) == 5 and sm.tri(1, 1) == 6


def test_spread_rule_hand_sequences():
    rule = sm.SpreadRule(max_pos_sigma=0.0625, min_n_eff=10.0, after=2)  # (a threshold a float sigma can equal)
    seq = [(0.01, 50.0), (0.07, 50.0), (0.01, 5.0), (0.01, 50.0), (0.0625, 10.0), (0.2, 1.0), (0.2, 1.0)]
    got = [rule.step(*v) for v in seq]
    assert got == [(False, 0, False), (True, 1, False), (True, 2, True), (False, 0, False), (False, 0, False),
                   (True, 1, False), (True, 2, True)]  # equality with either threshold is not uncertain
    # a call that was not evaluated keeps the state; reset clears it
    assert rule.step(0.0, 100.0, evaluated=False) == (True, 2, True)
    rule.reset()
    assert (rule.uncertain, rule.streak, rule.flagged) == (False, 0, False)
    # the defaults never fire
    assert all(sm.SpreadRule().step(s, n) == (False, 0, False) for s, n in ((1e9, 0.0), (0.0, 0.0), (3.0, 1.0)))
    # the rule inside stats(): the previous streak is carried
    p = population([[0, 0, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0]], [0.5, 0.5])
    r = sm.stats(p, pose(np.zeros(6)), max_pos_sigma=0.25, after=3, prev_streak=2)
    assert float(r["pos_sigma"][2]) == 0.5 and (r["uncertain"], r["streak"], r["flagged"]) == (1, 3, 1)
    r = sm.stats(p, pose(np.zeros(6)), max_pos_sigma=0.5, after=3, prev_streak=2)
    assert (r["uncertain"], r["streak"], r["flagged"]) == (0, 0, 0)


# ---- the one-lane finalisation header on the host --------------------------------------------------------------------
def _compile(out, extra=()):
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off", *extra, "-I",
                    os.path.join(ROOT, "pcl_tracking_amd", "csrc"), SRC, "-o", out], check=True)
    return out


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    return _compile(str(tmp_path_factory.mktemp("spread") / "spread_final_tool"))


def finalisation_cases():
    """(label, particles, pivot pose, thresholds, previous streak): the 29 sums come from the model's tree"""
    rng = np.random.default_rng(11)
    cases = []
    for n in (1, 2, 3, 64, 257):
        poses = rng.normal(0.0, 0.05, (n, 6)) + np.array([0.3, -0.2, 1.1, 0.1, -0.4, 2.0])
        w = rng.uniform(0.0, 1.0, n)
        w[rng.uniform(size=n) < 0.3] = 0.0
        w = w / max(w.sum(), 1e-30)
        cases.append(("random n=%d" % n, population(poses, w), pose([0.3, -0.2, 1.1, 0.1, -0.4, 2.0]), (0.04, n / 3.0, 2), 1))
    cases.append(("all zero", population(rng.normal(0, 0.1, (5, 6)), np.zeros(5)), pose(np.zeros(6)), (0.1, 1.0, 1), 7))
    one = np.zeros(9)
    one[4] = 1.0
    cases.append(("single mass", population(rng.normal(0, 0.1, (9, 6)), one), pose(rng.normal(0, 0.1, 6)), (np.inf, 0.0, 1), 0))
    cases.append(("uniform", population(rng.normal(0, 0.02, (128, 6)), np.full(128, 1 / 128)), pose(np.zeros(6)), (0.01, 0.0, 1), 0))
    far = rng.normal(0.0, 0.03, (50, 6))
    far[:, :3] += 1000.0
    cases.append(("10^3 m", population(far, rng.uniform(0, 1, 50)), pose([1000.0, 1000.0, 1000.0, 0, 0, 0]), (np.inf, 0.0, 1), 0))
    line = np.zeros((16, 6))
    line[:, 1] = np.linspace(-0.1, 0.1, 16)
    cases.append(("degenerate line", population(line, np.full(16, 1 / 16)), pose(np.zeros(6)), (0.05, 0.0, 1), 0xffffffff))
    return cases


def run_tool(exe, cases, tmp_path):
    rec = np.zeros(len(cases), CASE)
    want = []
    for i, (_, p, piv, thr, prev) in enumerate(cases):
        pivot = [np.float32(piv[k]) for k in sm.POSE]
        n, n_zero, w_max, i_max = sm.integers(p)
        sums = sm.sums(p, pivot)
        rec[i] = (sums, thr[0], thr[1], pivot, w_max, n, n_zero, i_max, thr[2], prev)
        want.append(sm.finalize(sums, n, n_zero, w_max, i_max, pivot, thr[0], thr[1], thr[2], prev))
    assert CASE.itemsize == 296
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    rec.tofile(fin)
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    from pcl_tracking_amd import _lib, tracker

    blob = open(fout, "rb").read()
    assert len(blob) == 688 * len(cases)
    got = [tracker.PopulationStats.from_struct(_lib.PopulationStatsStruct.from_buffer_copy(blob[688 * i:688 * (i + 1)]))
           for i in range(len(cases))]
    return got, want


def test_finalisation_header_equals_the_model(tool, tmp_path):
    cases = finalisation_cases()
    got, want = run_tool(tool, cases, tmp_path)
    bad = []
    for (label, *_), g, w in zip(cases, got, want):
        if label.startswith("degenerate"):  # a saturated streak stays saturated on the device; the model counts on
            assert g.streak == 0xffffffff and g.flagged and g.uncertain
            w = dict(w, streak=0xffffffff)
        bad += sm.compare(g, w, label)
        assert g.calls == 0
    assert not bad, bad[:5]


def test_finalisation_header_under_sanitizers(tmp_path):
    """the same program built with the address and undefined-behaviour sanitizers, as a program of its own"""
    san = _compile(str(tmp_path / "spread_final_tool_san"),
                   ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"))
    cases = finalisation_cases()
    got, want = run_tool(san, cases, tmp_path)
    for (label, *_), g, w in zip(cases, got, want):
        if not label.startswith("degenerate"):
            assert not sm.compare(g, w, label), label
