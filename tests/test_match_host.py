"""CPU checks of the match statistics (pft_match): the ABI struct, the new symbols, the mirrors,
the C++ driver's flags, and known answers of the NumPy restatement (tests/match_model.py) -- the lost rule on hand-written
sequences and the tree sum.  The device is compared with the oracle and the model in tests/test_gpu_match.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import match_model as mm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pft_set_match_threshold", "pft_get_match_threshold", "pft_match", "pft_get_match", "pft_get_match_pairs",
               "pft_reset_tracking")
MIRROR_CALLS = ("setMatchThreshold", "computeMatch", "getMatch", "getMatchPairs", "isLost", "resetTracking")
# (field, bytes)
FIELDS = [("transform", 48), ("coherence", 8), ("sum_sq_dist", 8), ("n_reference", 4), ("n_matched", 4), ("n_crop", 4),
          ("evaluated", 4), ("below", 4), ("streak", 4), ("lost", 4), ("calls", 4)]


# ---- the ABI ----------------------------------------------------------------------------------------------------------
def test_match_struct_layout(tmp_path):
    """pft_match_stats: 96 bytes, fields in order without gaps, the same in C (compiled here) and in ctypes"""
    from pcl_tracking_amd import _lib

    off, want = 0, {}
    for name, n in FIELDS:
        want[name] = off
        off += n
    assert off == 96 and want["coherence"] == 48 and want["n_reference"] == 64 and want["calls"] == 92
    assert C.sizeof(_lib.MatchStatsStruct) == 96
    for name, _ in FIELDS:
        assert getattr(_lib.MatchStatsStruct, name).offset == want[name], name
    src = tmp_path / "layout.c"
    src.write_text("#include <stddef.h>\n#include <stdio.h>\n#include \"pft.h\"\nint main(void) {\n"
                   "  printf(\"size %zu\\n\", sizeof(pft_match_stats));\n" +
                   "".join("  printf(\"%s %%zu\\n\", offsetof(pft_match_stats, %s));\n" % (f, f) for f, _ in FIELDS) +
                   "  printf(\"lost_status %d\\n\", (int)PFT_ERR_LOST);\n  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["size"]) == 96
    for name, _ in FIELDS:
        assert int(got[name]) == want[name], name
    assert int(got["lost_status"]) == 8


def test_match_symbols_are_declared_exported_and_bound():
    from pcl_tracking_amd import _lib

    header = open(os.path.join(ROOT, "include", "pft.h")).read()
    L = _lib.load()
    bound = {n: (res, args) for n, res, args in _lib.SYMBOLS}
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert hasattr(L, name), name
        assert name in bound and bound[name][0] is C.c_int, name
    assert "PFT_ABI_VERSION 5" in header, "pft_config and the ABI version stay as they are"
    assert L.pft_status_string(8) == b"object not recognized"
    assert _lib.STATUS[8] == "object not recognized"


def test_thresholds_are_validated_without_a_handle():
    from pcl_tracking_amd import tracker
    from pcl_tracking_amd._lib import PftError

    t = tracker.ParticleFilterTracker()
    assert t.getMatchThreshold() == (0.0, 1)
    t.setMatchThreshold(0.5, 3)
    assert t.getMatchThreshold() == (0.5, 3)
    for bad in ((-0.1, 1), (1.5, 1), (0.5, 0), (float("nan"), 1)):
        with pytest.raises(PftError) as e:
            t.setMatchThreshold(*bad)
        assert e.value.status == 1
    assert t.getMatchThreshold() == (0.5, 3)
    for call in ("computeMatch", "getMatch", "getMatchPairs"):
        with pytest.raises(PftError) as e:
            getattr(t, call)()
        assert e.value.status == 7
    t.resetTracking()  # without a handle there is nothing to forget


def test_match_stats_derived_values():
    from pcl_tracking_amd import _lib, tracker

    r = _lib.MatchStatsStruct()
    r.n_reference, r.n_matched, r.sum_sq_dist, r.evaluated, r.lost = 300, 75, 75 * 0.0004, 1, 1
    for k in range(12):
        r.transform[k] = float(k)
    m = tracker.MatchStats.from_struct(r)
    assert m.ratio == 0.25 and abs(m.rms_distance - 0.02) < 1e-15 and m.evaluated and m.lost and not m.below
    assert m.transform.shape == (3, 4) and m.transform[2, 3] == 11.0
    r.n_matched, r.n_reference = 0, 0
    m = tracker.MatchStats.from_struct(r)
    assert m.ratio == 0.0 and np.isnan(m.rms_distance)


def test_python_and_cpp_mirrors_have_the_match_calls():
    from pcl_tracking_amd import tracker

    for m in MIRROR_CALLS:
        assert callable(getattr(tracker.ParticleFilterTracker, m)), m
    assert {"ratio", "rms_distance"} <= set(dir(tracker.MatchStats))
    hpp = open(os.path.join(ROOT, "pcl_tracking_amd", "include", "pft", "particle_filter_tracker.hpp")).read()
    for m in MIRROR_CALLS:
        assert re.search(r"\b%s\(" % m, hpp), m
    assert "PFT_ERR_LOST" in hpp
    app = open(os.path.join(ROOT, "pcl_tracking_amd", "examples", "tracking_app.hpp")).read()
    assert "reportMatch(" in app and "resetTracking()" in app


def test_cpp_driver_compiles_with_the_match_flags():
    from pcl_tracking_amd import build

    exe = build.build_example()
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "--match[=min_ratio[,lost_after]]" in r.stderr and "--reset-on-loss" in r.stderr
    for bad in (["--match=2"], ["--match=0.5,0"], ["--match=x"]):
        r = subprocess.run([exe, "m.bin", "--frames", "f.bin"] + bad, capture_output=True, text=True)
        assert r.returncode == 2 and "min_ratio" in r.stderr, bad
    r = subprocess.run([exe, "m.bin", "--frames", "f.bin", "--reset-on-loss"], capture_output=True, text=True)
    assert r.returncode == 2 and "--reset-on-loss needs --match" in r.stderr
    src = open(os.path.join(ROOT, "pcl_tracking_amd", "examples", "auto_tracking_amd.cpp")).read()
    assert "computeMatch()" in src and "reportMatch(" in src


def test_match_source_is_part_of_the_build():
    from pcl_tracking_amd import build

    assert "pft_match.hip" in build.SOURCES
    assert "pft_match_search.h" in build.HEADERS and "pft_pair_tree.h" in build.HEADERS
    for h in ("pft_match_search.h", "pft_pair_tree.h"):
        assert os.path.exists(os.path.join(build.CSRC, h))
    assert os.path.exists(os.path.join(build.CSRC, "pft_match.hip"))
    internal = open(os.path.join(build.CSRC, "pft_internal.h")).read()
    assert re.search(r"\bvoid pftk_match\(", internal)


# ---- the model's known answers ------------------------------------------------------------------------------------------
def run_rule(rule, counts, M, evaluated=None):
    evaluated = [True] * len(counts) if evaluated is None else evaluated
    return [rule.step(n, M, e) for n, e in zip(counts, evaluated)]


def test_lost_rule_hand_sequences():
    counts = [280, 290, 10, 20, 5, 0, 270, 30, 280]
    got = run_rule(mm.LostRule(0.5, 1), counts, 300)
    assert got == [(False, 0, False), (False, 0, False), (True, 1, True), (True, 2, True), (True, 3, True),
                   (True, 4, True), (False, 0, False), (True, 1, True), (False, 0, False)]
    got = run_rule(mm.LostRule(0.5, 3), counts, 300)
    assert [g[2] for g in got] == [False, False, False, False, True, True, False, False, False]
    assert [g[1] for g in got] == [0, 0, 1, 2, 3, 4, 0, 1, 0]


def test_lost_rule_min_ratio_zero_and_one():
    assert all(g == (False, 0, False) for g in run_rule(mm.LostRule(0.0, 1), [0, 0, 300, 1], 300))  # never below
    got = run_rule(mm.LostRule(1.0, 2), [300, 299, 299, 300, 0], 300)  # below unless every point matched
    assert got == [(False, 0, False), (True, 1, False), (True, 2, True), (False, 0, False), (True, 1, False)]
    assert mm.LostRule(0.0, 1).step(0, 0) == (False, 0, False)  # an empty reference is never below at ratio 0


def test_lost_rule_equality_is_not_below():
    assert mm.LostRule(0.5, 1).step(150, 300) == (False, 0, False)  # n_matched == min_ratio * M
    assert mm.LostRule(0.5, 1).step(149, 300) == (True, 1, True)
    assert mm.LostRule(0.25, 1).step(256, 1024) == (False, 0, False)
    # the product is formed in double: 0.55 * 100 = 55.00000000000001 > 55, 0.7 * 90 = 62.99999999999999 < 63
    assert mm.LostRule(0.55, 1).step(55, 100) == (True, 1, True)
    assert mm.LostRule(0.7, 1).step(63, 90) == (False, 0, False)


def test_lost_rule_unevaluated_frames_keep_the_state():
    r = mm.LostRule(0.5, 2)
    got = run_rule(r, [10, 0, 0, 10, 300], 300, [True, False, False, True, True])
    assert got == [(True, 1, False), (True, 1, False), (True, 1, False), (True, 2, True), (False, 0, False)]
    r.step(0, 300)
    r.reset()
    assert (r.below, r.streak, r.lost) == (False, 0, False)


def test_tree_sum_does_not_depend_on_padding():
    rng = np.random.default_rng(3)
    v = rng.uniform(0.0, 1.0, 1025)
    assert mm.tree_sum(v) == mm.tree_sum(np.concatenate([v, np.zeros(1023)]))
    assert mm.tree_sum(v) == mm.tree_sum(np.concatenate([v, np.zeros(3071)]))  # a deeper padded tree
    assert mm.tree_sum([]) == 0.0 and mm.tree_sum([0.25]) == 0.25
    # adjacent pairs, not a chain: ((a + b) + (c + d))
    a = [1.0, 2.0 ** -53, 2.0 ** -53, 2.0 ** -53]
    assert mm.tree_sum(a) == (1.0 + 2.0 ** -53) + (2.0 ** -53 + 2.0 ** -53) == 1.0 + 2.0 ** -52
    assert mm.chain_sum(a) == 1.0
    # both orders stay within M * 2^-53 of each other on non-negative terms
    assert abs(mm.tree_sum(v) - mm.chain_sum(v)) <= len(v) * 2.0 ** -53 * mm.chain_sum(v)


def test_stored_order_is_the_morton_order():
    from pcl_tracking_amd import scene

    # one point per octant of a unit cube, in reverse: x is the most significant bit of each triple
    xyz = np.array([[(c >> 2) & 1, (c >> 1) & 1, c & 1] for c in range(7, -1, -1)], np.float32)
    pts = scene.make_points(xyz, np.zeros((8, 3)))
    assert mm.stored_order(pts).tolist() == [7, 6, 5, 4, 3, 2, 1, 0]
    # equal codes keep the caller's order; a single point and a degenerate cloud are the identity
    same = scene.make_points(np.tile([[0.5, 0.5, 0.5]], (5, 1)).astype(np.float32), np.zeros((5, 3)))
    assert mm.stored_order(same).tolist() == [0, 1, 2, 3, 4]
    assert mm.stored_order(pts[:1]).tolist() == [0]
    # the quantisation is 1 024 steps of the LARGEST extent: y spans a tenth of x's range and so a tenth of the steps
    line = scene.make_points(np.array([[0.0, 0.1, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 0.0]], np.float32), np.zeros((3, 3)))
    assert mm.stored_order(line).tolist() == [2, 0, 1]
    order = mm.stored_order(scene.make_model(300))
    assert sorted(order.tolist()) == list(range(300))


def test_gate_is_the_likelihoods():
    assert mm.gate(0.1) == np.float64(0.1) * np.float64(0.1)
    assert np.float64(np.float32(0.01)) < mm.gate(0.1)  # float 0.01 rounds below 0.1 * 0.1 = 0.010000000000000002
