"""CPU checks of the re-acquisition step (pft_reacquire): the two ABI structs and the defaults, the new
symbols and mirrors, the driver's flag, known answers of the NumPy restatement (tests/reacquire_model.py) -- the lattice,
the selection rule and its ties -- and the scenario itself on the CPU oracle alone: the inlier count at 0.02 m tells the
object's centre from a decoy, and a tracker started from the selected pose keeps its object.  The device is compared with
the oracle and the model in tests/test_gpu_reacquire.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import match_model as mm
import reacquire_model as rm
import test_gpu_match as tgm
from pcl_tracking_amd import scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pft_reacquire", "pft_reacquire_from_segmenter", "pft_get_reacquire_scores")
CONFIG_FIELDS = [("n_roll", 0), ("n_pitch", 4), ("n_yaw", 8), ("base_rpy", 12), ("span_rpy", 24), ("inlier_distance", 40),
                 ("accept_ratio", 48), ("apply", 56)]
RESULT_FIELDS = [("n_centres", 0), ("n_candidates", 4), ("n_reference", 8), ("n_crop", 12), ("best", 16), ("best_centre", 20),
                 ("pose", 24), ("transform", 56), ("n_inliers", 104), ("n_matched", 108), ("accepted", 112), ("applied", 116),
                 ("coherence", 120), ("sum_sq_dist", 128), ("inlier_sq_dist", 136)]


# ---- the ABI ----------------------------------------------------------------------------------------------------------
def test_reacquire_struct_layouts(tmp_path):
    """pft_reacquire_config 64 bytes, pft_reacquire_result 144 bytes: the same in C (compiled here) and in ctypes"""
    from pcl_tracking_amd import _lib

    pairs = (("pft_reacquire_config", _lib.ReacquireConfig, CONFIG_FIELDS, 64),
             ("pft_reacquire_result", _lib.ReacquireResultStruct, RESULT_FIELDS, 144))
    body = ""
    for cname, ct, fields, size in pairs:
        assert C.sizeof(ct) == size, cname
        for f, off in fields:
            assert getattr(ct, f).offset == off, (cname, f)
        body += "  printf(\"%s.size %%zu\\n\", sizeof(%s));\n" % (cname, cname)
        body += "".join("  printf(\"%s.%s %%zu\\n\", offsetof(%s, %s));\n" % (cname, f, cname, f) for f, _ in fields)
    src = tmp_path / "layout.c"
    src.write_text("#include <stddef.h>\n#include <stdio.h>\n#include \"pft.h\"\nint main(void) {\n" + body +
                   "  printf(\"cap %d\\n\", (int)PFT_REACQUIRE_MAX_CANDIDATES);\n  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    for cname, _, fields, size in pairs:
        assert int(got[cname + ".size"]) == size
        for f, off in fields:
            assert int(got["%s.%s" % (cname, f)]) == off, (cname, f)
    assert int(got["cap"]) == 65536 == _lib.PFT_REACQUIRE_MAX_CANDIDATES


def test_reacquire_config_defaults():
    from pcl_tracking_amd import _lib

    c = _lib.ReacquireConfig()
    _lib.load().pft_reacquire_config_default(C.byref(c))
    assert (c.n_roll, c.n_pitch, c.n_yaw) == (1, 1, 8)
    assert list(c.base_rpy) == [0.0, 0.0, 0.0]
    assert list(c.span_rpy) == [0.0, 0.0, float(np.float32(2.0 * np.pi))]
    assert c.inlier_distance == 0.02 and c.accept_ratio == 0.5 and c.apply == 1


def test_reacquire_symbols_are_declared_exported_and_bound():
    from pcl_tracking_amd import _lib

    header = open(os.path.join(ROOT, "include", "pft.h")).read()
    L = _lib.load()
    bound = {n: (res, args) for n, res, args in _lib.SYMBOLS}
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert hasattr(L, name), name
        assert name in bound and bound[name][0] is C.c_int, name
    assert re.search(r"\bvoid pft_reacquire_config_default\(", header) and hasattr(L, "pft_reacquire_config_default")
    assert "PFT_ABI_VERSION 5" in header, "pft_config and the ABI version stay as they are"


def test_mirrors_driver_and_build_have_the_feature():
    from pcl_tracking_amd import build, tracker

    for m in ("reacquire", "getReacquireScores"):
        assert callable(getattr(tracker.ParticleFilterTracker, m)), m
    hpp = open(os.path.join(ROOT, "pcl_tracking_amd", "include", "pft", "particle_filter_tracker.hpp")).read()
    for m in ("reacquire", "reacquireFromSegmenter"):
        assert re.search(r"\bint %s\(" % m, hpp), m
    assert "pft_reacquire.hip" in build.SOURCES
    exe = build.build_example()
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "--reacquire[=n_yaw[,accept_ratio[,inlier_distance]]]" in r.stderr
    r = subprocess.run([exe, "m.bin", "--frames", "f.bin", "--reacquire"], capture_output=True, text=True)
    assert r.returncode == 2 and "--reacquire needs --match" in r.stderr
    for bad in ("--reacquire=0", "--reacquire=8,1.5", "--reacquire=8,0.5,0", "--reacquire=x"):
        r = subprocess.run([exe, "m.bin", "--frames", "f.bin", "--match", bad], capture_output=True, text=True)
        assert r.returncode == 2 and "n_yaw" in r.stderr, bad


def test_python_arguments_are_checked_without_a_handle():
    from pcl_tracking_amd import tracker
    from pcl_tracking_amd._lib import PftError

    t = tracker.ParticleFilterTracker()
    for kw in (dict(), dict(centres=np.zeros((1, 3)), segmenter=object())):
        with pytest.raises(PftError) as e:
            t.reacquire(**kw)
        assert e.value.status == 1
    with pytest.raises(PftError) as e:
        t.getReacquireScores()
    assert e.value.status == 7


# ---- the lattice ------------------------------------------------------------------------------------------------------
def test_lattice_known_answers():
    assert rm.angles(0.3, 1.0, 1).tolist() == [float(np.float32(0.3))], "n = 1: the base itself, whatever the span"
    two = rm.angles(0.5, 1.0, 2)
    assert two.tolist() == [0.25, 0.75]
    full = rm.angles(0.0, 2.0 * np.pi, 8).astype(np.float64)
    assert np.allclose(full, 2.0 * np.pi * (np.arange(8) - 3.5) / 8.0, rtol=0, atol=1e-6)
    assert np.allclose(full, -full[::-1], rtol=0, atol=1e-6), "symmetric about the base"
    on_circle = np.sort(np.mod(full, 2.0 * np.pi))
    gaps = np.diff(np.concatenate([on_circle, on_circle[:1] + 2.0 * np.pi]))
    assert np.allclose(gaps, 2.0 * np.pi / 8.0, rtol=0, atol=1e-5), "a full-circle span has no duplicate"
    # the double expression, rounded once
    assert rm.angles(0.1, 0.7, 3)[2] == np.float32(np.float64(np.float32(0.1)) + np.float64(np.float32(0.7)) * (2.5 / 3.0 - 0.5))


def test_candidate_order():
    c = rm.candidates([[1, 2, 3], [4, 5, 6]], (2, 3, 4), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    assert len(c) == 48
    r, p, y = rm.angles(0, 1, 2), rm.angles(0, 1, 3), rm.angles(0, 1, 4)
    for cen in range(2):
        for ir in range(2):
            for ip in range(3):
                for iy in range(4):
                    k = ((cen * 2 + ir) * 3 + ip) * 4 + iy
                    assert (c[k]["x"], c[k]["roll"], c[k]["pitch"], c[k]["yaw"]) == ((1.0, 4.0)[cen], r[ir], p[ip], y[iy])
    assert (c["w"] == 1.0).all()


# ---- the selection ----------------------------------------------------------------------------------------------------
def test_selection_rule_and_ties():
    assert rm.select([], [], 300, 0.5) == (-1, False)
    assert rm.select([10, 200, 150], [0.1, 0.9, 0.0], 300, 0.5) == (1, True), "the inlier count comes first"
    assert rm.select([200, 200, 200], [0.3, 0.1, 0.2], 300, 0.5) == (1, True), "ties: the smaller inlier_sq_dist"
    assert rm.select([200, 200, 200], [0.3, 0.1, 0.1], 300, 0.5) == (1, True), "then the lowest index"
    assert rm.select([7, 7], [0.5, 0.5], 300, 0.5) == (0, False)
    assert rm.select([149], [0.0], 300, 0.5) == (0, False) and rm.select([150], [0.0], 300, 0.5) == (0, True)
    assert rm.select([0, 0], [0.0, 0.0], 300, 0.0) == (0, False), "never without an inlier"
    assert rm.select([1], [0.0], 300, 0.0) == (0, True)


# ---- the scenario on the CPU ------------------------------------------------------------------------------------------
def _scenario(orc):
    """the model of 300 points, frame 0 of test_gpu_match, three centres -- a background point, the object's position,
    another background point -- and 8 yaw steps around the ground-truth orientation"""
    w = tgm._world()
    ref, cloud = tgm.model(300), tgm.frame(0)
    xyz = np.stack([cloud["x"], cloud["y"], cloud["z"]], 1)
    far = np.flatnonzero(np.linalg.norm(xyz - w["gt"], axis=1) >= 0.6)
    gtp = scene.model_gt_pose()
    centres = np.stack([xyz[far[0]], np.array(gtp[:3], np.float32), xyz[far[len(far) // 2]]]).astype(np.float32)
    cand = rm.candidates(centres, (1, 1, 8), gtp[3:], (0.0, 0.0, 2.0 * np.pi))
    return ref, cloud, centres, cand


def test_the_scenario_holds_on_the_cpu(orc):
    ref, cloud, centres, cand = _scenario(orc)
    M = len(ref)
    cfg = orc.default_config(particle_num=tgm.P, threads=0, emulate_pcl_alloc=0)
    o = orc.Tracker(cfg)
    o.set_reference(ref)
    o.set_input(cloud)
    E = o.eval_weights(cand, want_nn=True)
    d2 = E["nn_d2"].astype(np.float64)
    ok = E["nn_idx"] >= 0
    inl = (ok & (d2 < np.float64(0.02) * np.float64(0.02))).sum(axis=1)
    gate = (ok & (d2 < mm.gate(cfg.max_distance))).sum(axis=1)
    print("within 0.1 m :", gate.reshape(3, 8).tolist())
    print("within 0.02 m:", inl.reshape(3, 8).tolist())
    isq = np.where(ok & (d2 < 0.0004), d2, 0.0).sum(axis=1)
    best, accepted = rm.select(inl, isq, M, 0.5)
    assert best // 8 == 1 and accepted, "the best candidate belongs to the object's centre"
    assert inl[best] >= 0.5 * M
    others = np.concatenate([inl[:8], inl[16:]])
    assert others.max() < 0.5 * M, "no decoy comes near"
    # a tracker started from the selected pose keeps the object
    p = cand[best]
    o = orc.Tracker(cfg)
    o.set_reference(ref)
    o.set_trans(orc.get_transformation(*(float(p[k]) for k in tgm.KEYS)))
    rule = mm.LostRule(0.5, 2)
    for f in range(1, 6):
        frame = tgm.frame(f)
        o.set_input(frame)
        assert o.compute() == 0
        R = o.eval_weights(np.array([o.get_result()]), want_nn=True)
        n = int(((R["nn_idx"][0] >= 0) & (R["nn_d2"][0].astype(np.float64) < mm.gate(cfg.max_distance))).sum())
        below, streak, lost = rule.step(n, M)
        print("frame %d: matched %d of %d" % (f, n, M))
        assert n >= 0.5 * M and not lost, f
