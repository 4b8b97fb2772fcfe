"""CPU checks of the pose refinement (pft_refine): the ABI structs and the defaults, the new symbols
and mirrors, the driver's flag, the one-lane solve header on the host against the NumPy restatement (tests/refine_model.py)
bit for bit -- also under the address and undefined-behaviour sanitizers --, known answers of the solve, and the scenario
itself on the CPU oracle alone: from the two lattice neighbours of the truth the refinement gains inliers and loses rotation
error.  The device is compared with the oracle and the model in tests/test_gpu_refine.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import match_model as mm
import refine_model as rfm
import test_gpu_match as tgm
from pcl_tracking_amd import scene
from test_reacquire_host import _scenario

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "refine_solve_tool.cpp")
NEW_SYMBOLS = ("pft_refine", "pft_get_refine_trace")
CONFIG_FIELDS = [("max_iterations", 0), ("min_pairs", 4), ("pair_distance", 8), ("inlier_distance", 16), ("margin", 24),
                 ("trans_eps", 32), ("rot_eps", 40), ("apply", 48)]
SCORE_FIELDS = [("n_pairs", 0), ("n_inliers", 4), ("sum_sq_dist", 8), ("inlier_sq_dist", 16)]
RESULT_FIELDS = [("status", 0), ("iterations", 4), ("n_reference", 8), ("n_crop", 12), ("bbox", 16), ("start", 64),
                 ("transform", 112), ("pose", 160), ("before", 192), ("after", 216), ("improved", 240), ("applied", 244)]
TRACE_FIELDS = [("transform", 0), ("n_pairs", 48), ("n_inliers", 52), ("sums", 56), ("step_t2", 192), ("step_r2", 200)]
CASE = np.dtype([("sums", "f8", 17), ("c", "f8", 3), ("start", "f4", 12), ("n", "u4"), ("pad", "u4")])
OUT = np.dtype([("Q0", "f8", 4), ("t0", "f8", 3), ("Q", "f8", 4), ("t", "f8", 3), ("dq", "f8", 4), ("step2", "f8", 2),
                ("T", "f4", 12), ("sweeps", "u4"), ("pad", "u4")])


# ---- the ABI ----------------------------------------------------------------------------------------------------------
def test_refine_struct_layouts(tmp_path):
    """pft_refine_config 56 bytes, pft_refine_score 24, pft_refine_result 248, pft_refine_trace_entry 208: the same in C
    (compiled here) and in ctypes"""
    from pcl_tracking_amd import _lib

    pairs = (("pft_refine_config", _lib.RefineConfig, CONFIG_FIELDS, 56), ("pft_refine_score", _lib.RefineScore, SCORE_FIELDS, 24),
             ("pft_refine_result", _lib.RefineResultStruct, RESULT_FIELDS, 248),
             ("pft_refine_trace_entry", _lib.RefineTraceEntry, TRACE_FIELDS, 208))
    body = ""
    for cname, ct, fields, size in pairs:
        assert C.sizeof(ct) == size, cname
        for f, off in fields:
            assert getattr(ct, f).offset == off, (cname, f)
        body += "  printf(\"%s.size %%zu\\n\", sizeof(%s));\n" % (cname, cname)
        body += "".join("  printf(\"%s.%s %%zu\\n\", offsetof(%s, %s));\n" % (cname, f, cname, f) for f, _ in fields)
    src = tmp_path / "layout.c"
    src.write_text("#include <stddef.h>\n#include <stdio.h>\n#include \"pft.h\"\nint main(void) {\n" + body +
                   "  printf(\"cap %d\\n\", (int)PFT_REFINE_MAX_ITERATIONS);\n  printf(\"sums %d\\n\", (int)PFT_REFINE_N_SUMS);\n"
                   "  printf(\"status %d%d%d\\n\", PFT_REFINE_CONVERGED, PFT_REFINE_MAX_ITERATIONS_REACHED, PFT_REFINE_TOO_FEW_PAIRS);\n"
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    for cname, _, fields, size in pairs:
        assert int(got[cname + ".size"]) == size
        for f, off in fields:
            assert int(got["%s.%s" % (cname, f)]) == off, (cname, f)
    assert int(got["cap"]) == 64 == _lib.PFT_REFINE_MAX_ITERATIONS
    assert int(got["sums"]) == 17 == _lib.PFT_REFINE_N_SUMS == rfm.N_SUMS
    assert got["status"] == "012" and _lib.REFINE_STATUS == ("CONVERGED", "MAX_ITERATIONS", "TOO_FEW_PAIRS")
    assert (rfm.CONVERGED, rfm.MAX_ITERATIONS, rfm.TOO_FEW_PAIRS) == (0, 1, 2)


def test_refine_config_defaults():
    from pcl_tracking_amd import _lib

    c = _lib.RefineConfig()
    _lib.load().pft_refine_config_default(C.byref(c))
    assert (c.max_iterations, c.min_pairs, c.apply) == (16, 3, 0)
    assert (c.pair_distance, c.inlier_distance, c.margin, c.trans_eps, c.rot_eps) == (0.0, 0.02, 0.0, 1e-4, 1e-3)


def test_refine_symbols_are_declared_exported_and_bound():
    from pcl_tracking_amd import _lib

    header = open(os.path.join(ROOT, "include", "pft.h")).read()
    L = _lib.load()
    bound = {n: (res, args) for n, res, args in _lib.SYMBOLS}
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert hasattr(L, name), name
        assert name in bound and bound[name][0] is C.c_int, name
    assert re.search(r"\bvoid pft_refine_config_default\(", header) and hasattr(L, "pft_refine_config_default")
    assert "PFT_ABI_VERSION 5" in header, "pft_config and the ABI version stay as they are"


def test_mirrors_driver_and_build_have_the_feature():
    import inspect

    from pcl_tracking_amd import build, tracker

    for m in ("refine", "getRefineTrace"):
        assert callable(getattr(tracker.ParticleFilterTracker, m)), m
    sig = inspect.signature(tracker.ParticleFilterTracker.refine)
    assert {k: v.default for k, v in sig.parameters.items() if k != "self"} == dict(
        start=None, max_iterations=16, pair_distance=None, inlier_distance=0.02, margin=None, trans_eps=1e-4, rot_eps=1e-3,
        min_pairs=3, apply=False)
    assert inspect.signature(tracker.ParticleFilterTracker.reacquire).parameters["refine"].default is False
    hpp = open(os.path.join(ROOT, "pcl_tracking_amd", "include", "pft", "particle_filter_tracker.hpp")).read()
    assert re.search(r"\bint refine\(", hpp) and re.search(r"\bpft_refine_config refineConfig\(", hpp)
    assert "pft_refine.hip" in build.SOURCES and "pft_refine_solve.h" in build.HEADERS
    exe = build.build_example()
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "--refine[=max_iterations[,pair_distance]]" in r.stderr
    r = subprocess.run([exe, "m.bin", "--frames", "f.bin", "--match", "--refine"], capture_output=True, text=True)
    assert r.returncode == 2 and "--refine needs --reacquire" in r.stderr
    for bad in ("--refine=0", "--refine=65", "--refine=8,-1", "--refine=x"):
        r = subprocess.run([exe, "m.bin", "--frames", "f.bin", "--match", "--reacquire", bad], capture_output=True, text=True)
        assert r.returncode == 2 and "max_iterations" in r.stderr, bad


def test_python_arguments_are_checked_without_a_device():
    from pcl_tracking_amd import tracker
    from pcl_tracking_amd._lib import PftError

    with pytest.raises(PftError) as e:
        tracker.ParticleFilterTracker().getRefineTrace()
    assert e.value.status == 7


# ---- the one-lane solve header on the host ----------------------------------------------------------------------------
def _compile(out, extra=()):
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off", *extra, "-I",
                    os.path.join(ROOT, "pcl_tracking_amd", "csrc"), SRC, "-o", out], check=True)
    return out


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    return _compile(str(tmp_path_factory.mktemp("refine") / "refine_solve_tool"))


def rot(axis, angle):
    """Rodrigues, double"""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)


def sums_of(a_pts, b_pts, c):
    """the 17 tree sums of explicit pairs (every pair inside both gates, d2 their squared distance in float)"""
    a32, b32 = np.asarray(a_pts, np.float32), np.asarray(b_pts, np.float32)
    d2 = ((a32 - b32).astype(np.float32) ** 2).sum(1).astype(np.float32)
    t, _, _ = rfm.terms(a32, b32, d2, np.ones(len(a32), bool), c, np.inf, np.inf)
    return np.array([mm.tree_sum(t[:, k]) for k in range(rfm.N_SUMS)], np.float64), len(a32)


def start_matrix(R, t):
    T = np.zeros((3, 4), np.float32)
    T[:, :3], T[:, 3] = R, t
    return T


def solve_cases():
    """(label, sums, n, pivot, start): seeded pairs and the degenerate shapes"""
    rng = np.random.default_rng(5)
    cases = []
    c0 = np.array([0.31, -0.12, 1.05])

    def add(label, a, b, c=c0, start=None):
        s, n = sums_of(a, b, c)
        cases.append((label, s, n, np.asarray(c, np.float64), start_matrix(np.eye(3), c) if start is None else start))

    for n in (3, 4, 17, 300):
        a = rng.normal(0.0, 0.1, (n, 3)) + c0
        R, t = rot(rng.normal(size=3), rng.uniform(0.05, 1.2)), rng.normal(0.0, 0.03, 3)
        b = (a - c0) @ R.T + c0 + t + rng.normal(0.0, 0.002, (n, 3))
        add("random n=%d" % n, a, b, start=start_matrix(rot(rng.normal(size=3), rng.uniform(0.0, 3.1)), c0))
    a = rng.normal(0.0, 0.1, (50, 3)) + c0
    add("a == b", a, a)
    # (dyadic coordinates around a zero pivot, four copies: every sum and S = H - A B^T / n are exact, S is exactly zero)
    add("all-zero S (one point repeated)", np.repeat([[0.25, 0.5, 0.75]], 4, 0), np.repeat([[1.5, -0.25, 0.5]], 4, 0), c=np.zeros(3))
    line = c0 + np.outer(np.linspace(-0.2, 0.2, 20), [0.3, 0.5, -0.8])
    add("collinear", line, (line - c0) @ rot([0, 0, 1], 0.3).T + c0 + [0.01, 0.0, -0.02])
    add("collinear a == b", line, line)
    plane = c0 + rng.normal(0.0, 0.1, (40, 3)) * [1.0, 1.0, 0.0]
    add("coplanar", plane, (plane - c0) @ rot([1, 2, 3], 0.4).T + c0 + [0.0, 0.02, 0.01])
    add("coplanar a == b", plane, plane)
    add("mirrored target (det < 0)", a, (a - c0) * [1.0, 1.0, -1.0] + c0)
    add("half turn", a, (a - c0) @ rot([0, 1, 0], np.pi).T + c0)
    # the Shoemake branches of the start: trace <= 0 with each diagonal entry the largest
    for ax in ([1, 0.1, 0.1], [0.1, 1, 0.1], [0.1, 0.1, 1]):
        b = (a - c0) @ rot([1, 1, 0], 0.2).T + c0
        add("start: half turn about %s" % ax, a, b, start=start_matrix(rot(ax, 3.0), c0))
    return cases


def run_tool(exe, cases, tmp_path):
    rec = np.zeros(len(cases), CASE)
    for k, (_, s, n, c, start) in enumerate(cases):
        rec[k]["sums"], rec[k]["n"], rec[k]["c"], rec[k]["start"] = s, n, c, start.reshape(-1)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    rec.tofile(fin)
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return np.fromfile(fout, OUT)


def model_out(case):
    _, s, n, c, start = case
    Q0, t0 = rfm.quat_from_matrix(start)
    Q, t, dq, st2, sr2, sweeps = rfm.solve(s, n, c, Q0, t0)
    return dict(Q0=Q0, t0=t0, Q=Q, t=t, dq=dq, step2=[st2, sr2], T=rfm.transform(Q, t).reshape(-1), sweeps=sweeps)


def check_tool(got, cases):
    for g, case in zip(got, cases):
        w = model_out(case)
        for f in ("Q0", "t0", "Q", "t", "dq", "step2"):
            assert rfm.bits(np.asarray(g[f], np.float64)).tolist() == rfm.bits(np.asarray(w[f], np.float64)).tolist(), (case[0], f)
        assert g["T"].tobytes() == np.asarray(w["T"], np.float32).tobytes(), case[0]
        assert int(g["sweeps"]) == w["sweeps"], case[0]


def test_solve_header_equals_the_model_bit_for_bit(tool, tmp_path):
    cases = solve_cases()
    got = run_tool(tool, cases, tmp_path)
    check_tool(got, cases)
    by = {c[0]: g for c, g in zip(cases, got)}
    print("sweeps:", {c[0]: int(g["sweeps"]) for c, g in zip(cases, got)})
    assert max(int(g["sweeps"]) for g in got) < rfm.JACOBI_SWEEPS, "every case reaches exact zeros below the cap"
    for label in ("a == b", "collinear a == b", "coplanar a == b", "all-zero S (one point repeated)"):
        assert by[label]["dq"].tolist() == [1.0, 0.0, 0.0, 0.0], label
        assert by[label]["step2"][1] == 0.0, label
    for label in ("a == b", "collinear a == b", "coplanar a == b"):  # the answer is exactly the identity: a zero step
        g = by[label]
        assert g["step2"].tolist() == [0.0, 0.0], label
        assert g["Q"].tobytes() == g["Q0"].tobytes() and g["t"].tobytes() == g["t0"].tobytes(), label
    g = by["mirrored target (det < 0)"]  # a proper rotation, never the reflection
    assert abs(np.linalg.det(np.array(rfm.rotation(g["dq"])).reshape(3, 3)) - 1.0) < 1e-12


def test_solve_header_under_sanitizers(tmp_path):
    """the same program built with the address and undefined-behaviour sanitizers, as a program of its own"""
    san = _compile(str(tmp_path / "refine_solve_tool_san"),
                   ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"))
    cases = solve_cases()
    check_tool(run_tool(san, cases, tmp_path), cases)


# ---- known answers ----------------------------------------------------------------------------------------------------
def eigh_rotation(s, n):
    """the rotation of the same Horn matrix by numpy.linalg.eigh"""
    _, _, N = rfm.horn_matrix(s, n)
    w, v = np.linalg.eigh(np.array(N, np.float64))
    q = v[:, np.argmax(w)]
    return np.array(rfm.rotation(list(q / np.linalg.norm(q)))).reshape(3, 3)


def test_exact_pairs_under_a_known_motion_are_recovered():
    """float32 points a, b = R a + t evaluated in double from the same a and handed over unrounded (the sums take doubles), so
    the pairs are exact to double rounding.  Tolerance: numpy.linalg.eigh of the same 4x4 matrix recovers R to 2.8e-17 ..
    2.2e-14 (largest entry of R_eigh - R_true over these ten motions, measured here; the worst is a three-point case) and
    the translation that follows from it is no worse; a Jacobi solve in the same precision has the same kind of error, a
    few hundred ulps of 1 at the most.  The bound 1e-12 is fifty times eigh's worst and six orders of magnitude below the
    1e-6 a wrong pair order or sign would show"""
    rng = np.random.default_rng(9)
    worst_eigh = 0.0
    for k in range(10):
        n = (3, 5, 40, 300)[k % 4]
        c = rng.normal(0.0, 0.5, 3)
        a = (rng.normal(0.0, 0.1, (n, 3)) + c).astype(np.float32).astype(np.float64)
        R, t = rot(rng.normal(size=3), rng.uniform(0.0, 3.0)), rng.normal(0.0, 0.05, 3)
        b = (a - c) @ R.T + c + t
        tm = np.zeros((n, rfm.N_SUMS))
        A, B = a - c, b - c
        tm[:, 0:3], tm[:, 3:6] = A, B
        for r in range(3):
            for q in range(3):
                tm[:, 6 + 3 * r + q] = A[:, r] * B[:, q]
        s = np.array([mm.tree_sum(tm[:, j]) for j in range(rfm.N_SUMS)])
        Q, tn, dq, st2, sr2, _ = rfm.solve(s, n, c, [1.0, 0.0, 0.0, 0.0], list(c))
        Rg = np.array(rfm.rotation(dq)).reshape(3, 3)
        e_rot, e_eigh = np.abs(Rg - R).max(), np.abs(eigh_rotation(s, n) - R).max()
        e_t = np.abs(np.array(tn) - (c + t)).max()
        worst_eigh = max(worst_eigh, e_eigh)
        print("motion %d n %d: rotation error %.3g (eigh %.3g) translation error %.3g" % (k, n, e_rot, e_eigh, e_t))
        assert e_rot < 1e-12 and e_t < 1e-12
        assert np.abs(np.array(rfm.rotation(Q)).reshape(3, 3) - R).max() < 1e-12, "from the identity the new state is the motion"
    print("worst eigh error %.3g" % worst_eigh)


def test_quat_from_matrix_round_trip():
    """R(quat_from_matrix(T)) == T to float rounding on every Shoemake branch"""
    for ax, ang in (([1, 2, 3], 0.4), ([1, 0.1, 0.1], 3.0), ([0.1, 1, 0.1], 3.0), ([0.1, 0.1, 1], 3.0), ([0, 0, 1], np.pi)):
        T = start_matrix(rot(ax, ang), [0.1, 0.2, 0.3])
        Q, t = rfm.quat_from_matrix(T)
        assert abs(sum(v * v for v in Q) - 1.0) < 4e-16
        assert np.abs(np.array(rfm.rotation(Q)).reshape(3, 3) - T[:, :3].astype(np.float64)).max() < 4e-7
        assert t == [float(v) for v in T[:, 3]]


# ---- the scenario on the CPU ------------------------------------------------------------------------------------------
def box_of(orc, ref, start, margin):
    m = np.eye(4, dtype=np.float32)
    m[:3] = start
    moved = orc.transform_cloud(ref, m)
    xyz = np.stack([moved["x"], moved["y"], moved["z"]], 1).astype(np.float64)
    lo, hi = xyz.min(0) - margin, xyz.max(0) + margin
    return np.array([lo[0], hi[0], lo[1], hi[1], lo[2], hi[2]], np.float32)


def test_the_scenario_holds_on_the_cpu(orc):
    """the defaults with pair_distance = 0.1 on the scenario of test_reacquire_host: from the two lattice neighbours of the
    truth (yaw -22.5 and +22.5 degrees) the refinement gains inliers and rotation accuracy; from the truth it loses none"""
    ref, cloud, centres, cand = _scenario(orc)
    gtp = scene.model_gt_pose()
    R_true = scene.pose_matrix(*gtp)
    ocfg = orc.default_config(particle_num=tgm.P, threads=0, emulate_pcl_alloc=0)
    o = orc.Tracker(ocfg)
    o.set_reference(ref)
    o.set_input(cloud)
    cfg = rfm.config(pair_distance=0.1)
    for label, pose in (("yaw -22.5", cand[8 + 3]), ("yaw +22.5", cand[8 + 4]), ("truth", None)):
        p = gtp if pose is None else tuple(float(pose[k]) for k in tgm.KEYS)
        start = np.asarray(orc.get_transformation(*p), np.float32).reshape(4, 4)[:3]
        trace, res = rfm.run(orc, o, ref, cloud, start, cfg, box_of(orc, ref, start, 0.1))
        before, after = rfm.rotation_error_deg(start, R_true), rfm.rotation_error_deg(res["transform"], R_true)
        dt = np.linalg.norm(res["transform"][:, 3].astype(np.float64) - R_true[:3, 3])
        print("%s: status %d iterations %d inliers %d -> %d of %d, pairs %d -> %d, rotation error %.2f -> %.2f deg, "
              "translation error %.4f m, improved %d" % (label, res["status"], res["iterations"], res["n_inliers_before"],
                                                          res["n_inliers_after"], len(ref), res["n_pairs_before"],
                                                          res["n_pairs_after"], before, after, dt, res["improved"]))
        assert len(trace) == res["iterations"] + 1
        if pose is None:
            assert res["n_inliers_after"] >= res["n_inliers_before"]
        else:
            assert abs(before - 22.5) < 0.01
            assert res["n_inliers_after"] > res["n_inliers_before"] and res["improved"]
            assert after < before
