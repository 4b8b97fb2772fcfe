"""The one-lane tail of the plane refit on the host (no GPU): csrc/pft_segment_solve.h, the very text the kernels compile,
run by tests/cpp/segment_solve_tool.cpp on the nine means of every refit case, on explicit matrices at the edges of the
scale rule and on seeded random covariances -- against the NumPy model (tests/segment_model.py) bit for bit once the
tool's own atan2f / cosf / sinf values are substituted into it, also under the address and undefined-behaviour
sanitizers; the three trig values within the OpenCL full-profile bounds of float64; and the model's normals against
numpy.linalg.eigh.  Also the ABI of pft_debug_segment_refit.  The device is compared in tests/test_gpu_segment_refit.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import refit_cases as RC
import segment_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "segment_solve_tool.cpp")
F = np.float32
CASE = np.dtype([("accu", "f4", 9), ("m", "u4")])
REC_OFFSETS = [("m", 0), ("branches", 4), ("accu", 8), ("cov", 44), ("scale", 68), ("trig_arg", 72), ("trig", 84),
               ("roots", 96), ("len", 108), ("coef", 120)]


# ---- the ABI ----------------------------------------------------------------------------------------------------------
def test_refit_debug_is_declared_exported_bound_and_laid_out(tmp_path):
    from pcl_tracking_amd import build

    build.build()
    from pcl_tracking_amd import _lib, segment

    header = open(os.path.join(ROOT, "include", "pft_segment.h")).read()
    L = _lib.load()
    bound = {n: (res, args) for n, res, args in _lib.SYMBOLS}
    assert re.search(r"\bint pft_debug_segment_refit\(", header) and hasattr(L, "pft_debug_segment_refit")
    assert bound["pft_debug_segment_refit"][0] is C.c_int
    assert callable(segment.ModelSegmenter.refitDebug)
    assert "pft_segment_solve.h" in build.HEADERS
    assert "PFT_ABI_VERSION 5" in open(os.path.join(ROOT, "include", "pft.h")).read()
    assert C.sizeof(_lib.SegmentRefitDebug) == 136 == RC.REC.itemsize and C.sizeof(_lib.SegmentPlane) == 72
    for f, off in REC_OFFSETS:
        assert getattr(_lib.SegmentRefitDebug, f).offset == off == RC.REC.fields[f][1], f
    body = "  printf(\"size %zu\\n\", sizeof(pft_segment_refit_debug));\n" + "".join(
        "  printf(\"%s %%zu\\n\", offsetof(pft_segment_refit_debug, %s));\n" % (f, f) for f, _ in REC_OFFSETS)
    body += "".join("  printf(\"bit%d %%u\\n\", (unsigned)PFT_REFIT_%s);\n" % (k, n.upper())
                    for k, n in enumerate(M.BRANCH_NAMES))
    src = tmp_path / "layout.c"
    src.write_text("#include <stddef.h>\n#include <stdio.h>\n#include \"pft_segment.h\"\nint main(void) {\n" + body +
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["size"]) == 136
    for f, off in REC_OFFSETS:
        assert int(got[f]) == off, f
    for k in range(13):  # the model's bit numbering is the header's
        assert int(got["bit%d" % k]) == 1 << k


def test_refit_debug_refuses_before_an_apply():
    from pcl_tracking_amd import _lib

    assert _lib.load().pft_debug_segment_refit(None, 0, None) == 1  # PFT_ERR_INVALID_ARG


# ---- the header on the host -------------------------------------------------------------------------------------------
def _compile(out, extra=()):
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off", *extra, "-I",
                    os.path.join(ROOT, "pcl_tracking_amd", "csrc"), SRC, "-o", out], check=True)
    return out


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    return _compile(str(tmp_path_factory.mktemp("segment_solve") / "segment_solve_tool"))


def _sym(xx, xy, xz, yy, yz, zz, mean=(0, 0, 0)):
    """the nine means that give this covariance about this mean (exactly so when the mean is 0)"""
    mx, my, mz = (F(v) for v in mean)
    c = [F(v) for v in (xx, xy, xz, yy, yz, zz)]
    return [F(c[0] + F(mx * mx)), F(c[1] + F(mx * my)), F(c[2] + F(mx * mz)), F(c[3] + F(my * my)), F(c[4] + F(my * mz)),
            F(c[5] + F(mz * mz)), mx, my, mz]


@pytest.fixture(scope="module")
def inputs():
    """[(label, accu[9], m)]: the means of every case, explicit matrices at and around the FLT_MIN edge of the scale and
    at the axes, 300 seeded random covariances"""
    out = []
    for m in sorted(set(RC.PCL_M + RC.TREE_M)):
        if m < 4:
            continue  # (no refit below 4)
        for order, lst in (("pcl", RC.PCL_M), ("tree", RC.TREE_M)):
            if m in lst:
                r = RC.model("sum", m, order)
                out.append(("sum m = %d %s" % (m, order), M.moment_means(r["xyz"][r["rounds"][0]["ransac_inliers"]], order), m))
    for order in RC.ORDERS:
        r = RC.model("rounds", None, order)
        for k, rd in enumerate(r["rounds"]):
            p = r["xyz"][rd["ransac_inliers"]]
            out.append(("rounds scene, round %d %s" % (k, order), M.moment_means(p, order), len(p)))
        for name in RC.SOLVE_CASES:
            r = RC.model("solve", name, order)
            p = r["xyz"][r["rounds"][0]["ransac_inliers"]]
            out.append(("%s %s" % (name, order), M.moment_means(p, order), len(p)))
    tiny = float(np.finfo(F).tiny)
    for label, a in (("explicit: the zero matrix (scale <= FLT_MIN, every length 0)", _sym(0, 0, 0, 0, 0, 0)),
                     ("explicit: largest entry FLT_MIN (scale <= FLT_MIN)", _sym(tiny, 0, 0, tiny / 2, 0, tiny / 4)),
                     ("explicit: subnormal entries (scale <= FLT_MIN)", _sym(3e-40, 1e-41, 0, 2e-40, 0, 1e-42)),
                     ("explicit: just above FLT_MIN (scaled)", _sym(tiny * 2, 0, 0, tiny, 0, tiny / 2)),
                     ("explicit: identity (triple root)", _sym(1, 0, 0, 1, 0, 1)),
                     ("explicit: diag(2, 1, 0) (c0 == 0)", _sym(2, 0, 0, 1, 0, 0)),
                     ("explicit: diag(0, 1, 2) (pick 2)", _sym(0, 0, 0, 1, 0, 2)),
                     ("explicit: diag(1, 0, 2) (pick 1)", _sym(1, 0, 0, 0, 0, 2)),
                     ("explicit: rank one", _sym(1, 2, 3, 4, 6, 9)),
                     ("explicit: huge entries", _sym(3e37, 1e37, 0, 2e37, 0, 1e37))):
        out.append((label, a, 8))
    rng = np.random.default_rng(20)
    for k in range(300):
        A = rng.normal(0, 1, (3, 3)) * [1, 10.0 ** rng.uniform(-3, 0), 10.0 ** rng.uniform(-4, 0)]
        c = (A @ A.T) * 10.0 ** rng.uniform(-6, 1)
        mean = rng.uniform(-2, 2, 3) if k % 2 else (0, 0, 0)
        out.append(("random %d" % k, _sym(c[0, 0], c[0, 1], c[0, 2], c[1, 1], c[1, 2], c[2, 2], mean), 100 + k))
    return out


def run_tool(exe, inputs, tmp_path):
    c = np.zeros(len(inputs), CASE)
    for rec, (_, accu, m) in zip(c, inputs):
        rec["accu"], rec["m"] = accu, m
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    c.tofile(fin)
    subprocess.run([exe, str(fin), str(fout)], check=True)
    got = np.fromfile(fout, RC.REC)
    assert len(got) == len(inputs)
    return got


def check_tool(got, inputs):
    worst, union = [0.0, 0.0, 0.0], 0
    for g, (label, accu, m) in zip(got, inputs):
        err = RC.check_record(g, accu, m, label)
        union |= int(g["branches"])
        if err is not None:
            worst = [max(a, b) for a, b in zip(worst, err)]
    return worst, union


def test_header_on_the_host_equals_the_model(tool, inputs, tmp_path):
    """with the tool's own three trig values substituted, every field equals the model's bit for bit; each trig value is
    within its cap of float64 on the same float arguments"""
    got = run_tool(tool, inputs, tmp_path)
    worst, union = check_tool(got, inputs)
    print("host libm, largest error in ulps over %d solves: atan2f %.3f, cosf %.3f, sinf %.3f (caps 6 / 4 / 4)"
          % ((len(inputs),) + tuple(worst)))
    print("branches taken:", M.branch_names(union))
    assert union == (1 << 13) - 1
    by = {label: g for g, (label, _, _) in zip(got, inputs)}
    for label in by:
        if label.startswith("explicit:") and "(scale <= FLT_MIN" in label:
            assert by[label]["branches"] & M.SCALE_TINY and by[label]["scale"] == 1.0, label
    assert not by["explicit: just above FLT_MIN (scaled)"]["branches"] & M.SCALE_TINY
    assert np.isnan(by["cube pcl"]["coef"]).all() and np.isnan(by["explicit: the zero matrix (scale <= FLT_MIN, every length 0)"]["coef"]).all()
    # without the substitution the host's libm and NumPy's may differ, but by no more than the slack measured in
    # tests/test_refit_cases_host.py: a few ulps of a coefficient on the well-conditioned cases
    g = by["normal z pcl"]
    own = M.solve_trace(g["accu"], int(g["m"]))
    assert np.abs(own["coef"] - g["coef"]).max() <= 1e-6


def test_segment_solve_header_under_sanitizers(tool, inputs, tmp_path):
    """the same program built with the address and undefined-behaviour sanitizers, as a program of its own: the same
    bytes"""
    san = _compile(str(tmp_path / "segment_solve_tool_san"),
                   ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"))
    a = run_tool(tool, inputs, tmp_path)
    b = run_tool(san, inputs, tmp_path)
    assert a.tobytes() == b.tobytes()
    check_tool(b, inputs)


# ---- known answers, model only ----------------------------------------------------------------------------------------
def _cov3(c):
    c = np.asarray(c, np.float64)
    return np.array([[c[0], c[1], c[2]], [c[1], c[3], c[4]], [c[2], c[4], c[5]]])


def test_model_normals_against_eigh():
    """the model's normal against the eigenvector of the smallest eigenvalue of numpy.linalg.eigh on the model's own float
    covariance taken to double, for every solve case and every round of the rounds scene.  Asserted (1e-2 rad: a wrong
    root or a swapped row gives at least 0.1) where the result is finite and the relative gap (l1 - l0) / l2 is at least
    0.1; the others are printed.  Measured on this case list: see DESIGN.md section 3.7."""
    rows = []
    for order in RC.ORDERS:
        r = RC.model("rounds", None, order)
        rows += [("rounds scene, round %d" % k, order, RC.model_trace(r, k, order)) for k in range(3)]
        rows += [(name, order, RC.model_trace(RC.model("solve", name, order), 0, order)) for name in RC.SOLVE_CASES]
    worst, n_asserted = 0.0, 0
    for name, order, t in rows:
        w, v = np.linalg.eigh(_cov3(t["cov"]))
        with np.errstate(invalid="ignore"):
            gap = (w[1] - w[0]) / w[2]  # (nan for the zero matrix of the far speck)
        n = t["coef"][:3].astype(np.float64)
        finite = bool(np.isfinite(n).all())
        ang = float(np.arccos(min(1.0, abs(float(n @ v[:, 0])) / np.linalg.norm(n)))) if finite else float("nan")
        asserted = finite and gap >= 0.1
        print("%-62s %-4s gap %.3g angle %.3g rad%s" % (name, order, gap, ang, "" if asserted else "  (not asserted)"))
        if asserted:
            n_asserted += 1
            worst = max(worst, ang)
            assert ang <= 1e-2, (name, order, ang)
    print("worst asserted angle: %.3g rad over %d cases" % (worst, n_asserted))
    assert n_asserted >= 20
