"""The alias-table search of the resample kernels, run on the CPU (no GPU needed).

pcl_tracking_amd/csrc/pft_alias.h -- alias_q, alias_a_small and the two-level searches through a coarse level of the
running sums -- is the text the kernels compile; tests/cpp/alias_search_tool.cpp compiles it for the host, builds the
prefix-sum form sequentially from its specification and writes the (a, q) table once without a coarse level and once per
stride (the kernels' own, and 1, 2, 3, 7, n forced).

(i)   every stride gives the bytes of the plain search;
(ii)  for dyadic inputs (n a power of two, every w * n a multiple of 2^-10: Walker's updates and the running sums are
      exact in double) the table equals the oracle's sequential genAliasTable byte for byte -- the prefix-form
      derivation itself, no tolerance;
(iii) the tool built with the address and undefined-behaviour sanitizers, as a program of its own, runs the ragged-block
      cases clean.
"""
import os
import subprocess

import numpy as np
import pytest

import alias_cases as AC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "alias_search_tool.cpp")
VARIANTS = ("plain", "kernel", "s=1", "s=2", "s=3", "s=7", "s=n")


def _compile(out, extra=()):
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *extra, "-I", os.path.join(ROOT, "pcl_tracking_amd", "csrc"),
                    SRC, "-o", out], check=True)
    return out


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    return _compile(str(tmp_path_factory.mktemp("alias") / "alias_search_tool"))


def run_tool(tool, cases, tmp_path):
    """cases: list of float32 weight arrays -> per case an array [variant] of (a, q)"""
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        for w in cases:
            w = np.ascontiguousarray(w, np.float32)
            f.write(np.uint32(len(w)).tobytes())
            f.write(w.tobytes())
    r = subprocess.run([tool, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    blob = np.fromfile(fout, np.uint8)
    res, o = [], 0
    for w in cases:
        n, nv = (int(x) for x in blob[o:o + 8].view(np.uint32))
        assert n == len(w) and nv == len(VARIANTS)
        o += 8
        tabs = []
        for _ in range(nv):
            a = blob[o:o + 4 * n].view(np.int32)
            o += 4 * n
            q = blob[o:o + 8 * n].view(np.float64)
            o += 8 * n
            tabs.append((a, q))
        res.append(tabs)
    assert o == len(blob)
    return res


def shapes_for(n, rng):
    out = AC.basic(n, rng)
    out.append(("random", rng.random(n).astype(np.float32) / np.float32(n) * np.float32(2)))
    out.append(("zeros", np.zeros(n, np.float32)))
    if n > 2:
        m = int(rng.integers(1, n))
        out.append(("m=%d" % m, AC.with_smalls(n, m, rng)))
    return out


def check_strides_agree(tool, labelled, tmp_path):
    res = run_tool(tool, [w for _, w in labelled], tmp_path)
    for (label, w), tabs in zip(labelled, res):
        a0, q0 = tabs[0]
        for name, (a, q) in zip(VARIANTS[1:], tabs[1:]):
            assert a.tobytes() == a0.tobytes(), (label, len(w), name, np.flatnonzero(a != a0)[:8])
            assert q.tobytes() == q0.tobytes(), (label, len(w), name, np.flatnonzero(q != q0)[:8])


def test_every_stride_gives_the_plain_search_small_sizes(tool, tmp_path):
    rng = np.random.default_rng(1)
    labelled = []
    for n in range(1, 71):
        labelled += [("%s n=%d" % (k, n), w) for k, w in shapes_for(n, rng)]
    check_strides_agree(tool, labelled, tmp_path)


def test_every_stride_gives_the_plain_search_seeded_sizes(tool, tmp_path):
    """300 sizes up to 70 000, log-uniform (so most are small and the whole run stays short), one shape each in turn, and
    the sizes around which the kernels' stride steps for a uniformly split population"""
    rng = np.random.default_rng(2)
    sizes = [int(x) for x in np.exp(rng.uniform(np.log(71), np.log(70000), 300))]
    labelled = []
    for i, n in enumerate(sizes):
        sh = shapes_for(n, rng)
        k, w = sh[i % len(sh)]
        labelled.append(("%s n=%d" % (k, n), w))
    for n in (511, 513, 1024, 4097, 8192, 16385, 65536, 70000):
        labelled += [("%s n=%d" % (k, n), w) for k, w in AC.basic(n, rng)]
    for n in (1024, 8192):
        labelled += [("%s n=%d" % (k, n), w) for k, w in AC.constructed(n, rng)]
    check_strides_agree(tool, labelled, tmp_path)


def dyadic_cases(rng):
    """[(label, w)]: n a power of two, every w * n a multiple of 2^-10 (w itself then is exact in float)"""
    out = []
    for n in (1, 2, 4, 64, 256, 512, 1024, 8192):
        fn = np.float32(n)
        out.append(("uniform n=%d" % n, AC.uniform(n)))
        out.append(("single n=%d" % n, AC.single_mass(n)))
        out.append(("ties n=%d" % n, AC.ties(n)))
        # skewed: integers k / 1024 with many zeros and a few heavy entries
        k = (rng.random(n) ** 6 * 4096).astype(np.int64)
        k[rng.random(n) < 0.15] = 0
        out.append(("skewed n=%d" % n, (k.astype(np.float32) / np.float32(1024)) / fn))
        # exact q == 1 mixed with smalls and larges
        q = rng.choice(np.array([0.0, 0.25, 0.5, 0.75, 1.0, 1.0, 1.0, 1.25, 1.5, 3.0], np.float32), n)
        out.append(("q==1 mixture n=%d" % n, q / fn))
        # constructed counts of smalls / larges: smalls q = 0.5, larges q = 1 + j / 1024
        for m in AC.COUNTS:
            for mm in (m, n - m):
                if 0 < mm < n:
                    q = np.float32(1) + rng.integers(1, 4096, n).astype(np.float32) / np.float32(1024)
                    q[rng.permutation(n)[:mm]] = 0.5
                    out.append(("m=%d n=%d" % (mm, n), q / fn))
    for label, w in out:
        q = w.astype(np.float32) * np.float32(len(w))
        assert w.dtype == np.float32 and np.array_equal(q * 1024, np.rint(q * 1024)), label
    return out


def test_dyadic_inputs_equal_the_sequential_walker_table(tool, orc, tmp_path):
    labelled = dyadic_cases(np.random.default_rng(3))
    res = run_tool(tool, [w for _, w in labelled], tmp_path)
    for (label, w), tabs in zip(labelled, res):
        a_w, q_w = orc.gen_alias_table(w)
        for name, (a, q) in zip(VARIANTS, tabs):
            assert a.tobytes() == a_w.tobytes(), (label, name, np.flatnonzero(a != a_w)[:8])
            assert q.tobytes() == q_w.tobytes(), (label, name, np.flatnonzero(q != q_w)[:8])


def test_ragged_blocks_run_clean_under_the_host_sanitizers(tmp_path):
    """host code in an executable of its own; the sanitizer runtimes are linked statically into it"""
    san = _compile(str(tmp_path / "alias_search_tool_san"),
                   ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"))
    rng = np.random.default_rng(4)
    labelled = []
    for n in (1024, 8192):
        for c in (255, 256, 257, 513):
            labelled.append(("m=%d n=%d" % (c, n), AC.with_smalls(n, c, rng)))
            labelled.append(("nh=%d n=%d" % (c, n), AC.with_smalls(n, n - c, rng)))
    labelled += [("%s n=%d" % (k, n), w) for n in (1, 2, 257, 513) for k, w in AC.basic(n, rng)]
    check_strides_agree(san, labelled, tmp_path)
