"""CPU checks of the summation-order option (pft_config::sum_order): ABI constant, default, the ctypes layout of the grown
struct against the C compiler's, and the C++ mirror's setter."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pft.h")


@pytest.fixture(scope="module")
def lib():
    from pcl_tracking_amd import build

    build.build()
    from pcl_tracking_amd import _lib

    return _lib


def _header_define(name):
    m = re.search(r"^#define\s+%s\s+(\d+)\s*$" % name, open(HEADER).read(), re.M)
    assert m, name
    return int(m.group(1))


def test_abi_version_and_sum_order_constants_agree(lib):
    assert _header_define("PFT_ABI_VERSION") == lib.PFT_ABI_VERSION == 5
    assert _header_define("PFT_SUM_TREE") == lib.PFT_SUM_TREE == 0
    assert _header_define("PFT_SUM_PCL") == lib.PFT_SUM_PCL == 1
    from pcl_tracking_amd import tracker

    assert tracker.SUM_ORDERS == {"tree": 0, "pcl": 1}


def test_default_config_keeps_the_tree_order(lib):
    L = lib.load()
    c = lib.Config()
    c.sum_order = 7
    L.pft_config_default(C.byref(c))
    assert c.sum_order == 0 and c.abi_version == 5


def test_python_option_sets_the_config_field(lib):
    from pcl_tracking_amd import tracker

    assert tracker.make_reference_tracker(particle_num=400)._cfg.sum_order == 0
    assert tracker.make_reference_tracker(particle_num=400, sum_order="pcl")._cfg.sum_order == 1
    assert tracker.make_reference_tracker(particle_num=400, kld=True, sum_order="pcl")._cfg.sum_order == 1
    with pytest.raises(lib.PftError):
        tracker.make_reference_tracker(particle_num=400, sum_order="sequential")


def test_ctypes_config_layout_matches_the_c_compiler(lib, tmp_path):
    fields = [f for f, _ in lib.Config._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pft.h"\nint main(void) {\n'
                   '  printf("sizeof %zu\\n", sizeof(pft_config));\n'
                   + "".join('  printf("%s %%zu\\n", offsetof(pft_config, %s));\n' % (f, f) for f in fields)
                   + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True,
                                                        check=True).stdout.splitlines())
    assert int(out["sizeof"]) == C.sizeof(lib.Config)
    for f in fields:
        assert int(out[f]) == getattr(lib.Config, f).offset, f
    assert fields[-1] == "sum_order"


def test_cpp_mirror_set_sum_order_compiles(tmp_path):
    src = tmp_path / "mirror.cpp"
    src.write_text('#include "pft/particle_filter_tracker.hpp"\n'
                   "using namespace pft;\nusing namespace pft::tracking;\n"
                   "int main() {\n"
                   "  ParticleFilterOMPTracker<PointXYZRGBA, ParticleXYZRPY> t(16);\n"
                   "  t.setSumOrder(PFT_SUM_PCL);\n"
                   "  KLDAdaptiveParticleFilterOMPTracker<PointXYZRGBA, ParticleXYZRPY> k(16);\n"
                   "  k.setSumOrder(PFT_SUM_TREE);\n"
                   "  return 0;\n}\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), "-I",
                        os.path.join(ROOT, "pcl_tracking_amd", "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
