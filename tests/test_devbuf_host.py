"""CPU checks of the owning device buffer (csrc/pft_devbuf.h) and of how the handle files use it: the header compiled into a
stand-alone program (tests/cpp/devbuf_tool.cpp) whose pft_dev_alloc / pft_dev_free sit on malloc, with a counter that makes
the k-th allocation fail -- reserve below the capacity is a no-op, growth frees exactly once, a failed reserve or alloc
leaves null with capacity 0 and a later reserve succeeds, move and swap hand ownership over without a double free or a
leak, and the build-in-locals-then-swap growth keeps the old buffers when any of its allocations fails.  The same program
runs a second time under the address and undefined-behaviour sanitizers.  The device side of the growth paths is
tests/test_gpu_handle_growth.py."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pcl_tracking_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "devbuf_tool.cpp")
HOST_FILES = ("pft_api.hip", "pft_frame.hip", "pft_api_debug.hip", "pft_api_features.hip")


def _compile(out, extra=()):
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *extra, "-I", CSRC, SRC, "-o", out], check=True)
    return out


def _run(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert "FAILED" not in r.stdout and "live 0 bad_frees 0" in r.stdout
    m = re.search(r"^ok (\d+)$", r.stdout, re.M)
    assert m and int(m.group(1)) > 60, r.stdout[-500:]


def test_devbuf_header_on_the_host(tmp_path):
    _run(_compile(str(tmp_path / "devbuf_tool")))


def test_devbuf_header_under_sanitizers(tmp_path):
    """the same program with the address (and leak) and undefined-behaviour sanitizers, as a program of its own"""
    _run(_compile(str(tmp_path / "devbuf_tool_san"),
                  ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan")))


def test_devbuf_header_needs_no_hip():
    text = open(os.path.join(CSRC, "pft_devbuf.h")).read()
    assert not re.search(r"#include\s*[<\"]hip", text)


def test_handle_sources_are_part_of_the_build():
    from pcl_tracking_amd import build

    for s in HOST_FILES:
        assert s in build.SOURCES and os.path.exists(os.path.join(CSRC, s)), s
    assert "pft_tracker.h" in build.HEADERS and "pft_devbuf.h" in build.HEADERS


def test_one_allocator_and_one_error_macro():
    """hipMalloc / hipFree are called in one place, the error macro is defined in one place, and the tracker's destroy
    names no buffer"""
    srcs = {s: open(os.path.join(CSRC, s)).read() for s in os.listdir(CSRC) if s.endswith((".hip", ".h"))}
    users = sorted(s for s, t in srcs.items() if re.search(r"\bhip(Malloc|Free)\(", t))
    assert users == ["pft_api.hip"], users
    assert len(re.findall(r"\bhipMalloc\(", srcs["pft_api.hip"])) == 1 and len(re.findall(r"\bhipFree\(", srcs["pft_api.hip"])) == 1
    macros = sorted(s for s, t in srcs.items() if re.search(r"#define \w*CHK\(", t))
    assert macros == ["pft_devbuf.h"], macros
    m = re.search(r'extern "C" void pft_destroy\(pft_tracker\* t\) \{(.*?)\n\}', srcs["pft_api.hip"], re.S)
    assert m and "d_" not in m.group(1) and "sv_" not in m.group(1)


@pytest.mark.parametrize("name", HOST_FILES + ("pft_tracker.h", "pft_devbuf.h"))
def test_handle_files_stay_readable(name):
    assert len(open(os.path.join(CSRC, name)).read().splitlines()) <= 1100, name
