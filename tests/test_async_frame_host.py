"""Host-side checks of the asynchronous frame path (no GPU): the new entry points are declared, exported and bound, and
a null handle is refused before any device is touched."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pft_filter_apply_async", "pft_filter_apply_device_async", "pft_set_input_from_filter")


def _decl(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_entry_points_are_declared_exported_and_bound():
    from pcl_tracking_amd import _lib

    L = _lib.load()
    filt, trk = _decl("pft_filters.h"), _decl("pft.h")
    assert re.search(r"int\s+pft_filter_apply_async\s*\(\s*pft_filter\s*\*", filt)
    assert re.search(r"int\s+pft_filter_apply_device_async\s*\(\s*pft_filter\s*\*", filt)
    assert re.search(r"int\s+pft_set_input_from_filter\s*\(\s*pft_tracker\s*\*\s*\w+,\s*(struct\s+)?pft_filter\s*\*\s*\w+,"
                     r"\s*size_t\s+max_points\s*\)", trk)
    bound = {n: (r, a) for n, r, a in _lib.SYMBOLS}
    for name in NEW:
        assert hasattr(L, name), name
        assert name in bound and bound[name][0] is C.c_int and len(bound[name][1]) == 3


def test_null_handles_are_refused_without_a_device():
    from pcl_tracking_amd import _lib

    L = _lib.load()
    buf = (C.c_char * 64)()
    assert L.pft_filter_apply_async(None, buf, 2) == 1  # PFT_ERR_INVALID_ARG
    assert L.pft_filter_apply_device_async(None, buf, 2) == 1
    assert L.pft_filter_apply_async(None, None, 0) == 1
    assert L.pft_set_input_from_filter(None, None, 0) == 1
    assert L.pft_set_input_from_filter(None, C.c_void_p(16), 7) == 1


def test_python_and_cpp_mirrors_have_the_members():
    from pcl_tracking_amd import filters, tracker

    assert callable(filters.InputFilter.filterAsync)
    assert callable(tracker.ParticleFilterTracker.setInputCloudFromFilter)
    inc = os.path.join(ROOT, "pcl_tracking_amd", "include", "pft")
    assert "filterAsync" in open(os.path.join(inc, "filters.hpp")).read()
    assert "setInputCloudFromFilter" in open(os.path.join(inc, "particle_filter_tracker.hpp")).read()
    drv = open(os.path.join(ROOT, "pcl_tracking_amd", "examples", "auto_tracking_amd.cpp")).read()
    assert '"--async"' in drv and "setInputCloudFromFilter" in drv
