"""GPU: the input filters (csrc/pft_filters.hip) on the edge cases of tests/filter_cases.py, against the CPU oracle BIT
FOR BIT (output bytes, counts(), passIndices()): long voxels across the tiles of VoxelGrid's emit and a shuffled input
(stable radix sort), points on cell faces, cell indices past 2^24, keys with the fourth radix byte set, both sides of
the INT32_MAX cell-product limit, huge and infinite coordinates, PassThrough limits hit exactly, every history-table
size from 1 to 2048, PassThrough fused with either grid, one handle reused over clouds of very different sizes, device
input.  No tolerance anywhere; the one exception is huge_and_inf without a PassThrough, whose centroids are NaN in
places: NaN positions are compared, NaN payload bits are not.  tests/test_filter_cases_host.py proves on the CPU that
every case reaches the path it is named for and that an independent model agrees with the oracle on it."""
import numpy as np
import pytest

import filter_cases as fc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def F():
    from pcl_tracking_amd import filters

    return filters


def same_cloud(got, want):
    assert len(got) == len(want)
    assert got.tobytes() == want.tobytes()


def make_filter(F, mode, leaf=0.01, hist=512, pass_=None):
    """the PCL-named class where one fits, the fused InputFilter for PassThrough + grid"""
    lf = [float(v) for v in ([leaf] * 3 if np.isscalar(leaf) else leaf)]
    if mode == "pass":
        f = F.PassThrough()
        f.setFilterFieldName(pass_[0])
        f.setFilterLimits(pass_[1], pass_[2])
        f.setFilterLimitsNegative(pass_[3])
        f.setKeepOrganized(False)
        return f
    if pass_ is None:
        f = F.ApproximateVoxelGrid() if mode == "approx" else F.VoxelGrid()
    else:
        f = F.InputFilter()
        f.setPassThrough(*pass_)
        f.setVoxelMode(F.VOXEL_APPROX if mode == "approx" else F.VOXEL_EXACT)
    f.setLeafSize(*lf)
    if mode == "approx":
        f.setHistorySize(hist)
    return f


def check_last_apply(f, got, e):
    """output, counts and kept indices of the apply that produced `got` against the oracle's chain"""
    assert f.counts() == (e.n_pass, len(e.out))
    same_cloud(got, e.out)
    idx = np.arange(e.n_pass, dtype=np.int32) if e.pass_idx is None else e.pass_idx
    np.testing.assert_array_equal(f.passIndices(), idx)


@pytest.mark.parametrize("c", fc.grid_cases() + fc.pass_cases(), ids=lambda c: c.name)
def test_case_bit_for_bit(F, orc, c):
    f = make_filter(F, c.mode, c.leaf, c.hist, c.pass_)
    f.setInputCloud(c.cloud)
    check_last_apply(f, f.filter(), fc.expected(orc, c))


def test_huge_and_infinite_coordinates_without_pass_through(F, orc):
    """cells are INT_MIN, sums inf or NaN: counts, NaN positions, the bits of every other value, colours"""
    c = fc.huge_and_inf("approx")
    f = make_filter(F, "approx")
    f.setInputCloud(c.cloud)
    got, want = f.filter(), orc.approx_voxel_grid(c.cloud, 0.01, 512)
    assert f.counts() == (len(c.cloud), len(want))
    for k in ("x", "y", "z"):
        nan = np.isnan(want[k])
        np.testing.assert_array_equal(np.isnan(got[k]), nan)
        np.testing.assert_array_equal(got[k][~nan].view(np.uint32), want[k][~nan].view(np.uint32))
    for k in ("w", "rgba", "pad"):
        np.testing.assert_array_equal(got[k], want[k])


def test_voxel_grid_leaf_too_small_behind_pass_through_hands_on_what_passed(F, orc):
    c = fc.huge_and_inf("exact", behind_pass=True, big=(3e6, -4e6))
    idx = orc.pass_through(c.cloud, *c.pass_[:3])
    assert orc.voxel_grid(c.cloud[idx], c.leaf) is None
    f = make_filter(F, "exact", pass_=c.pass_)
    f.setInputCloud(c.cloud)
    same_cloud(f.filter(), c.cloud[idx])
    assert f.counts() == (len(idx), len(idx))


def test_voxel_grid_without_pass_through_counts_the_finite_points(F, orc):
    """n_pass of include/pft_filters.h: VoxelGrid skips non-finite points, PassThrough or not"""
    c = fc.nan_cloud()
    fin = np.flatnonzero(fc.finite_mask(c.cloud))
    assert 0 < len(fin) < len(c.cloud)
    g = F.VoxelGrid()
    g.setLeafSize(0.01)
    g.setInputCloud(c.cloud)
    got = g.filter()
    assert g.counts()[0] == len(fin)
    np.testing.assert_array_equal(g.passIndices(), fin)
    same_cloud(got, orc.voxel_grid(c.cloud, 0.01))
    a = F.ApproximateVoxelGrid()  # takes every point
    a.setInputCloud(c.cloud)
    a.filter()
    assert a.counts()[0] == len(c.cloud)


@pytest.mark.parametrize("mode", sorted(fc.REUSE_MODES))
def test_one_handle_over_clouds_of_very_different_sizes(F, orc, mode):
    """no setter between the applies: the handle, created for 1024 points, grows twice, and every shorter cloud runs
    over the keys, heads, flags and tile counts its longer predecessor left"""
    m, pass_ = fc.REUSE_MODES[mode]
    f = make_filter(F, m, pass_=pass_)
    f._set(max_points=1024)  # (no public setter: the default capacity, a qhd frame, would never grow here)
    handle = None
    for cloud in fc.reuse_clouds():
        c = fc.case("reuse", cloud, m, pass_=pass_)
        f.setInputCloud(cloud)
        got = f.filter()
        assert handle is None or f._h is handle
        handle = f._h
        check_last_apply(f, got, fc.expected(orc, c))


@pytest.mark.parametrize("c", [fc.exact_long_runs(), fc.pairings(fc.PAIRING_PASSES[0], "approx")], ids=lambda c: c.name)
def test_device_input_gives_the_same_bytes(F, orc, c):
    import torch

    f = make_filter(F, c.mode, c.leaf, c.hist, c.pass_)
    f.setInputCloud(c.cloud)
    host = f.filter()
    dev = torch.from_numpy(c.cloud.view(np.uint8).reshape(-1).copy()).cuda()
    f.setInputCloudDevice(dev.data_ptr(), len(c.cloud), keepalive=dev)
    ptr, n = f.filterDevice()
    assert ptr and n == len(host)
    got = f.output()
    same_cloud(got, host)
    check_last_apply(f, got, fc.expected(orc, c))
