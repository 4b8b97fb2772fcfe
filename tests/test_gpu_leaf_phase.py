"""The leaf phase of k_likelihood (first record peeled, winner carried in registers) on the constructions of
tests/leaf_cases.py, in both leaf-record forms: approximate-NN index and squared distance of EVERY (particle, point) pair
against the oracle without tolerance, the weights as tests/test_gpu_parity.py compares them, and the weights of the product
instance (no NN arrays) byte for byte against those of the recording instance on the same handle.  tests/test_leaf_cases.py
shows on the CPU that the cases hold the leaf sizes, ties and gate distances they are meant to."""
import ctypes as C

import numpy as np
import pytest

import leaf_cases
from octree_model import decode_variant

pytestmark = pytest.mark.gpu


def ulp_diff(a, b):
    a = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64)
    a = np.where(a < 0, -(a & 0x7FFFFFFF), a)
    b = np.where(b < 0, -(b & 0x7FFFFFFF), b)
    return np.abs(a - b)


def ancestor_table_info(g):
    """pft_debug_get_ancestor_table's header: [0] filled for the last tree, [1] its level, [8] == [9] the epochs agree"""
    info, tab = np.zeros(10, np.uint32), np.zeros(1 << 18, np.uint32)
    g._check(g._L.pft_debug_get_ancestor_table(g._h, info.ctypes.data_as(C.c_void_p), tab.ctypes.data_as(C.c_void_p), len(tab)))
    return info


@pytest.fixture(scope="module")
def gpu():
    from pcl_tracking_amd import tracker

    return tracker


@pytest.fixture(scope="module")
def cases():
    return {c.name: c for c in leaf_cases.all_cases()}


@pytest.fixture(scope="module")
def oracle_results():
    return {}  # case name -> the oracle's eval_weights, computed once and shared by the two leaf forms


@pytest.mark.parametrize("indirect", [False, True], ids=["copied", "followed"])
@pytest.mark.parametrize("name", leaf_cases.CASE_NAMES)
def test_leaf_phase_against_the_oracle(gpu, orc, cases, oracle_results, monkeypatch, name, indirect):
    monkeypatch.setenv("PFT_LEAF_INDIRECT", "1" if indirect else "0")  # latched by the handle
    c = cases[name]
    g = gpu.make_reference_tracker(particle_num=c.P, seed=1)
    g.setReferenceCloud(c.model)
    g.setTrans(np.eye(4, dtype=np.float32))
    g.setInputCloud(c.cloud)
    # the builder's mode (who copies the leaf records, whether a table is filled) follows the crop size of the PREVIOUS
    # build, and a fresh handle has none: one evaluation first, so that the compared ones run the route of their size
    g.evalWeights(c.particles)
    G = g.evalWeights(c.particles, want_nn=True)
    if name not in oracle_results:
        o = orc.Tracker(orc.default_config(particle_num=c.P, seed=1, threads=0, emulate_pcl_alloc=0))
        o.set_reference(c.model)
        o.set_trans(np.eye(4, dtype=np.float32))
        o.set_input(c.cloud)
        oracle_results[name] = o.eval_weights(c.particles, want_nn=True, mats=g.debugPoseToMatrix(c.particles))
    O = oracle_results[name]
    np.testing.assert_array_equal(G["crop_idx"], O["crop_idx"])
    if not c.whole_crop:  # empty crop: no correspondence anywhere
        assert len(G["crop_idx"]) == 0
        assert (G["nn_idx"] == -1).all() and np.isinf(G["nn_d2"]).all() and (G["raw"] == 0).all() and (O["raw"] == 0).all()
        assert g.evalWeights(c.particles)["raw"].tobytes() == G["raw"].tobytes()
        return
    assert len(G["crop_idx"]) == len(c.cloud)
    tree = g.debugGetTree()
    # proof of the route: the kernel's own record of its instance and layout, the builder's of who wrote the leaf records
    # (0 the gather launch, 1 the builder, 2 nobody: the records are followed), and the ancestor table's header
    lay, variant, anc = G["lik_layout"], decode_variant(tree["build_variant"]), ancestor_table_info(g)
    print(name, "indirect" if indirect else "direct", lay, variant, anc, g.debugAncestorLevel())
    assert tree["leaf_indirect"] == int(indirect) and lay["valid"]
    assert lay["indirect"] == lay["leaf_indirect"] == indirect
    assert (lay["layout"], lay["descent"]) == ("u16_leaf_starts", "fast"), lay
    gathered = not indirect and len(c.cloud) > 5000
    assert variant["leaf_mode"] == (2 if indirect else 0 if gathered else 1), variant
    if gathered:  # crop_5001, copied form: the table of level depth - 2 was filled for this tree and this instance uses it
        assert name == "crop_5001"
        assert anc[0] == 1 and anc[1] == G["octree_depth"] - 2 and anc[8] == anc[9], anc
        assert g.debugAncestorLevel()["instance"] == 2
    else:
        assert anc[0] == 0, anc
    assert G["octree_depth"] == O["octree_depth"] and G["n_leaves"] == len(c.clusters)
    # every pair, no tolerance
    assert G["nn_idx"].shape == O["nn_idx"].shape == (c.P, len(c.model))
    np.testing.assert_array_equal(G["nn_idx"], O["nn_idx"])
    np.testing.assert_array_equal(G["nn_d2"].view(np.uint32), O["nn_d2"].view(np.uint32))
    assert G["scan_queries"] == O["scan_queries"] and G["scan_points"] == O["scan_points"]
    d = ulp_diff(G["raw"], O["raw"])
    assert d.max() <= 1, d.max()
    assert (d == 0).mean() > 0.99
    # what the construction predicts for the identity particle: winners at every position, the earlier record of a tie
    for qi, idx, d2 in c.expect:
        assert G["nn_idx"][0, qi] == idx and G["nn_d2"][0, qi].tobytes() == np.float32(d2).tobytes(), (name, qi)
    for qi, tie in c.ties:
        assert G["nn_idx"][0, qi] == min(tie)
    if c.end:  # the last leaf of the arrays: le == n_crop
        first, size = c.end
        np.testing.assert_array_equal(tree["leaf_order"][-size:], np.arange(first, first + size))
    # the product instance on the same handle (crop_5001, copied form: behind a gather launch that filled the table again)
    assert g.evalWeights(c.particles)["raw"].tobytes() == G["raw"].tobytes()
    if gathered:
        anc = ancestor_table_info(g)
        assert anc[0] == 1 and anc[8] == anc[9] and g.debugAncestorLevel()["instance"] in (1, 2), (anc, g.debugAncestorLevel())
