"""The constructions of tests/leaf_cases.py, checked on the CPU with the oracle alone: the leaves hold the intended numbers of
records, the crop is the whole cloud, the identity particle's queries reach the intended record at the intended float
distance, the ties are ties, and the gate pair lies on either side of max_distance^2."""
import numpy as np
import pytest

import leaf_cases


@pytest.fixture(scope="module")
def cases():
    return {c.name: c for c in leaf_cases.all_cases()}


def oracle_eval(orc, c):
    o = orc.Tracker(orc.default_config(particle_num=c.P, seed=1, threads=0, emulate_pcl_alloc=0))
    o.set_reference(c.model)
    o.set_trans(np.eye(4, dtype=np.float32))
    o.set_input(c.cloud)
    return o.eval_weights(c.particles, want_nn=True)


def test_case_names(cases):
    assert tuple(cases) == leaf_cases.CASE_NAMES
    for c in cases.values():
        assert 4 <= c.P <= 64 and 64 <= len(c.model) <= 256


@pytest.mark.parametrize("name", leaf_cases.CASE_NAMES)
def test_leaf_sizes_are_as_constructed(orc, cases, name):
    c = cases[name]
    keys = orc.Octree(c.cloud).point_keys()
    codes = (keys[:, 0].astype(np.int64) << 40) | (keys[:, 1].astype(np.int64) << 20) | keys[:, 2].astype(np.int64)
    seen = set()
    for first, size in c.clusters:
        mine = set(codes[first:first + size].tolist())
        assert len(mine) == 1, (name, first, size)  # one leaf ...
        assert not (mine & seen), (name, first)     # ... of its own
        seen |= mine
    assert sum(s for _, s in c.clusters) == len(c.cloud)
    if name.startswith("sizes"):
        assert sorted(s for _, s in c.clusters)[-1] == 9 and {1, 2, 3, 4, 5} <= {s for _, s in c.clusters}
        assert c.end[1] == (5 if name.endswith("odd") else 4)
        assert (keys[c.end[0]] >= keys).all()  # the largest key on every axis: the last leaf of the linearised tree
    if name.startswith("crop_"):
        assert len(c.cloud) == int(name[5:])


@pytest.mark.parametrize("name", leaf_cases.CASE_NAMES)
def test_oracle_gives_the_intended_winners(orc, cases, name):
    c = cases[name]
    O = oracle_eval(orc, c)
    if not c.whole_crop:
        assert len(O["crop_idx"]) == 0 and (O["raw"] == 0).all()
        return
    np.testing.assert_array_equal(O["crop_idx"], np.arange(len(c.cloud)))
    assert c.expect
    for qi, idx, d2 in c.expect:  # particle 0 is the identity
        assert O["nn_idx"][0, qi] == idx, (name, qi)
        assert O["nn_d2"][0, qi].tobytes() == np.float32(d2).tobytes(), (name, qi)
    xyz = np.stack([c.cloud["x"], c.cloud["y"], c.cloud["z"]], 1)
    q = np.stack([c.model["x"], c.model["y"], c.model["z"]], 1)
    for qi, tie in c.ties:  # the same float distance to every record of the tie, and the earliest one reported
        d = xyz[tie] - q[qi]
        dd = d[:, 0] * d[:, 0] + (d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
        assert dd.dtype == np.float32 and len(set(dd.tobytes()[4 * i:4 * i + 4] for i in range(len(tie)))) == 1
        assert O["nn_idx"][0, qi] == min(tie)
    if name.startswith("sizes"):
        assert len(c.ties) >= len(leaf_cases.TIES)
        positions = {(tuple(t[2]), len(t[0])) for t in leaf_cases.TIES}
        assert {((0, 1), 4), ((1, 2), 4), ((0, 3), 4)} <= positions  # first two, middle two, first and last
        # every position of every size wins for some query
        won = {int(i) for i in O["nn_idx"][0]}
        assert sorted(s for _, s in c.swept) == sorted([1, 1, 2, 3, 4, 5, 9, c.end[1]])
        for first, size in c.swept:
            assert set(range(first, first + size)) <= won, (name, first, size)
    for qi, idx, inside in c.gate:
        assert (float(O["nn_d2"][0, qi]) < 0.1 * 0.1) == inside
        assert abs(float(O["nn_d2"][0, qi]) - 0.01) < 2e-9  # within two float steps of the gate
    if c.gate:
        assert {g[2] for g in c.gate} == {True, False}


def test_mixed_wave_is_one_wave_of_sizes_one_and_five(orc, cases):
    c = cases["mixed_wave"]
    assert len(c.model) == 64
    O = oracle_eval(orc, c)
    size_of = {}
    for first, size in c.clusters:
        for i in range(first, first + size):
            size_of[i] = size
    sizes = [size_of[int(i)] for i in O["nn_idx"][0]]
    assert sizes.count(1) >= 24 and sizes.count(5) >= 24 and set(sizes) == {1, 5}
