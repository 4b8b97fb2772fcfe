"""CPU-only proof, with the oracle alone, that the inputs of tests/colour_cases.py are what the GPU tests take them for: the
oracle's integer RGB2HSV agrees with textbook HSV over all 2^24 colours (an independent restatement in numpy), the colour
lists reach every hue, the hue-difference tie and the edge classes, and the two rigs isolate one pair per particle (and put
pairs on both sides of, and exactly on, the gate) in the approximate and in the exact search mode."""
import numpy as np
import pytest

import colour_cases as cc
from pcl_tracking_amd import scene

PAIR_SEEDS = range(8)  # the seeds tests/test_gpu_colour_path.py uses
PAIR_AMP = 0.01


def test_div_table_has_no_entry_near_a_rounding_tie(orc):
    """lrint on the oracle's side and __double2int_rn on the device's round 1044480 / i: no quotient lies within 0.004 of a
    tie (measured: 0.0047), so the two cannot disagree whatever the last bits of the division"""
    i = np.arange(1, 256)
    frac = (1044480 % i) / i
    assert np.abs(frac - 0.5).min() > 0.004
    for k in (1, 2, 3, 127, 254, 255):
        assert orc.lib().orc_div_table(int(k)) == int(np.floor(1044480.0 / k + 0.5))
    assert orc.lib().orc_div_table(0) == 0


@pytest.mark.parametrize("argorder", [1, 0])
def test_oracle_rgb2hsv_agrees_with_textbook_hsv_over_all_colours(orc, argorder):
    """circular |h - H / 2| < 1.1 and |s - 255 S| < 1.1 (measured maxima 1.088 and 1.016), v == max(r, g, b)"""
    cfg = orc.default_config(hsv_pcl180_argorder=argorder)
    worst_h = worst_s = 0.0
    for lo in range(0, 1 << 24, 1 << 20):
        rgba = np.arange(lo, lo + (1 << 20), dtype=np.uint32) | np.uint32(0x5a000000)
        k = orc.hsv_pack_many(cfg, rgba)
        h, s, v = (k & 0xff).astype(np.float64), ((k >> 8) & 0xff).astype(np.float64), ((k >> 16) & 0xff).astype(np.float64)
        assert (k >> 24 == 0).all() and h.max() <= 179 and s.max() <= 255
        r, g, b = ((rgba >> 16) & 0xff).astype(np.float64), ((rgba >> 8) & 0xff).astype(np.float64), (rgba & 0xff).astype(np.float64)
        if argorder:
            g, b = b, g  # RGB2HSV(Red, Blue, Green) as written upstream
        mx, mn = np.maximum(np.maximum(r, g), b), np.minimum(np.minimum(r, g), b)
        d = mx - mn
        dd = np.where(d > 0, d, 1.0)
        H = np.where(mx == r, (g - b) / dd, np.where(mx == g, 2.0 + (b - r) / dd, 4.0 + (r - g) / dd)) * 60.0
        H = np.where(d > 0, np.mod(H, 360.0), 0.0)
        S = np.where(mx > 0, d / np.where(mx > 0, mx, 1.0), 0.0)
        assert (v == mx).all()
        dh = np.abs(h - H / 2.0)
        dh = np.minimum(dh, 180.0 - dh)
        worst_h, worst_s = max(worst_h, dh.max()), max(worst_s, np.abs(s - 255.0 * S).max())
    print("argorder %d: worst |h - H/2| %.4f, worst |s - 255 S| %.4f" % (argorder, worst_h, worst_s))
    assert worst_h < 1.1 and worst_s < 1.1


def test_bulk_forms_are_the_single_colour_routines(orc):
    c, rgba = cc.targets()
    for argorder in (1, 0):
        cfg = orc.default_config(hsv_pcl180_argorder=argorder)
        k, f = orc.hsv_pack_many(cfg, rgba), orc.hsv_floats_many(cfg, rgba)
        for i, (r, g, b) in enumerate(c.tolist()):
            args = (r, b, g) if argorder else (r, g, b)
            h, s, v = orc.rgb2hsv_int(*args)
            assert int(k[i]) == h | s << 8 | v << 16
            assert f[i].tobytes() == np.array(orc.rgb2hsv(*args), np.float32).tobytes()
        # the alpha byte is ignored
        np.testing.assert_array_equal(orc.hsv_pack_many(cfg, rgba ^ np.uint32(0xff000000)), k)


def test_colour_lists_hold_what_they_claim():
    c, rgba = cc.targets()
    rc, rrgba = cc.refs()
    assert len(cc.EDGES) == 24 and len(set(cc.EDGES)) == 24
    assert len(c) == 256 and len(rc) == len(cc.EDGES) + len(cc.REF_HUES)
    assert [tuple(x) for x in c[:24].tolist()] == cc.EDGES and [tuple(x) for x in rc[:24].tolist()] == cc.EDGES
    assert cc.hsv_of(cc.hues())[:, 0].tolist() == list(range(180))
    assert cc.hsv_of(rc[24:])[:, 0].tolist() == list(cc.REF_HUES)
    assert len(np.unique(rgba >> 24)) > 100 and len(np.unique(rrgba >> 24)) > 10  # alpha bytes vary
    np.testing.assert_array_equal(rgba & 0xffffff, (c[:, 0] << 16 | c[:, 1] << 8 | c[:, 2]).astype(np.uint32))
    for argorder in (1, 0):
        e = cc.hsv_of(cc.EDGES, argorder)
        assert (e[:5, :2] == 0).all() and e[0, 2] == 0 and e[1, 2] == 255  # greys: h = s = 0; black: v = 0
        assert (e[5:11, 1] == 255).all() and sorted(e[5:11, 0].tolist()) == [0, 30, 60, 90, 120, 150]
        # g - b = -1 rounds to hue 0 before the wrap; g - b = -17 gives -2 and wraps to 178
        assert sorted(e[11:15, 0].tolist()) == [0, 0, 2, 178]
        assert (e[15:18, 1] == 255).all() and (e[15:18, 2] == 1).all()
        assert (e[18:21, 1] == 1).all() and (e[18:21, 2] == 255).all()
        assert (e[21:24, 1] < 64).all() and (e[21:24, 2] == 255).all()
    h = cc.hsv_of(c)
    assert set(h[:, 0].tolist()) == set(range(180)) and 0 in h[:, 2] and 255 in h[:, 1] and 0 in h[:, 1]


def test_hue_tie_pairs_exist_in_the_cases():
    """hd1 == hd2 exactly for 68 of the 180 x 180 float hue pairs; REFS x TARGETS holds 67 pairs of colours on such a tie"""
    a, b = np.meshgrid(np.arange(180), np.arange(180), indexing="ij")
    tie = cc.hue_tie(a, b)
    assert tie.sum() == 68 and (np.abs(a - b)[tie] == 90).all()
    rh, th = cc.hsv_of(cc.refs()[0])[:, 0], cc.hsv_of(cc.targets()[0])[:, 0]
    assert cc.hue_tie(rh[:, None], th[None, :]).sum() == 67


def run_oracle(orc, rig, exact, **params):
    cfg = orc.default_config(particle_num=256, threads=0, emulate_pcl_alloc=0, exact_nearest=exact,
                             max_distance=rig["max_distance"], **params)
    o = orc.Tracker(cfg)
    o.set_reference(rig["model"])
    o.set_input(rig["cloud"])
    return cfg, o.eval_weights(rig["particles"], want_nn=True)


def single_pair_value(orc, cfg, rig, i):
    """-(float)(DistanceCoherence x HSVColorCoherence) of model point A under particle i and cloud point i"""
    p = rig["particles"][i]
    moved = orc.transform_cloud(rig["model"][:1], orc.get_transformation(p["x"], p["y"], p["z"], 0.0, 0.0, 0.0))
    tgt = rig["cloud"][i]
    val = 0.0 + 1.0 * orc.distance_coherence(cfg, moved[0], tgt) * orc.hsv_coherence(cfg, moved[0]["rgba"], tgt["rgba"])
    return -np.float32(val)


@pytest.mark.parametrize("exact", [0, 1])
def test_pair_rig_isolates_one_pair_per_particle(orc, exact):
    rc, rrgba = cc.refs()
    _, trgba = cc.targets()
    for seed in PAIR_SEEDS:
        rig = cc.pair_rig(rrgba[(5 * seed) % len(rrgba)], trgba, seed, PAIR_AMP)
        cfg, O = run_oracle(orc, rig, exact, hsv_weight=4.0, v_weight=1.0)
        gate = cfg.max_distance ** 2
        assert (O["nn_d2"][:, 1].astype(np.float64) >= gate).all()  # B is outside the gate for every particle
        own = cc.own_paired(O) & (O["nn_d2"][:, 0].astype(np.float64) < gate)
        print("pair rig seed %d exact %d: own-paired share %.4f, crop %d" % (seed, exact, own.mean(), len(O["crop_idx"])))
        assert own.mean() >= (1.0 if exact else 0.90)
        assert (O["nn_d2"][rig["zero_offset"], 0] == 0).all() and rig["zero_offset"].sum() == 64
        assert (O["nn_d2"][own & ~rig["zero_offset"], 0] > 0).mean() > 0.99
        want = np.array([single_pair_value(orc, cfg, rig, i) for i in np.flatnonzero(own)], np.float32)
        assert O["raw"][own].tobytes() == want.tobytes()
        assert (want < 0).all() and len(np.unique(want)) > 0.9 * len(want)
    assert rig["zero_offset"][own].any()


@pytest.mark.parametrize("exact", [0, 1])
def test_pair_rig_without_offsets_pairs_every_particle(orc, exact):
    rig = cc.pair_rig(cc.refs()[1][0], cc.targets()[1], 0, 0.0)
    cfg, O = run_oracle(orc, rig, exact)
    assert cc.own_paired(O).all() and (O["nn_d2"][:, 0] == 0).all()


@pytest.mark.parametrize("exact", [0, 1])
def test_gate_rig_puts_pairs_on_inside_and_outside_the_gate(orc, exact):
    rig = cc.gate_rig()
    cfg, O = run_oracle(orc, rig, exact)
    assert cfg.max_distance ** 2 == 0.015625 and np.float32(cfg.max_distance ** 2) == np.float32(0.015625)
    own, kind = cc.own_paired(O), rig["kind"]
    d2, raw = O["nn_d2"][:, 0], O["raw"]
    counts = [int((own & (kind == k)).sum()) for k in range(3)]
    print("gate rig exact %d: own-paired per kind %s of %s" % (exact, counts, [int((kind == k).sum()) for k in range(3)]))
    for k in range(3):
        assert counts[k] == (kind == k).sum() if exact else counts[k] >= 50
    assert (d2[own & (kind == 0)] == np.float32(0.015625)).all() and (raw[own & (kind == 0)] == 0).all()
    assert (d2[own & (kind == 1)] < np.float32(0.015625)).all() and (raw[own & (kind == 1)] != 0).all()
    assert (d2[own & (kind == 2)] > np.float32(0.015625)).all() and (raw[own & (kind == 2)] == 0).all()
    # a position one float off the gate: squared distances within 1e-5 (relative) of it, so kind 2 lies inside the slack of
    # the exact search's float pruning bounds (gate * 1.0001) and kind 1 must survive them
    assert d2[own & (kind == 1)].min() > 0.015625 * (1 - 1e-5) and d2[own & (kind == 2)].max() < 0.015625 * (1 + 1e-5)
    assert (O["nn_d2"][:, 1].astype(np.float64) >= 0.015625).all()
