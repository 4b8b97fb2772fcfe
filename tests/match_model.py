"""NumPy restatement of the match statistics (pft_match) for the tests: the statistics of one
result pose from the CPU oracle's nearest-neighbour arrays, the two summation orders, and the lost rule.

The search itself is the oracle's (oracle.Tracker.eval_weights with the device's transform and crop box); this module only
turns its (nn_idx, nn_d2) into what pft_match reports.
"""
import numpy as np


def tree_sum(v):
    """adjacent-pair tree in double over positions 0 .. n-1, padded with +0.0 to a power of two"""
    v = np.asarray(v, np.float64)
    n = 1
    while n < len(v):
        n *= 2
    w = np.zeros(n, np.float64)
    w[:len(v)] = v
    while len(w) > 1:
        w = w[0::2] + w[1::2]
    return float(w[0])


def chain_sum(v):
    """index-order chain in double from +0.0"""
    s = np.float64(0.0)
    for x in np.asarray(v, np.float64):
        s = s + x
    return float(s)


def stored_order(reference):
    """the order a handle stores its reference cloud in (pft_set_reference): ascending 30-bit Morton code of the
    coordinates quantised in float to 1 024 steps of the largest extent, x the most significant of each triple, ties by
    index.  pft_match's tree sums run over these positions"""
    c = np.stack([reference["x"], reference["y"], reference["z"]], 1).astype(np.float32)
    n = len(c)
    if n == 0:
        return np.zeros(0, np.int64)
    fin = np.isfinite(c)
    lo = np.where(fin, c, np.float32(np.inf)).min(axis=0).astype(np.float32)
    hi = np.where(fin, c, np.float32(-np.inf)).max(axis=0).astype(np.float32)
    ext = np.float32(0.0)
    for a in range(3):
        if hi[a] >= lo[a]:
            ext = max(ext, np.float32(hi[a] - lo[a]))
    scale = np.float32(1023.0) / ext if ext > 0 else np.float32(0.0)
    with np.errstate(invalid="ignore"):
        v = np.where(fin, ((c - lo).astype(np.float32) * scale).astype(np.float32), np.float32(0.0))
    q = np.minimum(np.float32(1023.0), np.maximum(np.float32(0.0), v)).astype(np.uint64)
    code = np.zeros(n, np.uint64)
    for b in range(9, -1, -1):
        code = (code << np.uint64(3)) | (((q[:, 0] >> np.uint64(b)) & np.uint64(1)) << np.uint64(2)) | \
               (((q[:, 1] >> np.uint64(b)) & np.uint64(1)) << np.uint64(1)) | ((q[:, 2] >> np.uint64(b)) & np.uint64(1))
    return np.argsort(code, kind="stable")


def gate(max_distance):
    """the likelihood's gate: (double)d2 < max_distance * max_distance"""
    return np.float64(max_distance) * np.float64(max_distance)


def pair_values(orc, cfg, reference, transform, frame, nn_idx, crop_idx, matched):
    """DistanceCoherence x HSVColorCoherence of every matched pair, the oracle's bits; 0.0 elsewhere"""
    m = np.eye(4, dtype=np.float32)
    t = np.asarray(transform, np.float32)
    m[:t.shape[0], :] = t
    moved = orc.transform_cloud(reference, m)
    out = np.zeros(len(reference), np.float64)
    for j in np.flatnonzero(matched):
        tgt = frame[crop_idx[nn_idx[j]]]
        out[j] = np.float64(1.0) * orc.distance_coherence(cfg, moved[j], tgt) * orc.hsv_coherence(cfg, moved[j]["rgba"], tgt["rgba"])
    return out


def stats(orc, cfg, reference, transform, frame, nn_idx, nn_d2, crop_idx):
    """what pft_match reports for one pose, from the oracle's search results (arrays in the caller's reference order):
    coherence / sum_sq_dist as index-order chains over the matched pairs, coherence_tree / sum_sq_dist_tree as the device
    forms them, adjacent-pair trees over the handle's stored order"""
    nn_idx = np.asarray(nn_idx, np.int64)
    d2 = np.asarray(nn_d2, np.float32)
    matched = (nn_idx >= 0) & (d2.astype(np.float64) < gate(cfg.max_distance))
    input_idx = np.full(len(nn_idx), -1, np.int64)
    input_idx[matched] = np.asarray(crop_idx, np.int64)[nn_idx[matched]]
    val = pair_values(orc, cfg, reference, transform, frame, nn_idx, crop_idx, matched)
    sq = np.where(matched, d2.astype(np.float64), 0.0)
    o = stored_order(reference)
    return dict(n_matched=int(matched.sum()), matched=matched, input_idx=input_idx.astype(np.int32), sq_dist=d2,
                coherence=chain_sum(val), sum_sq_dist=chain_sum(sq), coherence_tree=tree_sum(val[o]),
                sum_sq_dist_tree=tree_sum(sq[o]), n_crop=len(crop_idx))


class LostRule:
    """below = n_matched < min_ratio * M (in double); streak = below ? streak + 1 : 0; lost = streak >= lost_after.
    A frame that was not evaluated leaves all three as they were"""

    def __init__(self, min_ratio=0.0, lost_after=1):
        assert 0.0 <= min_ratio <= 1.0 and lost_after >= 1
        self.min_ratio, self.lost_after = float(min_ratio), int(lost_after)
        self.below, self.streak, self.lost = False, 0, False

    def step(self, n_matched, n_reference, evaluated=True):
        if evaluated:
            self.below = np.float64(n_matched) < np.float64(self.min_ratio) * np.float64(n_reference)
            self.streak = self.streak + 1 if self.below else 0
            self.lost = self.streak >= self.lost_after
        return bool(self.below), int(self.streak), bool(self.lost)

    def reset(self):
        self.below, self.streak, self.lost = False, 0, False
