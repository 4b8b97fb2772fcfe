"""NumPy restatement of the population statistics (include/pft.h pft_population_stats) for the
tests: from a population as getParticles() returns it, the representative state as getResult() returns it and the
thresholds to every field of the block.  The sums are match_model.tree_sum (adjacent pairs in double, +0.0 padding); the
position ellipsoid goes through report_model.solve.  Every operation is one IEEE double (or float) operation, in the order
the definition states, so the device is compared with it bit for bit.  It needs no oracle tracker."""
import numpy as np

import match_model as mm
import report_model as rm

POSE = ("x", "y", "z", "roll", "pitch", "yaw")
D = np.float64
F = np.float32
N_SUMS = 29
SUM_NAMES = ["sum_w", "sum_w2"] + ["s%d" % k for k in range(6)] + ["S%d%d" % (k, l) for k in range(6) for l in range(k, 6)]
DOUBLE_FIELDS = ("sum_w", "sum_w2", "s", "S", "n_eff", "mean", "cov", "rpy_sigma")
FLOAT_FIELDS = ("pos_sigma", "pos_axes", "w_max")
INT_FIELDS = ("n", "n_zero", "i_max", "solve_info", "evaluated", "uncertain", "streak", "flagged")


def tri(k, l):
    """position of S_kl (k <= l) in the 21 values: the upper triangle row by row"""
    return k * 6 - k * (k - 1) // 2 + (l - k)


def terms(particles, pivot):
    """the 29 per-particle terms (n x 29, double): w, w * w, w * d_k, (w * d_k) * d_l for k <= l; pivot: six floats"""
    n = len(particles)
    w = particles["weight"].astype(F).astype(D)
    d = np.stack([particles[k].astype(F).astype(D) - D(F(pivot[a])) for a, k in enumerate(POSE)], 1) if n else np.zeros((0, 6), D)
    t = np.zeros((n, N_SUMS), D)
    t[:, 0] = w
    t[:, 1] = w * w
    for k in range(6):
        wd = w * d[:, k]
        t[:, 2 + k] = wd
        for l in range(k, 6):
            t[:, 8 + tri(k, l)] = wd * d[:, l]
    return t


def sums(particles, pivot):
    """the 29 tree sums {sum_w, sum_w2, s[6], S[21]} as one float64 array"""
    t = terms(particles, pivot)
    return np.array([mm.tree_sum(t[:, q]) for q in range(N_SUMS)], D)


def integers(particles):
    """n, n_zero, w_max, i_max (the lowest index on a tie; 0 and 0.0 for an empty population)"""
    w = particles["weight"].astype(F)
    n = len(w)
    if n == 0:
        return 0, 0, F(0), 0
    i_max = int(np.argmax(w))  # the first occurrence of the maximum
    return n, int((w == F(0)).sum()), F(w[i_max]), i_max


def finalize(sm, n, n_zero, w_max, i_max, pivot, max_pos_sigma=np.inf, min_n_eff=0.0, after=1, prev_streak=0):
    """the one-lane part: every derived field and the spread rule from the 29 sums; plain double + - x /, correctly rounded
    square roots, report_model.solve on the float 3 x 3 position block"""
    sm = np.asarray(sm, D)
    sum_w, sum_w2 = D(sm[0]), D(sm[1])
    out = dict(sum_w=sum_w, sum_w2=sum_w2, s=sm[2:8].copy(), S=sm[8:29].copy(), n=int(n), n_zero=int(n_zero),
               w_max=F(w_max), i_max=int(i_max), evaluated=1)
    if sum_w == 0.0:
        out.update(n_eff=D(0), mean=np.zeros(6, D), cov=np.zeros((6, 6), D), rpy_sigma=np.zeros(3, D),
                   pos_sigma=np.zeros(3, F), pos_axes=np.zeros((3, 3), F), solve_info=0)
    else:
        with np.errstate(all="ignore"):
            out["n_eff"] = D(sum_w * sum_w) / sum_w2 if sum_w2 > 0.0 else D(0)
            m = np.array([D(sm[2 + k]) / sum_w for k in range(6)], D)
            out["mean"] = np.array([D(F(pivot[k])) + m[k] for k in range(6)], D)
            cov = np.zeros((6, 6), D)
            for k in range(6):
                for l in range(k, 6):
                    c = D(D(sm[8 + tri(k, l)]) / sum_w) - D(m[k] * m[l])
                    cov[k, l] = cov[l, k] = c
            out["cov"] = cov
            c3 = [[F(cov[r, c]) for c in range(3)] for r in range(3)]
            evals, axes, info = rm.solve(c3, None)
            out["pos_sigma"] = np.array([F(np.sqrt(e if e > F(0) else F(0))) for e in evals], F)
            out["pos_axes"] = np.array(axes, F).reshape(3, 3)
            out["solve_info"] = int(info)
            out["rpy_sigma"] = np.array([np.sqrt(cov[3 + a, 3 + a] if cov[3 + a, 3 + a] > 0.0 else D(0)) for a in range(3)], D)
    uncertain = bool(D(out["pos_sigma"][2]) > D(max_pos_sigma) or out["n_eff"] < D(min_n_eff))
    streak = prev_streak + 1 if uncertain else 0
    out.update(uncertain=int(uncertain), streak=int(streak), flagged=int(streak >= after))
    return out


def stats(particles, result, max_pos_sigma=np.inf, min_n_eff=0.0, after=1, prev_streak=0):
    """what pft_spread reports for the population `particles` (getParticles()) around `result` (getResult())"""
    pivot = [F(result[k]) for k in POSE]
    n, n_zero, w_max, i_max = integers(particles)
    return finalize(sums(particles, pivot), n, n_zero, w_max, i_max, pivot, max_pos_sigma, min_n_eff, after, prev_streak)


class SpreadRule:
    """uncertain = pos_sigma[2] > max_pos_sigma or n_eff < min_n_eff (in double); streak = uncertain ? streak + 1 : 0;
    flagged = streak >= after.  A call that was not evaluated leaves all three as they were"""

    def __init__(self, max_pos_sigma=np.inf, min_n_eff=0.0, after=1):
        assert max_pos_sigma >= 0.0 and min_n_eff >= 0.0 and after >= 1
        self.max_pos_sigma, self.min_n_eff, self.after = float(max_pos_sigma), float(min_n_eff), int(after)
        self.uncertain, self.streak, self.flagged = False, 0, False

    def step(self, pos_sigma_max, n_eff, evaluated=True):
        if evaluated:
            self.uncertain = bool(D(F(pos_sigma_max)) > D(self.max_pos_sigma) or D(n_eff) < D(self.min_n_eff))
            self.streak = self.streak + 1 if self.uncertain else 0
            self.flagged = self.streak >= self.after
        return bool(self.uncertain), int(self.streak), bool(self.flagged)

    def reset(self):
        self.uncertain, self.streak, self.flagged = False, 0, False


def bits(a):
    """the bit pattern of a float64 / float32 value or array, for exact comparisons that tell -0.0 from +0.0"""
    a = np.asarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def compare(got, want, what=""):
    """every field of a PopulationStats (tracker.py) against the model's dict, bit for bit; returns the list of differences"""
    bad = []
    for f in DOUBLE_FIELDS:
        g, w = np.asarray(getattr(got, f), D).reshape(-1), np.asarray(want[f], D).reshape(-1)
        if bits(g).tolist() != bits(w).tolist():
            bad.append((what, f, g.tolist(), w.tolist()))
    for f in FLOAT_FIELDS:
        g, w = np.asarray(getattr(got, f), F).reshape(-1), np.asarray(want[f], F).reshape(-1)
        if bits(g).tolist() != bits(w).tolist():
            bad.append((what, f, g.tolist(), w.tolist()))
    for f in INT_FIELDS:
        if int(getattr(got, f)) != int(want[f]):
            bad.append((what, f, int(getattr(got, f)), int(want[f])))
    return bad
