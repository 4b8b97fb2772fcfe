"""NumPy restatement of model creation (include/pft_segment.h): the rules recalled from PCL 1.8.0
that csrc/pft_segment.hip follows, one function per rule ("RULE <name>" there), float32 with explicit operation order.
Test infrastructure: the tests compare the device against it; PCL itself is not available, so parity stays unpinned."""
import math

import numpy as np

F = np.float32
INT_MAX = 2147483647
MAX_SAMPLE_CHECKS = 1000
DBL_EPS = np.finfo(np.float64).eps


# ---- RULE rng: boost::mt19937 written out, uniform_int<>(0, INT_MAX) = engine() >> 1 ----
class MT19937:
    def __init__(self, seed=5489):
        self.mt = [0] * 624
        self.mt[0] = seed & 0xFFFFFFFF
        for i in range(1, 624):
            x = self.mt[i - 1]
            self.mt[i] = (1812433253 * (x ^ (x >> 30)) + i) & 0xFFFFFFFF
        self.idx = 624

    def _twist(self):
        mt = self.mt
        for i in range(624):
            y = (mt[i] & 0x80000000) | (mt[(i + 1) % 624] & 0x7FFFFFFF)
            mt[i] = mt[(i + 397) % 624] ^ (y >> 1) ^ (0x9908B0DF if y & 1 else 0)
        self.idx = 0

    def __call__(self):
        if self.idx >= 624:
            self._twist()
        y = self.mt[self.idx]
        self.idx += 1
        y ^= y >> 11
        y ^= (y << 7) & 0x9D2C5680
        y ^= (y << 15) & 0xEFC60000
        y ^= y >> 18
        return y & 0xFFFFFFFF


def uniform_int_0_intmax(engine):
    """boost::uniform_int<>(0, INT_MAX) over a 32-bit engine: brange = 2^32 - 1, range + 1 = 2^31, so bucket_size =
    brange / 2^31 = 1, and brange % 2^31 == range increments it to 2; result = engine() / 2, always <= INT_MAX"""
    brange, rng = 0xFFFFFFFF, INT_MAX
    bucket = brange // (rng + 1)
    if brange % (rng + 1) == rng:
        bucket += 1
    while True:
        r = engine() // bucket
        if r <= rng:
            return r


# ---- RULE draw: drawIndexSample over a sparse shuffled_indices_ that is never reset ----
class Sampler:
    def __init__(self, n, seed=12345):
        self.n = n
        self.eng = MT19937(seed)
        self.map = {}

    def _get(self, k):
        return self.map.get(k, k)

    def draw(self):
        for i in range(3):
            j = i + uniform_int_0_intmax(self.eng) % (self.n - i)
            a, b = self._get(i), self._get(j)
            self.map[i], self.map[j] = b, a
        return [self._get(0), self._get(1), self._get(2)]


# ---- RULE good: isSampleGood ----
def sample_good(p0, p1, p2):
    with np.errstate(divide="ignore", invalid="ignore"):
        r = [F(F(p1[k] - p0[k]) / F(p2[k] - p0[k])) for k in range(3)]
    return bool(r[0] != r[1] or r[2] != r[1])


# ---- RULE coef: computeModelCoefficients ----
def plane_of(p0, p1, p2):
    p0, p1, p2 = (np.asarray(p, F) for p in (p0, p1, p2))
    a = [F(p1[k] - p0[k]) for k in range(3)]
    b = [F(p2[k] - p0[k]) for k in range(3)]
    c0 = F(F(a[1] * b[2]) - F(a[2] * b[1]))
    c1 = F(F(a[2] * b[0]) - F(a[0] * b[2]))
    c2 = F(F(a[0] * b[1]) - F(a[1] * b[0]))
    sq = F(F(F(c0 * c0) + F(c1 * c1)) + F(F(c2 * c2) + F(0)))
    nrm = F(np.sqrt(sq))
    with np.errstate(divide="ignore", invalid="ignore"):
        c0, c1, c2, c3 = F(c0 / nrm), F(c1 / nrm), F(c2 / nrm), F(F(0) / nrm)
    dot = F(F(F(c0 * p0[0]) + F(c1 * p0[1])) + F(F(c2 * p0[2]) + F(c3 * F(1))))
    return np.array([c0, c1, c2, F(F(-1) * dot)], F)


def float_bound_below(thr):
    """smallest float f with (double)x < thr <=> x < f: how PCL's float-against-double compares behave"""
    f = F(thr)
    if float(f) < thr:
        f = np.nextafter(f, F(np.inf))
    return f


# ---- RULE dist: |c . (x, y, z, 1)|, (a0 + a1) + (a2 + a3), strict ----
def distances(c, xyz):
    c = np.asarray(c, F)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    d = ((c[0] * x + c[1] * y).astype(F) + (c[2] * z + c[3] * F(1)).astype(F)).astype(F)
    return np.abs(d)


def within(c, xyz, thr):
    return distances(c, xyz) < float_bound_below(thr)


# ---- RULE loop: RandomSampleConsensus::computeModel ----
def ransac_stop(counts, n, max_iterations=1000, probability=0.99):
    """replay the loop over a sequence of inlier counts (None = no sample could be drawn);
    -> (iterations, best index or -1)"""
    log_probability = math.log(1.0 - probability)
    one_over = 1.0 / n
    k, best, best_h, it = 1.0, -INT_MAX, -1, 0
    for h, c in enumerate(counts):
        if not (it < k):
            break
        if c is None:
            break
        if c > best:
            best, best_h = c, h
            w = best * one_over
            p = 1.0 - math.pow(w, 3.0)
            p = max(DBL_EPS, p)
            p = min(1.0 - DBL_EPS, p)
            k = log_probability / math.log(p)
        it += 1
        if it > max_iterations:
            break
    return it, best_h


# ---- RULE eigen + refit: csrc/pft_segment_solve.h line for line ----
# branch bits of the record (include/pft_segment.h PFT_REFIT_*)
SCALE_TINY, C0_SMALL, A_CLAMPED, Q_CLAMPED, SWAP_01, SWAP_12, SWAP_01_AGAIN, R0_FALLBACK, D_NEGATIVE, PICK_0, PICK_1, \
    PICK_2, ZERO_LENGTH = (1 << k for k in range(13))
BRANCH_NAMES = ("scale_tiny", "c0_small", "a_clamped", "q_clamped", "swap_01", "swap_12", "swap_01_again", "r0_fallback",
                "d_negative", "pick_0", "pick_1", "pick_2", "zero_length")


def branch_names(bits):
    return [n for k, n in enumerate(BRANCH_NAMES) if bits >> k & 1]


def _roots2(b, c, t):
    d = F(float(F(b * b)) - 4.0 * float(c))
    if d < 0:
        d = F(0)
        t["branches"] |= D_NEGATIVE
    sd = F(np.sqrt(d))
    return [F(0), F(F(0.5) * F(b - sd)), F(F(0.5) * F(b + sd))]


def _roots(m, t, trig=None):
    m00, m01, m02, m11, m12, m22 = m[0, 0], m[0, 1], m[0, 2], m[1, 1], m[1, 2], m[2, 2]
    c0 = F(F(F(F(F(F(m00 * m11) * m22) + F(F(F(F(2) * m01) * m02) * m12)) - F(F(m00 * m12) * m12)) - F(F(m11 * m02) * m02))
           - F(F(m22 * m01) * m01))
    c1 = F(F(F(F(F(F(m00 * m11) - F(m01 * m01)) + F(m00 * m22)) - F(m02 * m02)) + F(m11 * m22)) - F(m12 * m12))
    c2 = F(F(m00 + m11) + m22)
    if abs(c0) < np.finfo(F).eps:
        t["branches"] |= C0_SMALL
        return _roots2(c2, c1, t)
    s_inv3 = F(1.0 / 3.0)
    s_sqrt3 = F(np.sqrt(F(3)))
    c2o3 = F(c2 * s_inv3)
    a_o3 = F(F(c1 - F(c2 * c2o3)) * s_inv3)
    if a_o3 > 0:
        a_o3 = F(0)
        t["branches"] |= A_CLAMPED
    half_b = F(F(0.5) * F(c0 + F(c2o3 * F(F(F(F(2) * c2o3) * c2o3) - c1))))
    q = F(F(half_b * half_b) + F(F(a_o3 * a_o3) * a_o3))
    if q > 0:
        q = F(0)
        t["branches"] |= Q_CLAMPED
    rho = F(np.sqrt(F(-a_o3)))
    ay = F(np.sqrt(F(-q)))
    at = F(np.arctan2(ay, half_b)) if trig is None else F(trig[0])
    theta = F(at * s_inv3)
    ct, st = (F(np.cos(theta)), F(np.sin(theta))) if trig is None else (F(trig[1]), F(trig[2]))
    t["trig_arg"] = np.array([ay, half_b, theta], F)
    t["trig"] = np.array([at, ct, st], F)
    r = [F(c2o3 + F(F(F(2) * rho) * ct)), F(c2o3 - F(rho * F(ct + F(s_sqrt3 * st)))),
         F(c2o3 - F(rho * F(ct - F(s_sqrt3 * st))))]
    if r[0] >= r[1]:
        r[0], r[1] = r[1], r[0]
        t["branches"] |= SWAP_01
    if r[1] >= r[2]:
        r[1], r[2] = r[2], r[1]
        t["branches"] |= SWAP_12
        if r[0] >= r[1]:
            r[0], r[1] = r[1], r[0]
            t["branches"] |= SWAP_01_AGAIN
    if r[0] <= 0:
        t["branches"] |= R0_FALLBACK
        return _roots2(c2, c1, t)
    return r


def eigen33_trace(mat, trig=None):
    """pcl::eigen33 (the smallest eigenvalue's vector) with the record of pft_segment_refit_debug: scale, trig_arg[3],
    trig[3], roots[3], len[3], branches, and `vec`.  trig = (atan2 value, cos, sin): used in place of NumPy's own, so that
    everything else can be compared bit for bit with a solve that ran on another libm"""
    mat = np.asarray(mat, F)
    t = {"branches": 0, "trig_arg": np.zeros(3, F), "trig": np.zeros(3, F)}
    scale = F(np.max(np.abs(mat)))
    if scale <= np.finfo(F).tiny:
        scale = F(1)
        t["branches"] |= SCALE_TINY
    t["scale"] = scale
    with np.errstate(all="ignore"):
        m = (mat / scale).astype(F)
        r = _roots(m, t, trig)
        t["roots"] = np.array(r, F)
        for k in range(3):
            m[k, k] = F(m[k, k] - r[0])
        vs, ls = [], []
        for a, b in ((0, 1), (0, 2), (1, 2)):
            A, B = m[a], m[b]
            v = [F(F(A[1] * B[2]) - F(A[2] * B[1])), F(F(A[2] * B[0]) - F(A[0] * B[2])),
                 F(F(A[0] * B[1]) - F(A[1] * B[0]))]
            vs.append(v)
            ls.append(F(F(v[0] * v[0]) + F(F(v[1] * v[1]) + F(v[2] * v[2]))))
        t["len"] = np.array(ls, F)
        if ls[0] >= ls[1] and ls[0] >= ls[2]:
            k = 0
        elif ls[1] >= ls[0] and ls[1] >= ls[2]:
            k = 1
        else:
            k = 2
        t["branches"] |= (PICK_0, PICK_1, PICK_2)[k]
        if ls[k] == 0:
            t["branches"] |= ZERO_LENGTH
        s = F(np.sqrt(ls[k]))
        t["vec"] = np.array([F(v / s) for v in vs[k]], F)
    return t


def eigen33(mat):
    return eigen33_trace(mat)["vec"]


def moment_terms(xyz):
    x, y, z = (xyz[:, k].astype(F) for k in range(3))
    return [(x * x).astype(F), (x * y).astype(F), (x * z).astype(F), (y * y).astype(F), (y * z).astype(F),
            (z * z).astype(F), x, y, z]


def moment_sums(xyz, order):
    """the nine sums: "pcl" sequential float sums in index order, "tree" adjacent-pair trees"""
    if order == "pcl":
        return np.array([F(np.cumsum(t, dtype=F)[-1]) for t in moment_terms(xyz)], F)
    from report_model import tree_sum
    return np.array([F(tree_sum(t)) for t in moment_terms(xyz)], F)


def moment_means(xyz, order):
    """the nine sums divided by the count"""
    return np.array([F(a / F(len(xyz))) for a in moment_sums(xyz, order)], F)


def solve_trace(accu, m, trig=None):
    """sg_refit_solve: from the nine means to the record (coef included)"""
    accu = np.asarray(accu, F)
    cov = np.zeros((3, 3), F)
    with np.errstate(all="ignore"):
        cov[0, 0] = F(accu[0] - F(accu[6] * accu[6]))
        cov[0, 1] = F(accu[1] - F(accu[6] * accu[7]))
        cov[0, 2] = F(accu[2] - F(accu[6] * accu[8]))
        cov[1, 1] = F(accu[3] - F(accu[7] * accu[7]))
        cov[1, 2] = F(accu[4] - F(accu[7] * accu[8]))
        cov[2, 2] = F(accu[5] - F(accu[8] * accu[8]))
        cov[1, 0], cov[2, 0], cov[2, 1] = cov[0, 1], cov[0, 2], cov[1, 2]
        t = eigen33_trace(cov, trig)
        e = t["vec"]
        dot = F(F(F(e[0] * accu[6]) + F(e[1] * accu[7])) + F(F(e[2] * accu[8]) + F(F(0) * F(1))))
        t["coef"] = np.array([e[0], e[1], e[2], F(F(-1) * dot)], F)
    t["m"] = int(m)
    t["accu"] = accu
    t["cov"] = np.array([cov[0, 0], cov[0, 1], cov[0, 2], cov[1, 1], cov[1, 2], cov[2, 2]], F)
    return t


def refit_trace(xyz, coef, order="pcl", trig=None):
    """optimizeModelCoefficients over the inlier points (in index order) in either summation order, with the record;
    fewer than 4 points: None (the coefficients stay).  `coef` is not read: the refit starts from the points alone, the
    parameter keeps the signature of `refit`, which hands it back below 4 points"""
    if len(xyz) < 4:
        return None
    return solve_trace(moment_means(xyz, order), len(xyz), trig)


def refit(xyz, coef, order="pcl"):
    t = refit_trace(xyz, coef, order)
    return np.asarray(coef, F) if t is None else t["coef"]


# ---- stages 1, 2, 5 ----
def transform(xyz, T):
    T = np.asarray(T, F).reshape(4, 4)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    out = np.empty_like(xyz)
    for r in range(3):
        out[:, r] = (((T[r, 0] * x).astype(F) + (T[r, 1] * y).astype(F)).astype(F) + (T[r, 2] * z).astype(F)).astype(F) \
            + T[r, 3]
    return out.astype(F)


def keep_nonzero(xyz):
    t = float_bound_below(0.01)
    with np.errstate(invalid="ignore"):
        zero = (np.abs(xyz[:, 0]) < t) & (np.abs(xyz[:, 1]) < t) & (np.abs(xyz[:, 2]) < t)
    return ~zero & ~np.isnan(xyz).any(axis=1)


def in_box(xyz, enable, lo, hi):
    keep = np.ones(len(xyz), bool)
    for a in range(3):
        if enable[a]:
            keep &= ~((xyz[:, a] < F(lo[a])) | (xyz[:, a] > F(hi[a])))
    return keep


# ---- RULE link / size / order: clusters ----
def clusters(xyz, tol, min_size, max_size):
    """-> list of index arrays into xyz, by size descending, ties by smallest index"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from scipy.spatial import cKDTree

    n = len(xyz)
    if n == 0:
        return []
    xyz = xyz.astype(F)
    pairs = cKDTree(xyz.astype(np.float64)).query_pairs(tol * 1.001 + 1e-9, output_type="ndarray")
    tol2 = F(tol * tol)
    if len(pairs):
        d = (xyz[pairs[:, 0]] - xyz[pairs[:, 1]]).astype(F)
        dd = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).astype(F) + d[:, 2] * d[:, 2]).astype(F)
        pairs = pairs[dd < tol2]
    g = coo_matrix((np.ones(len(pairs)), (pairs[:, 0], pairs[:, 1])) if len(pairs) else ([], ([], [])), shape=(n, n))
    _, lab = connected_components(g, directed=False)
    out = []
    for l in np.unique(lab):
        idx = np.flatnonzero(lab == l)
        if min_size <= len(idx) <= max_size:
            out.append(idx)
    out.sort(key=lambda a: (-len(a), a[0]))
    return out


# ---- the whole pipeline ----
def pipeline(points, transform_matrix=None, plane=True, max_iterations=1000, threshold=0.015, probability=0.99,
             seed=12345, optimize=True, box_enable=(1, 1, 0), box_lo=(0.45, -0.6, -0.17), box_hi=(1.1, 0.6, 0.2),
             tol=0.02, min_size=500, max_size=25000):
    xyz = np.stack([points["x"], points["y"], points["z"]], 1).astype(F)
    if transform_matrix is not None:
        xyz = transform(xyz, transform_matrix)
    valid = np.flatnonzero(keep_nonzero(xyz))
    cx = xyz[valid]
    n = len(cx)
    r = {"n_valid": n, "samples": [], "counts": [], "iterations": 0, "best": -1, "found": False}
    fin = np.zeros(n, bool)
    if plane:
        samples, counts = [], []
        if n >= 3:
            smp = Sampler(n, seed)
            limit = max_iterations + 1
            while len(samples) < limit:
                for _ in range(MAX_SAMPLE_CHECKS):
                    s = smp.draw()
                    if sample_good(cx[s[0]], cx[s[1]], cx[s[2]]):
                        break
                else:
                    samples.append(None)
                    counts.append(None)
                    break
                samples.append(s)
                counts.append(int(within(plane_of(cx[s[0]], cx[s[1]], cx[s[2]]), cx, threshold).sum()))
                it, _ = ransac_stop(counts, n, max_iterations, probability)
                if it < len(counts):  # the loop stopped before the last scored hypothesis
                    break
        it, best = ransac_stop(counts, n, max_iterations, probability) if n >= 3 else (0, -1)
        r.update(samples=samples[:it], counts=counts[:it], iterations=it, best=best)
        if best >= 0:
            s = samples[best]
            c0 = plane_of(cx[s[0]], cx[s[1]], cx[s[2]])
            inl0 = np.flatnonzero(within(c0, cx, threshold))
            c1 = refit(cx[inl0], c0) if optimize else c0
            fin = within(c1, cx, threshold)
            r.update(found=True, ransac_coefficients=c0, coefficients=c1, ransac_inliers=valid[inl0],
                     inliers=valid[np.flatnonzero(fin)], sample=s, dist_final=distances(c1, cx))
    keep = ~fin & in_box(cx, box_enable, box_lo, box_hi)
    surv = np.flatnonzero(keep)
    cl = clusters(cx[surv], tol, min_size, max_size)
    r["survivors"] = valid[surv]
    r["clusters"] = [valid[surv[c]] for c in cl]
    r["xyz"] = xyz
    return r
