"""NumPy restatement of the object report (include/pft.h pft_report): what
auto_tracking.cpp's drawResult and viz_cb compute from a result pose, recalled from PCL 1.8.0 and Eigen 3.3, float32
with explicit operation order.  csrc/pft_report.hip follows it step for step (report_solve mirrors `solve` line for
line).  The per-point passes are elementwise float32 array operations (each one rounded, nothing contracted); the sums
are written out: `tree_sum` (pairs of neighbours, padded with -0.0 to a power of two) or `chain_sum` (index order).
Test infrastructure: the tests compare the device against it; PCL and Eigen are not available, so parity stays
unpinned."""
import numpy as np

F = np.float32
FLT_MIN = F(np.finfo(np.float32).tiny)
FLT_EPS = F(np.finfo(np.float32).eps)
MAX_ITERATIONS = 30  # SelfAdjointEigenSolver::m_maxIterations
SUM_TREE, SUM_PCL = 0, 1


# ---- sums ----
def tree_sum(v):
    """adjacent-pair tree: T0 = v padded with -0.0 (the exact additive identity, so the padding length does not change a
    bit) to a power of two, T(k+1)[i] = Tk[2i] + Tk[2i+1], result = the root"""
    a = np.ascontiguousarray(v, F)
    if a.size == 0:
        return F(0)
    p = 1
    while p < a.size:
        p *= 2
    a = np.concatenate([a, np.full(p - a.size, F(-0.0), F)])
    while a.size > 1:
        a = a[0::2] + a[1::2]
    return F(a[0])


def chain_sum(v):
    """index order from +0.0, as PCL's loops add"""
    s = F(0)
    for x in np.asarray(v, F):
        s = F(s + x)
    return s


def _sum(v, order):
    return chain_sum(v) if order == SUM_PCL else tree_sum(v)


def min_last(v):
    """getMinMax3D's `min_p = min_p.min(pt)` (SSE minps: the new value unless the running one is smaller): the value of the
    LAST point equal to the minimum -- the sign of a zero bound follows the later point"""
    return F(v[np.flatnonzero(v == v.min())[-1]])


def max_last(v):
    return F(v[np.flatnonzero(v == v.max())[-1]])


# ---- step 1: the transform ----
def transform(x, y, z, T):
    """pcl::transformPointCloud: ((T0 x + T1 y) + T2 z) + T3 per row, float, unfused; T row-major 3x4 (or 4x4)"""
    T = np.asarray(T, F).reshape(-1)
    return (((T[0] * x + T[1] * y) + T[2] * z) + T[3],
            ((T[4] * x + T[5] * y) + T[6] * z) + T[7],
            ((T[8] * x + T[9] * y) + T[10] * z) + T[11])


def report_transform(pose_matrix):
    """drawResult: toEigenMatrix(result), translation += (0, 0, -0.005f)"""
    T = np.array(pose_matrix, F).reshape(4, 4).copy()
    T[2, 3] = F(T[2, 3] + F(-0.005))
    return T


# ---- step 5: SelfAdjointEigenSolver<Matrix3f>::compute (Eigen 3.3) ----
def _hypot(x, y):
    """numext::hypot (positive_real_hypot)"""
    ax, ay = F(abs(x)), F(abs(y))
    p, o = (ax, ay) if ax > ay else (ay, ax)
    if p == F(0):
        return F(0)
    qp = F(o / p)
    return F(p * F(np.sqrt(F(F(1) + F(qp * qp)))))


def _make_givens(p, q):
    """JacobiRotation::makeGivens(p, q) for a real scalar: (c, s)"""
    if q == F(0):
        return (F(-1) if p < F(0) else F(1)), F(0)
    if p == F(0):
        return F(0), (F(1) if q < F(0) else F(-1))
    if abs(p) > abs(q):
        t = F(q / p)
        u = F(np.sqrt(F(F(1) + F(t * t))))
        if p < F(0):
            u = F(-u)
        c = F(F(1) / u)
        s = F(F(-t) * c)
        return c, s
    t = F(p / q)
    u = F(np.sqrt(F(F(1) + F(t * t))))
    if q < F(0):
        u = F(-u)
    s = F(F(-1) / u)
    c = F(F(-t) * s)
    return c, s


def _qr_step(diag, sub, start, end, Q):
    """tridiagonal_qr_step with the Wilkinson shift; Q (3x3, [row][col]) = Q * G (applyOnTheRight(k, k+1, rot))"""
    td = F(F(diag[end - 1] - diag[end]) * F(0.5))
    e = sub[end - 1]
    mu = diag[end]
    if td == F(0):
        mu = F(mu - F(abs(e)))
    else:
        e2 = F(e * e)
        h = _hypot(td, e)
        if e2 == F(0):
            mu = F(mu - F(F(e / F(td + (F(1) if td > F(0) else F(-1)))) * F(e / h)))
        else:
            mu = F(mu - F(e2 / F(td + (h if td > F(0) else F(-h)))))
    x = F(diag[start] - mu)
    z = sub[start]
    for k in range(start, end):
        c, s = _make_givens(x, z)
        sdk = F(F(s * diag[k]) + F(c * sub[k]))
        dkp1 = F(F(s * sub[k]) + F(c * diag[k + 1]))
        diag[k] = F(F(c * F(F(c * diag[k]) - F(s * sub[k]))) - F(s * F(F(c * sub[k]) - F(s * diag[k + 1]))))
        diag[k + 1] = F(F(s * sdk) + F(c * dkp1))
        sub[k] = F(F(c * sdk) - F(s * dkp1))
        if k > start:
            sub[k - 1] = F(F(c * sub[k - 1]) - F(s * z))
        x = sub[k]
        if k < end - 1:
            z = F(F(-s) * sub[k + 1])
            sub[k + 1] = F(c * sub[k + 1])
        # apply_rotation_in_the_plane(col k, col k+1, rot.transpose()): x' = c x + (-s) y, y' = -(-s) x + c y
        ms = F(-s)
        for i in range(3):
            xi, yi = Q[i][k], Q[i][k + 1]
            Q[i][k] = F(F(c * xi) + F(ms * yi))
            Q[i][k + 1] = F(F(F(-ms) * xi) + F(c * yi))


def solve(cov, centroid):
    """viz_cb after the covariance, for the 3x3 `cov` ([row][col], symmetric) and the centroid (3): returns
    (eigenvalues ascending, axes [row][col] with col 2 = col 0 x col 1, info) -- one lane's scalar code, mirrored line for
    line by report_solve in csrc/pft_report.hip"""
    # scale: the largest |coefficient| of the lower triangle (1 if 0); lower triangle / scale
    m = [[F(0)] * 3 for _ in range(3)]
    for r in range(3):
        for c in range(r + 1):
            m[r][c] = F(cov[r][c])
    scale = F(0)
    for r in range(3):
        for c in range(r + 1):
            a = F(abs(m[r][c]))
            if a > scale:
                scale = a
    if scale == F(0):
        scale = F(1)
    for r in range(3):
        for c in range(r + 1):
            m[r][c] = F(m[r][c] / scale)
    # tridiagonalization_inplace, 3x3 closed form (extractQ)
    diag = [F(0)] * 3
    sub = [F(0)] * 2
    diag[0] = m[0][0]
    v1norm2 = F(m[2][0] * m[2][0])
    if v1norm2 <= FLT_MIN:
        diag[1] = m[1][1]
        diag[2] = m[2][2]
        sub[0] = m[1][0]
        sub[1] = m[2][1]
        Q = [[F(1), F(0), F(0)], [F(0), F(1), F(0)], [F(0), F(0), F(1)]]
    else:
        beta = F(np.sqrt(F(F(m[1][0] * m[1][0]) + v1norm2)))
        inv_beta = F(F(1) / beta)
        m01 = F(m[1][0] * inv_beta)
        m02 = F(m[2][0] * inv_beta)
        q = F(F(F(F(2) * m01) * m[2][1]) + F(m02 * F(m[2][2] - m[1][1])))
        diag[1] = F(m[1][1] + F(m02 * q))
        diag[2] = F(m[2][2] - F(m02 * q))
        sub[0] = beta
        sub[1] = F(m[2][1] - F(m01 * q))
        Q = [[F(1), F(0), F(0)], [F(0), m01, m02], [F(0), m02, F(-m01)]]
    # computeFromTridiagonal_impl
    n = 3
    end, start, it = n - 1, 0, 0
    precision = F(F(2) * FLT_EPS)
    while end > 0:
        for i in range(start, end):
            if F(abs(sub[i])) <= F(F(F(abs(diag[i])) + F(abs(diag[i + 1]))) * precision) or F(abs(sub[i])) <= FLT_MIN:
                sub[i] = F(0)
        while end > 0 and sub[end - 1] == F(0):
            end -= 1
        if end <= 0:
            break
        it += 1
        if it > MAX_ITERATIONS * n:
            break
        start = end - 1
        while start > 0 and sub[start - 1] != F(0):
            start -= 1
        _qr_step(diag, sub, start, end, Q)
    info = 0 if it <= MAX_ITERATIONS * n else 1
    if info == 0:  # selection sort, first minimum; the vector columns follow
        for i in range(n - 1):
            k = i
            for j in range(i + 1, n):
                if diag[j] < diag[k]:
                    k = j
            if k > i:
                diag[i], diag[k] = diag[k], diag[i]
                for r in range(3):
                    Q[r][i], Q[r][k] = Q[r][k], Q[r][i]
    evals = [F(d * scale) for d in diag]
    # eigDx.col(2) = eigDx.col(0).cross(eigDx.col(1))
    a = [Q[0][0], Q[1][0], Q[2][0]]
    b = [Q[0][1], Q[1][1], Q[2][1]]
    Q[0][2] = F(F(a[1] * b[2]) - F(a[2] * b[1]))
    Q[1][2] = F(F(a[2] * b[0]) - F(a[0] * b[2]))
    Q[2][2] = F(F(a[0] * b[1]) - F(a[1] * b[0]))
    return evals, Q, info


def p2w_matrix(axes, c):
    """p2w: linear part eigDx^T, translation -(eigDx^T c) with Eigen's a0 + (a1 + a2); row-major 3x4"""
    R = [[axes[j][i] for j in range(3)] for i in range(3)]
    out = np.zeros(12, F)
    for i in range(3):
        out[4 * i:4 * i + 3] = R[i]
        out[4 * i + 3] = F(-F(F(R[i][0] * c[0]) + F(F(R[i][1] * c[1]) + F(R[i][2] * c[2]))))
    return out


def quaternion(m):
    """Quaternion(Matrix3) assignment (Shoemake): (x, y, z, w)"""
    q = [F(0)] * 4  # x, y, z, w
    t = F(m[0][0] + F(m[1][1] + m[2][2]))
    if t > F(0):
        t = F(np.sqrt(F(t + F(1))))
        q[3] = F(F(0.5) * t)
        t = F(F(0.5) / t)
        q[0] = F(F(m[2][1] - m[1][2]) * t)
        q[1] = F(F(m[0][2] - m[2][0]) * t)
        q[2] = F(F(m[1][0] - m[0][1]) * t)
    else:
        i = 0
        if m[1][1] > m[0][0]:
            i = 1
        if m[2][2] > m[i][i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = F(np.sqrt(F(F(F(m[i][i] - m[j][j]) - m[k][k]) + F(1))))
        q[i] = F(F(0.5) * t)
        t = F(F(0.5) / t)
        q[3] = F(F(m[k][j] - m[j][k]) * t)
        q[j] = F(F(m[j][i] + m[i][j]) * t)
        q[k] = F(F(m[k][i] + m[i][k]) * t)
    return q


def report(xyz, T, order=SUM_TREE):
    """the whole report for model points xyz (n x 3) under the 4x4 (or 3x4) transform T as used (offset included).
    Returns (dict of float32 arrays in pft_object_report's fields, tracked xyz n x 3)"""
    xyz = np.ascontiguousarray(xyz, F)
    n = len(xyz)
    Tm = np.asarray(T, F).reshape(-1)
    tx, ty, tz = transform(xyz[:, 0], xyz[:, 1], xyz[:, 2], Tm)
    nf = F(n)
    c = [F(_sum(tx, order) / nf), F(_sum(ty, order) / nf), F(_sum(tz, order) / nf)]
    px, py, pz = tx - c[0], ty - c[1], tz - c[2]
    c11 = _sum(py * py, order)
    c12 = _sum(py * pz, order)
    c22 = _sum(pz * pz, order)
    c00 = _sum(px * px, order)
    c01 = _sum(py * px, order)
    c02 = _sum(pz * px, order)
    cov = [[F(c00 / nf), F(c01 / nf), F(c02 / nf)],
           [F(c01 / nf), F(c11 / nf), F(c12 / nf)],
           [F(c02 / nf), F(c12 / nf), F(c22 / nf)]]
    evals, axes, info = solve(cov, c)
    P = p2w_matrix(axes, c)
    ux, uy, uz = transform(tx, ty, tz, P)
    bmin = [min_last(ux), min_last(uy), min_last(uz)]
    bmax = [max_last(ux), max_last(uy), max_last(uz)]
    mean_diag = [F(F(0.5) * F(bmax[i] + bmin[i])) for i in range(3)]
    centre = [F(F(F(axes[i][0] * mean_diag[0]) + F(F(axes[i][1] * mean_diag[1]) + F(axes[i][2] * mean_diag[2]))) + c[i])
              for i in range(3)]
    T16 = np.zeros(16, F)
    T16[:len(Tm)] = Tm
    T16[12:16] = [0, 0, 0, 1]
    out = {
        "transform": T16,
        "centroid": np.array(c + [F(1)], F),
        "covariance": np.array(cov, F).reshape(9),
        "eigenvalues": np.array(evals, F),
        "axes": np.array(axes, F).reshape(9),
        "box_min": np.array(bmin, F),
        "box_max": np.array(bmax, F),
        "box_centre": np.array(centre, F),
        "box_quat": np.array(quaternion(axes), F),
        "box_size": np.array([F(bmax[i] - bmin[i]) for i in range(3)], F),
        "n_points": n,
        "info": info,
    }
    return out, np.stack([tx, ty, tz], axis=1)
