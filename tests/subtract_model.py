"""NumPy model of scene subtraction (include/pft_subtract.h): all pairs, in float32 with every
product and sum rounded on its own, in the order of the specification.

    slots    {slot number: (model xyz float32[M, 3], T float32[3, 4])}
    xform    per row ((T0 x + T1 y) + T2 z) + T3
    d2       (dx dx + dy dy) + dz dz
    explained iff (double)d2 < (double)r * (double)r for some moved point of some slot (strict)
    owner    the slot of the smallest such d2, ties between slots to the lowest slot number; -1
    d2[i]    that smallest d2; +inf
    support  points per owner (64 slots)
    residual the unexplained records in input order, residual_idx their indices
"""
import numpy as np

F = np.float32
MAX_OBJECTS = 64


def xyz_of(cloud):
    return np.stack([cloud["x"], cloud["y"], cloud["z"]], 1).astype(F)


def xform(T, pts):
    T = np.asarray(T, F).reshape(3, 4)
    pts = np.asarray(pts, F).reshape(-1, 3)
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    out = np.empty((len(pts), 3), F)
    with np.errstate(over="ignore", invalid="ignore"):
        for r in range(3):
            a = (T[r, 0] * x).astype(F)
            b = (T[r, 1] * y).astype(F)
            c = (T[r, 2] * z).astype(F)
            out[:, r] = (((a + b).astype(F) + c).astype(F) + T[r, 3]).astype(F)
    return out


def sq_dist(x, q):
    """d2 of every pair: x float32[n, 3], q float32[m, 3] -> float32[n, m]"""
    with np.errstate(over="ignore", invalid="ignore"):
        dx = (x[:, None, 0] - q[None, :, 0]).astype(F)
        dy = (x[:, None, 1] - q[None, :, 1]).astype(F)
        dz = (x[:, None, 2] - q[None, :, 2]).astype(F)
        return (((dx * dx).astype(F) + (dy * dy).astype(F)).astype(F) + (dz * dz).astype(F)).astype(F)


def subtract(frame_xyz, slots, radius, chunk=2048):
    """-> dict(owner int32[n], d2 float32[n], support uint32[64], residual_idx int32[], n_in, n_explained, n_residual,
    ties: frame points whose smallest d2 is attained by more than one slot)"""
    x = np.asarray(frame_xyz, F).reshape(-1, 3)
    n = len(x)
    r2 = float(F(radius)) * float(F(radius))
    owner = np.full(n, -1, np.int32)
    best = np.full(n, np.inf, F)
    ties = np.zeros(n, bool)
    finite_x = np.isfinite(x).all(axis=1)
    for s in sorted(slots):
        model, T = slots[s]
        q = xform(T, model)
        q = q[np.isfinite(q).all(axis=1)]  # a non-finite moved point explains nothing
        if len(q) == 0:
            continue
        for i0 in range(0, n, chunk):
            sl = slice(i0, min(n, i0 + chunk))
            d = sq_dist(x[sl], q)
            ok = d.astype(np.float64) < r2
            d = np.where(ok, d, F(np.inf))
            m = d.min(axis=1)
            m = np.where(finite_x[sl], m, F(np.inf))  # a non-finite frame point is never explained
            ties[sl] |= (m == best[sl]) & np.isfinite(m)
            better = m < best[sl]  # strict: a tie stays with the lower slot
            ties[sl] &= ~better
            owner[sl] = np.where(better, s, owner[sl])
            best[sl] = np.where(better, m, best[sl])
    support = np.zeros(MAX_OBJECTS, np.uint32)
    for s in slots:
        support[s] = int((owner == s).sum())
    residual_idx = np.flatnonzero(owner < 0).astype(np.int32)
    return dict(owner=owner, d2=best, support=support, residual_idx=residual_idx, n_in=n,
                n_explained=int(n - len(residual_idx)), n_residual=int(len(residual_idx)), ties=ties)
