"""NumPy restatement of pft_visibility (include/pft_visibility.h): all pairs, no pruning, float32
arithmetic op by op.  Every output of the device is compared with this bit for bit."""
import numpy as np

VISIBLE, OCCLUDED, SELF_OCCLUDED, OUT_OF_VIEW = range(4)
F = np.float32

DEFAULT_CAMERA = dict(width=160, height=90, fx=90.0, fy=90.0, cx=79.5, cy=44.5, z_near=0.05, splat=1,
                      occlusion_margin=0.03, self_margin=0.03)
DEFAULT_THRESHOLD = (0.25, 0.0, 1)  # min_visible_ratio, min_ratio, lost_after


def camera(**kw):
    c = dict(DEFAULT_CAMERA)
    c.update(kw)
    return c


def project(cam, xyz):
    """(in_view bool[n], u int[n], v int[n]) of float32 points (n, 3); u, v are meaningful only where in_view"""
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    W, H = int(cam["width"]), int(cam["height"])
    with np.errstate(all="ignore"):
        front = z > F(cam["z_near"])  # NaN fails
        xn, yn = x / z, y / z
        uf = F(cam["fx"]) * xn + F(cam["cx"])
        vf = F(cam["fy"]) * yn + F(cam["cy"])
        in_view = front & (uf >= F(0)) & (uf < F(W)) & (vf >= F(0)) & (vf < F(H))
        u = np.where(in_view, np.floor(uf), F(0)).astype(np.int64)
        v = np.where(in_view, np.floor(vf), F(0)).astype(np.int64)
    assert uf.dtype == F and vf.dtype == F
    return in_view, u, v


def depth_image(cam, xyz):
    """Z[v, u] = the smallest z over the points whose footprint covers the pixel, else +inf"""
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    W, H, s = int(cam["width"]), int(cam["height"]), int(cam["splat"])
    Z = np.full((H, W), np.inf, F)
    ok, u, v = project(cam, xyz)
    for i in np.flatnonzero(ok):
        ua, ub = max(u[i] - s, 0), min(u[i] + s, W - 1)
        va, vb = max(v[i] - s, 0), min(v[i] + s, H - 1)
        Z[va:vb + 1, ua:ub + 1] = np.minimum(Z[va:vb + 1, ua:ub + 1], xyz[i, 2])
    return Z


def xform(T, xyz):
    """((T0 x + T1 y) + T2 z) + T3 per row, float32, unfused"""
    T = np.asarray(T, F).reshape(-1)[:12].reshape(3, 4)
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    with np.errstate(all="ignore"):
        out = np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], 1)
    assert out.dtype == F
    return out


def rule(n_visible, n_visible_matched, M, has_match, threshold, prev_streak):
    """(hidden, below, streak, lost)"""
    min_visible_ratio, min_ratio, lost_after = threshold
    hidden = float(n_visible) < min_visible_ratio * float(M)
    below, streak = False, prev_streak
    if has_match and not hidden:
        below = float(n_visible_matched) < min_ratio * float(n_visible)
        streak = prev_streak + 1 if below else 0
    return hidden, below, streak, streak >= lost_after


def visibility(cam, ref_xyz, T, frame_xyz, match_idx=None, threshold=DEFAULT_THRESHOLD, prev_streak=0):
    """every output of one evaluated pft_visibility call.  ref_xyz in the caller's order; match_idx: input_idx of an
    evaluated pft_match of the same frame (has_match), or None"""
    ref_xyz = np.asarray(ref_xyz, F).reshape(-1, 3)
    frame_xyz = np.asarray(frame_xyz, F).reshape(-1, 3)
    M = len(ref_xyz)
    q = xform(T, ref_xyz)
    Zs, Zm = depth_image(cam, frame_xyz), depth_image(cam, q)
    ok, u, v = project(cam, q)
    state = np.full(M, OUT_OF_VIEW, np.uint8)
    scene_gap, self_gap = np.zeros(M, F), np.zeros(M, F)
    with np.errstate(all="ignore"):
        z = q[ok, 2]
        self_gap[ok] = np.fmax(z - Zm[v[ok], u[ok]], F(0))  # fmaxf: a NaN (inf - inf) gives 0
        scene_gap[ok] = np.fmax(z - Zs[v[ok], u[ok]], F(0))
    s = np.where(self_gap > F(cam["self_margin"]), SELF_OCCLUDED,
                 np.where(scene_gap > F(cam["occlusion_margin"]), OCCLUDED, VISIBLE))
    state[ok] = s[ok]
    has_match = match_idx is not None
    n_visible = int((state == VISIBLE).sum())
    n_vm = int(((state == VISIBLE) & (np.asarray(match_idx) >= 0)).sum()) if has_match else 0
    hidden, below, streak, lost = rule(n_visible, n_vm, M, has_match, threshold, prev_streak)
    return dict(transform=np.asarray(T, F).reshape(-1)[:12].reshape(3, 4), state=state, scene_gap=scene_gap,
                self_gap=self_gap, n_reference=M, n_visible=n_visible, n_occluded=int((state == OCCLUDED).sum()),
                n_self=int((state == SELF_OCCLUDED).sum()), n_out=int((state == OUT_OF_VIEW).sum()),
                n_frame=len(frame_xyz), has_match=has_match, n_visible_matched=n_vm, hidden=hidden, below=below,
                streak=streak, lost=lost)
