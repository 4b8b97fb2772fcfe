"""NumPy restatement of pft_view_select (include/pft_view.h): float32 arithmetic op by op, the
ranks and the decimation in Python integers.  Every output of the device is compared with this bit for bit."""
import numpy as np

from visibility_model import depth_image, project, xform

KEPT, DECIMATED, SELF_OCCLUDED, OUT_OF_VIEW, NONFINITE = range(5)
F = np.float32


def select(cam, model_xyz, T, max_points=0, rule1=True, q_finite=True):
    """every output of one evaluated select over the float32 points (N, 3).  rule1=False leaves the non-finite rule out,
    q_finite=False the finiteness clause of rule 2 (the host test shows what each is needed for)"""
    p = np.asarray(model_xyz, F).reshape(-1, 3)
    N = len(p)
    T = np.asarray(T, F).reshape(-1)[:12].reshape(3, 4)
    state = np.full(N, OUT_OF_VIEW, np.uint8)
    gap = np.zeros(N, F)
    finite = np.isfinite(p).all(1) if rule1 else np.ones(N, bool)
    state[~finite] = NONFINITE
    q = xform(T, p)
    ok, u, v = project(cam, q)
    ok &= finite
    if q_finite:
        ok &= np.isfinite(q).all(1)
    Zm = depth_image(cam, q[ok])  # (the points that passed rules 1 and 2 all project in view: none is dropped here)
    with np.errstate(all="ignore"):
        gap[ok] = np.fmax(q[ok, 2] - Zm[v[ok], u[ok]], F(0))  # fmaxf: a NaN (inf - inf) gives 0
    assert gap.dtype == F
    occluded = ok & (gap > F(cam["self_margin"]))
    state[occluded] = SELF_OCCLUDED
    visible = np.flatnonzero(ok & ~occluded)
    n_visible, K = len(visible), int(max_points)
    if K == 0 or n_visible <= K:
        keep = np.ones(n_visible, bool)
    else:
        keep = np.array([((r + 1) * K) // n_visible > (r * K) // n_visible for r in range(n_visible)], bool)
    state[visible] = np.where(keep, KEPT, DECIMATED)
    kept_index = visible[keep].astype(np.uint32)
    return dict(transform=T, state=state, self_gap=gap, kept_index=kept_index, n_model=N, n_visible=n_visible,
                n_kept=len(kept_index), n_state=tuple(int((state == s).sum()) for s in range(5)))
