"""NumPy restatement of the plane rounds (include/pft_segment.h, DESIGN.md section 3.7 "plane rounds"): the loop of the
reference's test/cluster_euclid.cpp:59-85 and test/cluster_extraction.cpp over segment_model's rules, with the refit in
either summation order (PCL's serial float chain, or report_model.tree_sum).  Test infrastructure, like segment_model:
PCL itself is not available, so parity stays unpinned."""
import numpy as np

import segment_model as M

F = np.float32
STOP_FRACTION, STOP_NO_PLANE, STOP_MAX_PLANES = 0, 1, 2


def refit(xyz, coef, order="pcl"):
    """optimizeModelCoefficients; order "tree": the nine sums as adjacent-pair trees in float over the inlier list
    padded with -0.0 to a power of two, the products rounded to float first; everything after the sums is the same"""
    return M.refit(xyz, coef, order)


def segment_once(cx, max_iterations=1000, threshold=0.015, probability=0.99, seed=12345, optimize=True, order="pcl"):
    """one SACSegmentation::segment over the cloud cx (indices 0 .. n - 1): M.pipeline's plane stage"""
    n = len(cx)
    r = {"n_valid": n, "samples": [], "counts": [], "iterations": 0, "best": -1, "found": False}
    samples, counts = [], []
    if n >= 3:
        smp = M.Sampler(n, seed)
        limit = max_iterations + 1
        while len(samples) < limit:
            for _ in range(M.MAX_SAMPLE_CHECKS):
                s = smp.draw()
                if M.sample_good(cx[s[0]], cx[s[1]], cx[s[2]]):
                    break
            else:
                samples.append(None)
                counts.append(None)
                break
            samples.append(s)
            counts.append(int(M.within(M.plane_of(cx[s[0]], cx[s[1]], cx[s[2]]), cx, threshold).sum()))
            it, _ = M.ransac_stop(counts, n, max_iterations, probability)
            if it < len(counts):
                break
    it, best = M.ransac_stop(counts, n, max_iterations, probability) if n >= 3 else (0, -1)
    r.update(samples=samples[:it], counts=counts[:it], iterations=it, best=best)
    if best >= 0:
        s = samples[best]
        c0 = M.plane_of(cx[s[0]], cx[s[1]], cx[s[2]])
        inl0 = np.flatnonzero(M.within(c0, cx, threshold))
        c1 = refit(cx[inl0], c0, order) if optimize else c0
        d = M.distances(c1, cx)
        r.update(found=True, ransac_coefficients=c0, coefficients=c1, ransac_local=inl0,
                 final_local=np.flatnonzero(d < M.float_bound_below(threshold)), sample=s, dist_final=d)
    return r


def another_round(remaining, nr, fraction):
    """RULE rounds: the reference's `cloud_filtered->points.size() > 0.3 * nr_points`, a double product and compare"""
    return float(remaining) > float(fraction) * float(nr)


def pipeline(points, max_planes=16, fraction=0.3, order="pcl", transform_matrix=None, plane=True, max_iterations=100,
             threshold=0.02, probability=0.99, seed=12345, optimize=True, box_enable=(0, 0, 0),
             box_lo=(0.45, -0.6, -0.17), box_hi=(1.1, 0.6, 0.2), tol=0.02, min_size=10, max_size=2500, near_eps=1e-6):
    """-> rounds (each: segment_once's record with `ransac_inliers` / `inliers` as input indices and `near`, the input
    indices within near_eps of the threshold of the round's final plane), n_planes, stopped_by, survivors, clusters"""
    xyz = np.stack([points["x"], points["y"], points["z"]], 1).astype(F)
    if transform_matrix is not None:
        xyz = M.transform(xyz, transform_matrix)
    valid = np.flatnonzero(M.keep_nonzero(xyz))
    nr = len(valid)
    left = valid  # input indices of the remaining cloud, ascending
    rounds, n_planes, stopped_by = [], 0, STOP_FRACTION
    while plane:
        if not another_round(len(left), nr, fraction):
            stopped_by = STOP_FRACTION
            break
        if len(rounds) >= max_planes:
            stopped_by = STOP_MAX_PLANES
            break
        r = segment_once(xyz[left], max_iterations, threshold, probability, seed, optimize, order)
        if r["found"]:
            r["ransac_inliers"] = left[r["ransac_local"]]
            r["inliers"] = left[r["final_local"]]
            r["near"] = left[np.abs(r["dist_final"].astype(np.float64) - threshold) < near_eps]
        else:
            r["near"] = np.zeros(0, np.int64)
        rounds.append(r)
        if not r["found"] or len(r["final_local"]) == 0:  # the reference's break: nothing is removed
            stopped_by = STOP_NO_PLANE
            break
        n_planes += 1
        keep = np.ones(len(left), bool)
        keep[r["final_local"]] = False
        left = left[keep]
    surv = left[M.in_box(xyz[left], box_enable, box_lo, box_hi)]
    cl = M.clusters(xyz[surv], tol, min_size, max_size)
    return {"n_valid": nr, "rounds": rounds, "n_planes": n_planes, "stopped_by": stopped_by, "remaining": len(left),
            "survivors": surv, "clusters": [surv[c] for c in cl], "xyz": xyz}
