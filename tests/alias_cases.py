"""Weight shapes for the alias-table tests (test_alias_search_host.py, test_gpu_resample_prefix.py): the shapes at which
the two-level search of the resample kernels (pcl_tracking_amd/csrc/pft_alias.h) changes its path.

With n weights, q_i = w_i * n; m = number of smalls (q < 1), nh = n - m larges.  The kernels stage every s-th element of
the running sums D (over the smalls) and E (over the larges) in LDS, s = ceil(m / 256) resp. ceil(nh / 256): s steps
1 -> 2 -> 3 at m (nh) = 256 -> 257 and 512 -> 513, and the last coarse block is ragged whenever s does not divide m (nh)."""
import numpy as np

F1 = np.float32(1)


def skewed(n, rng):
    """rng.random(n)**6 with 15 % zeros, normalised"""
    w = rng.random(n).astype(np.float32) ** 6
    w[rng.random(n) < 0.15] = 0
    return (w / max(w.sum(), 1e-30)).astype(np.float32)


def uniform(n):
    """1/n: at a power of two every q == 1, m = 0, E all zero"""
    return np.full(n, F1 / np.float32(n), np.float32)


def single_mass(n):
    """all mass on one particle: nh = 1, m = n - 1"""
    w = np.zeros(n, np.float32)
    w[n // 2] = 1.0
    return w


def ties(n):
    """uniform with the first half halved, not renormalised: E all equal"""
    w = uniform(n)
    w[: n // 2] *= np.float32(0.5)
    return w


def with_smalls(n, m, rng):
    """exactly m weights are 0.5 / n (q = 0.5), at seeded positions; the other n - m share the remainder (q > 1)"""
    assert 0 < m < n
    w = np.full(n, np.float32((1.0 - 0.5 * m / n) / (n - m)), np.float32)
    w[rng.permutation(n)[:m]] = np.float32(0.5 / n)
    q = (w * np.float32(n)).astype(np.float64)
    assert int((q < 1.0).sum()) == m
    return w


COUNTS = (1, 255, 256, 257, 512, 513)  # of smalls, and of larges: where s steps and where the last block is ragged


def constructed(n, rng):
    """[(label, w)] with m in COUNTS and with nh in COUNTS"""
    out = [("m=%d" % m, with_smalls(n, m, rng)) for m in COUNTS if m < n]
    out += [("nh=%d" % nh, with_smalls(n, n - nh, rng)) for nh in COUNTS if nh < n]
    return out


def basic(n, rng):
    """[(label, w)]: the four shapes every size is run with"""
    return [("skewed", skewed(n, rng)), ("uniform", uniform(n)), ("single", single_mass(n)), ("ties", ties(n))]
