"""NumPy restatement of ParticleFilterTracker's change detector (PCL 1.8.0 testChangeDetection over
OctreePointCloudChangeDetector) and of the counter schedule of weight(), for the tests.

The box and key arithmetic is the unmodified oracle's: the detector octree's bounding box is never reset, so after testing
crops C1 .. Ck it is the box of oracle.Octree(C1 + .. + Ck), and the final-frame keys of the points of C(k-1) and Ck are
rows of that tree's point_keys().  The new points are those of voxels of Ck that hold no point of C(k-1) and at least
min_points points of Ck (a leaf holds at least one point, so min_points 0 and 1 agree)."""
import numpy as np


class ChangeDetectorModel:
    def __init__(self, oracle, resolution=0.01):
        self.orc = oracle
        self.res = resolution
        self.clouds = []  # every crop tested so far (the box grows over all of them, in order)
        self.prev_len = 0  # points of the previous tested crop (the last entry of self.clouds before this test)

    def test(self, cloud, min_points):
        """one testChangeDetection: returns (new point indices ascending, new voxels, box (min xyz, max xyz), depth)"""
        cloud = np.ascontiguousarray(cloud, self.orc.POINT_DTYPE)
        prev_len = len(self.clouds[-1]) if self.clouds else 0
        self.clouds.append(cloud)
        allpts = np.concatenate(self.clouds) if self.clouds else cloud
        if len(allpts) == 0:
            return np.zeros(0, np.int64), 0, np.zeros(6), 0
        tree = self.orc.Octree(allpts, self.res)
        info = tree.info()
        box = np.concatenate([info["min"], info["max"]])
        n = len(cloud)
        if n == 0:
            return np.zeros(0, np.int64), 0, box, info["depth"]
        # only the last two crops' keys are needed: a tree over everything, keys read for the tail
        keys = _keys_tail(tree, len(allpts) - n - prev_len, len(allpts))
        prev_keys = keys[:prev_len]
        cur_keys = keys[prev_len:]
        prev_set = set(map(tuple, prev_keys.tolist()))
        uniq, inv, counts = np.unique(cur_keys, axis=0, return_inverse=True, return_counts=True)
        inv = inv.reshape(-1)
        minp = max(int(min_points), 1)
        new_vox = np.array([tuple(u) not in prev_set and c >= minp for u, c in zip(uniq.tolist(), counts)], bool)
        idx = np.nonzero(new_vox[inv])[0]
        return idx, int(new_vox.sum()), box, info["depth"]


def _keys_tail(tree, start, stop):
    import ctypes as C

    from oracle import lib as orc_lib

    out = np.zeros((stop - start, 3), np.uint32)
    tmp = np.zeros(3, np.uint32)
    L = orc_lib()
    for i in range(start, stop):
        L.orc_octree_point_key(tree.h, i, C.c_void_p(tmp.ctypes.data))
        out[i - start] = tmp
    return out


class CounterModel:
    """weight()'s bookkeeping: change_counter_ and changed_ (PCL constructor defaults 0 and false)"""

    def __init__(self, counter=0, changed=False):
        self.counter = counter
        self.changed = changed

    def step(self, use, interval, test):
        """one iteration; test() runs the detector and returns whether it found a change.  Returns (tested, changed_,
        counter after)"""
        tested = False
        if self.counter == 0:
            if not use:
                self.changed, self.counter = True, interval
            else:
                tested = True
                if test():
                    self.changed, self.counter = True, interval
                else:
                    self.changed = False
        else:
            self.counter -= 1
        return tested, self.changed, self.counter
