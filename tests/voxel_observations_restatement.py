"""NumPy restatement of the voxel observations (include/rdmnet_hip.h, "voxel observations"), written from the
definition on top of tests/voxel_map_restatement.py and sharing no code with the library.

Every integrated scan has an integer id.  A voxel OBSERVES scan s when at least one point of s is integrated into it (the gates, the
transform and the quantisation are voxel_map_restatement.quantise; a skipped point observes nothing).  Per voxel: scans = the number
of distinct ids observed, first = the smallest, last = the largest.  All points of an id come in one `integrate` call, so the (voxel,
id) pairs of two calls are distinct and the three values are a function of the set of (id, point) pairs.

`Observed` holds a voxel_map_restatement.Map and, row-aligned with its sorted keys, the three values as int64."""
import numpy as np

import voxel_map_restatement as VM

MAX_SCANS = 64  # of one call of the library; the restatement takes any number
MAX_ID = 2 ** 31 - 1  # ids lie below this


class Observed:
    def __init__(self, voxel, channels=4):
        self.map = VM.Map(voxel, channels)
        self.scans = np.zeros(0, np.int64)
        self.first = np.zeros(0, np.int64)
        self.last = np.zeros(0, np.int64)
        self.num_scans = 0

    def integrate(self, clouds, poses, min_range=0.0, max_range=np.inf, first_id=None):
        """Scan s of `clouds` has the id first_id + s (first_id None: numbered on from the scans integrated so far)."""
        first_id = self.num_scans if first_id is None else int(first_id)
        assert len(clouds) == len(poses) and 0 <= first_id and first_id + len(clouds) <= MAX_ID
        old = self.map.keys
        keys, ids = [], []
        for s, (c, X) in enumerate(zip(clouds, poses)):
            k = np.unique(VM.quantise(c, X, self.map.voxel, self.map.channels, min_range, max_range)[0])  # the voxels that see scan s
            keys.append(k)
            ids.append(np.full(len(k), first_id + s, np.int64))
        self.map.integrate(clouds, poses, min_range, max_range)
        new = self.map.keys
        scans, first, last = np.zeros(len(new), np.int64), np.full(len(new), MAX_ID, np.int64), np.full(len(new), -1, np.int64)
        at = np.searchsorted(new, old)
        scans[at], first[at], last[at] = self.scans, self.first, self.last
        keys, ids = np.concatenate(keys + [np.zeros(0, np.uint64)]), np.concatenate(ids + [np.zeros(0, np.int64)])
        at = np.searchsorted(new, keys)
        np.add.at(scans, at, 1)
        np.minimum.at(first, at, ids)
        np.maximum.at(last, at, ids)
        self.scans, self.first, self.last = scans, first, last
        self.num_scans = max(self.num_scans, first_id + len(clouds))
        return self

    def extract(self, min_points=1):
        """-> (scans, first, last) int32 [M], row-aligned with self.map.extract(min_points)."""
        take = self.map.counts >= max(int(min_points), 1)
        return tuple(v[take].astype(np.int32) for v in (self.scans, self.first, self.last))

    def keep(self, min_scans, min_points=1):
        """The voxels of the pruned map as a mask over the rows of extract(1): count >= min_points and scans >= min_scans."""
        return (self.map.counts >= int(min_points)) & (self.scans >= int(min_scans))

    def pruned(self, min_scans, min_points=1):
        """-> a new Observed that holds only the voxels of `keep`; the three skip counters are carried over."""
        take = self.keep(min_scans, min_points)
        out = Observed(self.map.voxel, self.map.channels)
        out.map.keys, out.map.counts, out.map.sums = self.map.keys[take], self.map.counts[take], self.map.sums[take]
        out.map.skipped = dict(self.map.skipped)
        out.scans, out.first, out.last, out.num_scans = self.scans[take], self.first[take], self.last[take], self.num_scans
        return out


def build(clouds, poses, voxel, channels=4, min_range=0.0, max_range=np.inf):
    return Observed(voxel, channels).integrate(clouds, poses, min_range, max_range)
