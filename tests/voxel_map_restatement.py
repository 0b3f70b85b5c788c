"""NumPy restatement (int64 / float64) of the voxel map (include/rdmnet_hip.h, "voxel map"), written from the
definition and sharing no code with the library.

A map has a voxel size, C channels (xyz and C - 3 attributes) and F = 20 fractional bits.  Per point p (fp32 row) of a scan with pose
X (float64 4 x 4, world = X p), in float64 with the stated association:
  gate       r2 = (x x + y y) + z z; a row with a non-finite value among its C counts as skipped_nonfinite, else one without
             min_range^2 <= r2 <= max_range^2 as skipped_range;
  transform  w_d = ((X[d][0] x + X[d][1] y) + X[d][2] z) + X[d][3];
  quantise   Q_d = (int64) floor(w_d / voxel 2^F), cell_d = Q_d >> F; A_k = rint(v_k 2^F) (ties to even); a cell outside [-2^20, 2^20)
             or |v_k| >= 2^20 counts as out_of_extent;
  add        per voxel (key = the three cells + 2^20 at 21 bits each) a count and C int64 sums of Q_d / A_k.
Extraction: the voxels with count >= min_points in ascending key order, row = (float32)(sum / count / 2^F voxel) for xyz and the same
without voxel for the attributes, with counts int32 and cells int32 [M, 3].

`Map` holds the voxels as arrays sorted by key, merged with np.unique and np.add.at; it never fills up.  Which keys a FULL table
stores depends on the schedule, but what it stores for a key does not: `Map.subset` gives those rows."""
import numpy as np

F = 20
SCALE = 1048576.0
HALF = 1 << 20
STATS = ('occupied', 'integrated', 'skipped_nonfinite', 'skipped_range', 'out_of_extent', 'dropped_full')


def quantise(points, pose, voxel, channels, min_range=0.0, max_range=np.inf):
    """One scan -> (keys uint64 [K], values int64 [K, C], dict of the three skip counters) for its K kept points, in row order."""
    p32 = np.asarray(points, np.float32)[:, :channels]
    X = np.asarray(pose, np.float64)
    assert p32.ndim == 2 and p32.shape[1] == channels and X.shape == (4, 4)
    p = p32.astype(np.float64)
    finite = np.isfinite(p).all(1)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(invalid='ignore', over='ignore'):
        r2 = (x * x + y * y) + z * z
        in_range = (np.float64(min_range) * np.float64(min_range) <= r2) & (r2 <= np.float64(max_range) * np.float64(max_range))
        inside = np.ones(len(p), bool)
        q = np.zeros((len(p), channels), np.int64)
        for d in range(3):
            w = ((X[d, 0] * x + X[d, 1] * y) + X[d, 2] * z) + X[d, 3]
            f = np.floor(w / np.float64(voxel) * SCALE)
            ok = (f >= -2.0 ** 40) & (f < 2.0 ** 40)  # (NaN and infinities fail)
            inside &= ok
            q[:, d] = np.where(ok, f, 0.0).astype(np.int64)
        for k in range(3, channels):
            ok = np.abs(p[:, k]) < SCALE
            inside &= ok
            q[:, k] = np.rint(np.where(ok, p[:, k], 0.0) * SCALE).astype(np.int64)
    kept = finite & in_range & inside
    cells = q[:, :3] >> F  # arithmetic: floor
    key = (((cells[:, 0] + HALF).astype(np.uint64) << np.uint64(42)) | ((cells[:, 1] + HALF).astype(np.uint64) << np.uint64(21))
           | (cells[:, 2] + HALF).astype(np.uint64))
    skipped = dict(skipped_nonfinite=int((~finite).sum()), skipped_range=int((finite & ~in_range).sum()),
                   out_of_extent=int((finite & in_range & ~inside).sum()))
    return key[kept], q[kept], skipped


class Map:
    def __init__(self, voxel, channels=4):
        assert voxel > 0 and 3 <= channels <= 8
        self.voxel, self.channels = float(voxel), int(channels)
        self.keys = np.zeros(0, np.uint64)
        self.counts = np.zeros(0, np.int64)
        self.sums = np.zeros((0, channels), np.int64)
        self.skipped = dict(skipped_nonfinite=0, skipped_range=0, out_of_extent=0)

    def integrate(self, clouds, poses, min_range=0.0, max_range=np.inf):
        assert len(clouds) == len(poses)
        ks, vs = [self.keys], [self.sums]
        ns = [self.counts]
        for c, X in zip(clouds, poses):
            k, v, skipped = quantise(c, X, self.voxel, self.channels, min_range, max_range)
            ks.append(k)
            vs.append(v)
            ns.append(np.ones(len(k), np.int64))
            for name, n in skipped.items():
                self.skipped[name] += n
        k, v, n = np.concatenate(ks), np.concatenate(vs), np.concatenate(ns)
        self.keys, inverse = np.unique(k, return_inverse=True)
        self.counts = np.zeros(len(self.keys), np.int64)
        self.sums = np.zeros((len(self.keys), self.channels), np.int64)
        np.add.at(self.counts, inverse, n)
        np.add.at(self.sums, inverse, v)
        return self

    def stats(self):
        """The six counters of a table that never filled up."""
        return dict(occupied=len(self.keys), integrated=int(self.counts.sum()), dropped_full=0, **self.skipped)

    def extract(self, min_points=1):
        """-> (points float32 [M, C], counts int32 [M], cells int32 [M, 3]), ascending key order."""
        take = self.counts >= max(int(min_points), 1)
        keys, n, s = self.keys[take], self.counts[take], self.sums[take]
        mean = s.astype(np.float64) / n.astype(np.float64)[:, None] / SCALE
        mean[:, :3] = mean[:, :3] * self.voxel
        cells = np.stack([((keys >> np.uint64(42)) & np.uint64(0x1fffff)).astype(np.int64) - HALF,
                          ((keys >> np.uint64(21)) & np.uint64(0x1fffff)).astype(np.int64) - HALF,
                          (keys & np.uint64(0x1fffff)).astype(np.int64) - HALF], 1)
        return mean.astype(np.float32), n.astype(np.int32), cells.astype(np.int32)

    def subset(self, cells):
        """The restatement's (points, counts, cells) rows of the given cells int [K, 3] (each must be a voxel of this map), in the
        given order: what a table that dropped some keys must hold for the keys it stored."""
        c = np.asarray(cells, np.int64)
        key = (((c[:, 0] + HALF).astype(np.uint64) << np.uint64(42)) | ((c[:, 1] + HALF).astype(np.uint64) << np.uint64(21))
               | (c[:, 2] + HALF).astype(np.uint64))
        pos = np.searchsorted(self.keys, key)
        assert (pos < len(self.keys)).all() and np.array_equal(self.keys[pos], key), 'a stored key is not a voxel of the points'
        pts, n, cl = self.extract(1)
        return pts[pos], n[pos], cl[pos]


def build(clouds, poses, voxel, channels=4, min_range=0.0, max_range=np.inf):
    return Map(voxel, channels).integrate(clouds, poses, min_range, max_range)
