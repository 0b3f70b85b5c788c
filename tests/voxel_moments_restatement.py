"""NumPy restatement (int64 / float64) of the voxel moments (include/rdmnet_hip.h, "voxel moments"), written
from the definition and sharing no code with the library.  It builds on voxel_map_restatement.quantise: the gates, the transform
and the quantisation are the map's.

For a point the map integrates, with Q_d and cell_d = Q_d >> 20 of the map:
  local      u_d = (Q_d - (cell_d << 20)) >> 8, in [0, 4096): 12 bits, a resolution of voxel / 4096;
  add        nine non-negative integers to the point's voxel: u_x, u_y, u_z, u_x u_x, u_x u_y, u_x u_z, u_y u_y, u_y u_z, u_z u_z.
Per extracted voxel (the map's selection and order), in float64 with this association:
  n = (double)count, m_a = S_a / n, s = voxel / 4096.0, s2 = s s, cov_ab = (S_ab / n - m_a m_b) s2
-- the population covariance, six values (xx, xy, xz, yy, yz, zz), no clamp.  Eigenvalues ascending l0 <= l1 <= l2 (here:
numpy.linalg.eigh); normal = the unit eigenvector of l0, signed so that its component of largest magnitude is positive (on a tie
the lowest axis decides).  The report over the voxels with count >= min_points: plane_thickness = sqrt(mean(max(l0, 0))) in
metres; entropy = the mean of 0.5 ln((2 pi e)^3 l0 l1 l2) over the voxels with l0 > 0; the others are `degenerate`."""
import math

import numpy as np

import voxel_map_restatement as VM

SHIFT = 8
STEPS = 4096.0
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


def local(q):
    """Q int64 [K, >= 3] -> u int64 [K, 3]."""
    q = np.asarray(q, np.int64)[:, :3]
    cell = q >> VM.F
    return (q - (cell << VM.F)) >> SHIFT


def nine(u):
    """u int64 [K, 3] -> the nine addends int64 [K, 9]."""
    return np.concatenate([u, np.stack([u[:, a] * u[:, b] for a, b in PAIRS], 1)], 1)


def covariance(sums, counts, voxel):
    """sums int64 [M, 9], counts [M] -> float64 [M, 6]."""
    n = np.asarray(counts).astype(np.float64)
    S = np.asarray(sums, np.int64).astype(np.float64)
    m = S[:, :3] / n[:, None]
    s = np.float64(voxel) / STEPS
    s2 = s * s
    return np.stack([(S[:, 3 + k] / n - m[:, a] * m[:, b]) * s2 for k, (a, b) in enumerate(PAIRS)], 1)


def full(cov):
    """[M, 6] -> symmetric [M, 3, 3]."""
    c = np.asarray(cov, np.float64)
    return np.stack([c[:, [0, 1, 2]], c[:, [1, 3, 4]], c[:, [2, 4, 5]]], 1)


def signed(normals):
    """The sign rule: the component of largest magnitude positive, the lowest axis on a tie."""
    v = np.array(normals, np.float64, copy=True).reshape(-1, 3)
    big = np.argmax(np.abs(v), axis=1)  # (the first maximum)
    flip = v[np.arange(len(v)), big] < 0
    v[flip] = -v[flip]
    return v


def eigen(cov):
    """-> (eigenvalues [M, 3] ascending, normals [M, 3])."""
    if len(cov) == 0:
        return np.zeros((0, 3)), np.zeros((0, 3))
    w, v = np.linalg.eigh(full(cov))
    return w, signed(v[:, :, 0])


def report(eigenvalues, voxels):
    """eigenvalues [Q, 3] of the voxels with count >= min_points, voxels = the number of all voxels."""
    w = np.asarray(eigenvalues, np.float64).reshape(-1, 3)
    good = w[w[:, 0] > 0]
    k = (2.0 * math.pi * math.e) ** 3
    return dict(voxels=int(voxels), qualified=len(w), degenerate=len(w) - len(good),
                plane_thickness=math.sqrt(float(np.maximum(w[:, 0], 0.0).mean())) if len(w) else float('nan'),
                entropy=float((0.5 * np.log(k * good[:, 0] * good[:, 1] * good[:, 2])).mean()) if len(good) else float('nan'))


class Moments:
    """The map of voxel_map_restatement with the nine sums beside it; it never fills up."""

    def __init__(self, voxel, channels=4):
        self.map = VM.Map(voxel, channels)
        self.voxel = float(voxel)
        self.keys = np.zeros(0, np.uint64)
        self.sums = np.zeros((0, 9), np.int64)

    def integrate(self, clouds, poses, min_range=0.0, max_range=np.inf):
        self.map.integrate(clouds, poses, min_range, max_range)
        ks, vs = [self.keys], [self.sums]
        for c, X in zip(clouds, poses):
            k, q, _ = VM.quantise(c, X, self.voxel, self.map.channels, min_range, max_range)
            ks.append(k)
            vs.append(nine(local(q)))
        k, v = np.concatenate(ks), np.concatenate(vs)
        self.keys, inverse = np.unique(k, return_inverse=True)
        self.sums = np.zeros((len(self.keys), 9), np.int64)
        np.add.at(self.sums, inverse.reshape(-1), v)
        assert np.array_equal(self.keys, self.map.keys)
        return self

    def extract(self, min_points=1):
        """-> (sums int64 [M, 9], cov [M, 6], eigenvalues [M, 3], normals [M, 3]), the rows of Map.extract(min_points)."""
        take = self.map.counts >= max(int(min_points), 1)
        sums, n = self.sums[take], self.map.counts[take]
        cov = covariance(sums, n, self.voxel)
        w, normal = eigen(cov)
        return sums, cov, w, normal

    def subset(self, cells):
        """(sums, cov) of the given cells int [K, 3], in the given order: what a table that dropped some keys must hold."""
        c = np.asarray(cells, np.int64)
        key = (((c[:, 0] + VM.HALF).astype(np.uint64) << np.uint64(42)) | ((c[:, 1] + VM.HALF).astype(np.uint64) << np.uint64(21))
               | (c[:, 2] + VM.HALF).astype(np.uint64))
        pos = np.searchsorted(self.keys, key)
        assert (pos < len(self.keys)).all() and np.array_equal(self.keys[pos], key), 'a stored key is not a voxel of the points'
        return self.sums[pos], covariance(self.sums[pos], self.map.counts[pos], self.voxel)

    def sharpness(self, min_points=4):
        return report(self.extract(min_points)[2], len(self.keys))


def build(clouds, poses, voxel, channels=4, min_range=0.0, max_range=np.inf):
    return Moments(voxel, channels).integrate(clouds, poses, min_range, max_range)
