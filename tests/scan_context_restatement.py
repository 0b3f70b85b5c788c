"""Float64 numpy restatement of the Scan Context descriptor, distance and search (include/rdmnet_hip.h, "scan context"; DESIGN.md
section 7), written from the definitions and sharing no code with the library.

Descriptor of a cloud [N, >=3]: r = sqrt(x^2 + y^2); a point is skipped if x, y or z is not finite, r == 0 or r > max_range; ring =
min(floor(r / max_range n_rings), n_rings - 1); theta = atan2(y, x) (+ 2 pi if negative); sector = min(floor(theta / (2 pi)
n_sectors), n_sectors - 1); the point's value is the FLOAT32 sum z + lidar_height (so that bins compare bit for bit); a bin holds the
maximum value of its points, 0 without one.

`descriptor_interval` also brackets every bin for an implementation whose atan2 / radius round differently: `lo` is the value from
the points that are certainly in the bin (>= ANGLE_TOL rad from a sector edge, >= RADIUS_TOL max(r, 1) m from a ring edge, >=
RADIUS_TOL max_range inside the range limit), `hi` the value when every point that is possibly in the bin (its own bin and the
neighbours across a near edge, the first and last sector being neighbours) counts.  A bin without a certain point may also be
empty, so 0 is inside its interval.

Distance of descriptors Q, C: columns of 2-norm 0 are invalid; for shift n query column j meets candidate column (j - n) mod
n_sectors; d_n = 1 - mean of the cosines of the column pairs valid on both sides (1 without one); d = min_n d_n at the lowest n.
Search: candidate j is eligible for query i iff (q_base + i) - (c_base + j) >= exclude_recent (negative: always); the best is the
eligible candidate of lowest d, the lowest index among equals; none: (-1, -1, +inf)."""
import numpy as np

ANGLE_TOL = 1e-5
RADIUS_TOL = 1e-5
DEFAULTS = dict(n_rings=20, n_sectors=60, max_range=80.0, lidar_height=2.0)


def point_values(points, lidar_height=2.0):
    return points[:, 2].astype(np.float32) + np.float32(lidar_height)


def point_bins(points, n_rings=20, n_sectors=60, max_range=80.0):
    """-> (keep bool [N], ring int [N], sector int [N], r float64 [N], theta float64 [N]); ring / sector are 0 where not kept."""
    p = np.asarray(points)[:, :3].astype(np.float64)
    x, y = p[:, 0], p[:, 1]
    with np.errstate(invalid='ignore', over='ignore'):
        r = np.sqrt(x * x + y * y)
        keep = np.isfinite(p).all(1) & (r != 0.0) & ~(r > max_range)
        theta = np.arctan2(y, x)
        theta = np.where(theta < 0.0, theta + 2.0 * np.pi, theta)
        ring = np.where(keep, np.minimum(np.floor(np.where(keep, r, 0.0) / max_range * n_rings), n_rings - 1), 0).astype(np.int64)
        sector = np.where(keep, np.minimum(np.floor(np.where(keep, theta, 0.0) / (2.0 * np.pi) * n_sectors), n_sectors - 1),
                          0).astype(np.int64)
    return keep, ring, sector, r, theta


def descriptor(points, n_rings=20, n_sectors=60, max_range=80.0, lidar_height=2.0):
    """-> float32 [n_rings, n_sectors]."""
    points = np.asarray(points, np.float32)
    if points.ndim != 2:
        points = points.reshape(-1, 3)
    keep, ring, sector, _, _ = point_bins(points, n_rings, n_sectors, max_range)
    v = point_values(points, lidar_height)
    best = np.full((n_rings, n_sectors), -np.inf, np.float32)
    np.maximum.at(best, (ring[keep], sector[keep]), v[keep])
    return np.where(np.isinf(best), np.float32(0), best).astype(np.float32)


def descriptor_interval(points, n_rings=20, n_sectors=60, max_range=80.0, lidar_height=2.0):
    """-> (D, lo, hi) float32 [n_rings, n_sectors] each, lo <= D <= hi (see the module text)."""
    points = np.asarray(points, np.float32)
    D = descriptor(points, n_rings, n_sectors, max_range, lidar_height)
    p = points[:, :3].astype(np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        r = np.sqrt(p[:, 0] ** 2 + p[:, 1] ** 2)
    tol_m = RADIUS_TOL * max_range
    maybe = np.isfinite(p).all(1) & (r != 0.0) & (r <= max_range + tol_m)  # possibly kept
    p, r, v = p[maybe], r[maybe], point_values(points, lidar_height)[maybe]
    theta = np.arctan2(p[:, 1], p[:, 0])
    theta = np.where(theta < 0.0, theta + 2.0 * np.pi, theta)
    w, h = 2.0 * np.pi / n_sectors, max_range / n_rings
    ring = np.minimum(np.floor(r / max_range * n_rings), n_rings - 1).astype(np.int64)
    sector = np.minimum(np.floor(theta / (2.0 * np.pi) * n_sectors), n_sectors - 1).astype(np.int64)
    tol_r = RADIUS_TOL * np.maximum(r, 1.0)
    s_dn = theta - sector * w < ANGLE_TOL            # possibly in the sector below (sector 0: the last one)
    s_up = (sector + 1) * w - theta < ANGLE_TOL      # possibly in the sector above (the last one: sector 0)
    r_dn = (ring > 0) & (r - ring * h < tol_r)
    r_up = (ring < n_rings - 1) & ((ring + 1) * h - r < tol_r)
    certain = ~(s_dn | s_up | r_dn | r_up) & (r <= max_range - tol_m)
    sure = np.full((n_rings, n_sectors), -np.inf, np.float32)
    np.maximum.at(sure, (ring[certain], sector[certain]), v[certain])
    top = np.full((n_rings, n_sectors), -np.inf, np.float32)
    low = np.full((n_rings, n_sectors), np.inf, np.float32)  # the lowest value a bin without a certain point can take
    for dr, rm in ((0, np.ones_like(r_dn)), (-1, r_dn), (1, r_up)):
        for dsec, sm in ((0, np.ones_like(s_dn)), (-1, s_dn), (1, s_up)):
            m = rm & sm
            rr, ss = ring[m] + dr, (sector[m] + dsec) % n_sectors
            np.maximum.at(top, (rr, ss), v[m])
            np.minimum.at(low, (rr, ss), v[m])
    has_sure, has_any = ~np.isinf(sure), ~np.isinf(top)
    zero = np.float32(0)
    hi = np.where(has_sure, top, np.where(has_any, np.maximum(top, zero), zero))
    lo = np.where(has_sure, sure, np.where(has_any, np.minimum(low, zero), zero))
    return D, lo.astype(np.float32), hi.astype(np.float32)


def normalise(D):
    """-> (column-normalised float64 [R, S] with 0 in invalid columns, valid bool [S])."""
    D = np.asarray(D, np.float64)
    norms = np.sqrt((D * D).sum(0))
    valid = norms > 0.0
    return np.where(valid, D / np.where(valid, norms, 1.0), 0.0), valid


def shift_distances(Q, C):
    """d_n for every shift n -> float64 [n_sectors]."""
    Qn, vq = normalise(Q)
    Cn, vc = normalise(C)
    S = Qn.shape[1]
    idx = (np.arange(S)[None, :] - np.arange(S)[:, None]) % S  # idx[n, j] = (j - n) mod S
    cos = np.einsum('rj,rnj->nj', Qn, Cn[:, idx])             # cosine of query column j with candidate column idx[n, j]
    both = vq[None, :] & vc[idx]
    cnt = both.sum(1)
    total = np.where(both, cos, 0.0).sum(1)
    return np.where(cnt > 0, 1.0 - total / np.maximum(cnt, 1), 1.0)


def distance(Q, C):
    """-> (d, shift, margin): margin = the second-lowest d_n minus the lowest (+inf with one sector)."""
    d = shift_distances(Q, C)
    n = int(np.argmin(d))  # (the first of equals)
    rest = np.delete(d, n)
    return float(d[n]), n, float(rest.min() - d[n]) if rest.size else float('inf')


def distance_matrix(Qs, Cs):
    """-> (d float64 [n_q, n_c], shift int64 [n_q, n_c], margin float64 [n_q, n_c])."""
    nq, nc = len(Qs), len(Cs)
    d, s, m = np.zeros((nq, nc)), np.zeros((nq, nc), np.int64), np.zeros((nq, nc))
    for i in range(nq):
        for j in range(nc):
            d[i, j], s[i, j], m[i, j] = distance(Qs[i], Cs[j])
    return d, s, m


def eligible(n_q, n_c, q_base=0, c_base=0, exclude_recent=50):
    if exclude_recent < 0:
        return np.ones((n_q, n_c), bool)
    return (q_base + np.arange(n_q))[:, None] - (c_base + np.arange(n_c))[None, :] >= exclude_recent


def search(d, q_base=0, c_base=0, exclude_recent=50):
    """d [n_q, n_c] -> (index int64 [n_q] (-1: none), distance [n_q] (+inf), gap [n_q]: the second-lowest eligible distance minus the
    lowest, +inf with fewer than two)."""
    d = np.asarray(d)
    ok = eligible(d.shape[0], d.shape[1], q_base, c_base, exclude_recent)
    index = np.full(d.shape[0], -1, np.int64)
    best = np.full(d.shape[0], np.inf, d.dtype)
    gap = np.full(d.shape[0], np.inf)
    for i in range(d.shape[0]):
        cols = np.nonzero(ok[i])[0]
        if cols.size:
            k = int(np.argmin(d[i, cols]))  # (the first of equals = the lowest candidate)
            index[i], best[i] = cols[k], d[i, cols[k]]
            if cols.size > 1:
                gap[i] = float(np.delete(d[i, cols], k).min()) - float(best[i])
    return index, best, gap


def rotate_z(points, degrees):
    """The cloud rotated by +degrees about z (float64 arithmetic, float32 result); further columns are kept."""
    a = np.deg2rad(degrees)
    R = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    out = np.array(points, np.float32)
    out[:, :3] = (np.asarray(points)[:, :3].astype(np.float64) @ R.T).astype(np.float32)
    return out


def random_descriptors(n, seed, n_rings=20, n_sectors=60):
    """Seeded descriptors: about half the bins empty, heights in [-0.7, 3), one column in ten without any point."""
    rng = np.random.default_rng(seed)
    D = rng.uniform(-0.7, 3.0, (n, n_rings, n_sectors))
    keep = (rng.random((n, n_rings, n_sectors)) < 0.5) & (rng.random((n, 1, n_sectors)) >= 0.1)
    return np.where(keep, D, 0.0).astype(np.float32)


RANDOM_FIXTURE = dict(n_q=37, n_c=53, q_seed=20181, c_seed=20182)  # neither count is a multiple of a tile


def random_fixture():
    f = RANDOM_FIXTURE
    return random_descriptors(f['n_q'], f['q_seed']), random_descriptors(f['n_c'], f['c_seed'])
