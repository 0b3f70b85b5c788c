"""NumPy restatement (float64) of the scan-to-map registration with robust weights (include/rdmnet_hip.h, "voxel map registration
with robust weights"), built on voxel_register_restatement: its gates, visit and per-pair r, M and q
(`evaluate(..., terms=True)`), its `cholesky_solve` and its `apply`; it shares no code with the library.

Per pair, with mu = robust_scale > 0 in units of squared Mahalanobis distance (the Geman-McClure weight of the pose graph's line process):
  d2 = r^T M r, s = mu / (mu + d2), l = s s;
  totals    H = sum l J^T M J, g = sum l J^T M r, cost = sum s d2 (= mu d2 / (mu + d2): its gradient with the associations held
            fixed is 2 g), weight_sum = sum l, n_corr = the number of pairs, whatever their weights.
The iteration is voxel_register_restatement.register's.  robust_scale = None is the plain form: what voxel_register_restatement
returns, unchanged.

Also the scene of the tests: test_voxel_register.street plus a box that stands somewhere else in one scan than in the others."""
import numpy as np

import voxel_register_restatement as RR

BOX = (4.0, 1.8, 1.5)  # a van: length, width and height in metres


def evaluate(table, cloud, X, sigma=0.02, min_points=4, neighbors=1, min_range=0.0, max_range=np.inf, robust_scale=None, terms=False):
    """robust_scale None: voxel_register_restatement.evaluate, unchanged.  Else -> dict(H [6, 6], g [6], cost, weight_sum, n_corr,
    n_points, and `abs_H`, `abs_g`, `abs_cost`, `abs_weight_sum`: the sums of the absolute values of the weighted terms of every
    entry).  terms: also the per-pair `r`, `M`, `q`, `d2` [P] and `l` [P]."""
    if robust_scale is None:
        return RR.evaluate(table, cloud, X, sigma, min_points, neighbors, min_range, max_range, terms=terms)
    mu = np.float64(robust_scale)
    assert mu > 0 and np.isfinite(mu)
    e = RR.evaluate(table, cloud, X, sigma, min_points, neighbors, min_range, max_range, terms=True)
    r, M, q = e['r'], e['M'], e['q']
    P = len(r)
    J = np.concatenate([-RR.skew(q), np.broadcast_to(np.eye(3), (P, 3, 3))], 2) if P else np.zeros((0, 3, 6))
    Mr = (M @ r[:, :, None])[:, :, 0]
    d2 = (r * Mr).sum(1)
    s = mu / (mu + d2)
    l = s * s
    Hk = l[:, None, None] * (np.swapaxes(J, 1, 2) @ (M @ J))
    gk = l[:, None] * (np.swapaxes(J, 1, 2) @ Mr[:, :, None])[:, :, 0]
    ck = s * d2
    out = dict(H=Hk.sum(0), g=gk.sum(0), cost=float(ck.sum()), weight_sum=float(l.sum()), n_corr=P, n_points=e['n_points'],
               abs_H=np.abs(Hk).sum(0), abs_g=np.abs(gk).sum(0), abs_cost=float(np.abs(ck).sum()), abs_weight_sum=float(np.abs(l).sum()))
    return dict(out, r=r, M=M, q=q, d2=d2, l=l) if terms else out


def register(table, cloud, X0, sigma=0.02, min_points=4, neighbors=1, max_iteration=30, rot_eps=1e-5, trans_eps=1e-4, min_range=0.0,
             max_range=np.inf, robust_scale=None):
    """voxel_register_restatement.register on the weighted evaluation -> dict(transform [4, 4], H, g, cost, weight_sum, abs_*, n_corr,
    n_points, iterations, status); robust_scale None: voxel_register_restatement.register, unchanged."""
    if robust_scale is None:
        return RR.register(table, cloud, X0, sigma, min_points, neighbors, max_iteration, rot_eps, trans_eps, min_range, max_range)
    X = np.array(X0, np.float64, copy=True)
    updates, last = 0, False
    while True:
        e = evaluate(table, cloud, X, sigma, min_points, neighbors, min_range, max_range, robust_scale)
        status = None
        if last:
            status = 1
        elif updates >= max_iteration:
            status = 0
        else:
            delta = RR.cholesky_solve(e['H'], e['g']) if e['n_corr'] > 0 else None
            if delta is None:
                status = 2
        if status is not None:
            return dict(e, transform=X, iterations=updates, status=status)
        X = RR.apply(X, delta)
        updates += 1
        last = bool(np.linalg.norm(delta[:3]) < rot_eps and np.linalg.norm(delta[3:]) < trans_eps)


# ---- the scene -------------------------------------------------------------------------------------------------------------------

def box_points(rng, centre, size, n, noise=0.02):
    """n world points on the top and the four sides of the axis-aligned box (a face's share is its share of the area), each moved by
    N(0, noise) per axis."""
    c, (a, b, h) = np.asarray(centre, np.float64), size
    areas = np.array([a * b, a * h, a * h, b * h, b * h])
    face = rng.choice(5, n, p=areas / areas.sum())
    u, v = rng.uniform(-0.5, 0.5, n), rng.uniform(-0.5, 0.5, n)
    half = np.full(n, 0.5)
    p = np.zeros((n, 3))
    for f, cols in enumerate(((u * a, v * b, half * h), (u * a, -half * b, v * h), (u * a, half * b, v * h), (-half * a, u * b, v * h),
                              (half * a, u * b, v * h))):
        p[face == f] = np.stack(cols, 1)[face == f]
    return c + p + rng.normal(0.0, noise, (n, 3))


def street_with_box(rng, centres, n_box, size=BOX, per_scan=4000, noise=0.02):
    """test_voxel_register.street (eight scans) where scan k also sees a box of n_box points centred at centres[k] in the world, stored
    in the sensor frame after the scan's own points -> (clouds float32 [<= per_scan + n_box, 3], true poses [8, 4, 4])."""
    from test_voxel_register import street
    clouds, poses = street(rng, per_scan=per_scan)
    centres = np.broadcast_to(np.asarray(centres, np.float64), (len(clouds), 3))
    out = []
    for k, cloud in enumerate(clouds):
        inv = np.linalg.inv(poses[k])
        box = box_points(rng, centres[k], size, n_box, noise)
        out.append(np.concatenate([cloud, (box @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)]))
    return out, poses


def moved_box(rng, n_box, centre=(16.0, 3.0, 0.75), shift=(0.3, 0.3, 0.0), moved=4, **kw):
    """The box stands at `centre` in every scan but `moved`, where it stands `shift` further."""
    centres = np.tile(np.asarray(centre, np.float64), (8, 1))
    centres[moved] += shift
    return street_with_box(rng, centres, n_box, **kw)


def moving_box(rng, n_box, centre=(6.0, 3.0, 0.75), step=(0.3, 0.0, 0.0), **kw):
    """The box moves by `step` from every scan to the next."""
    centres = np.asarray(centre, np.float64) + np.arange(8)[:, None] * np.asarray(step, np.float64)
    return street_with_box(rng, centres, n_box, **kw)
