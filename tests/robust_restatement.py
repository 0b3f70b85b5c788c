"""Float64 numpy restatement of rdm_robust_registration (include/rdmnet_hip.h), written from the
definition and not from the kernels: compatibility graph, core numbers (networkx.core_number), maximum clique
(networkx.find_cliques: all maximal cliques, of the largest the lexicographically smallest ascending row list), GNC-TLS
rotation and per-axis truncated-least-squares translation voting.  Also the fixture generator of the robust tests and the
conditions a fixture has to meet (`check_fixture`), asserted here so that a test cannot run on a fixture that would make
it a test of rounding."""
import numpy as np

MARGIN = 1e-9


def horn_rotation(H):
    """The rotation R that maximises trace(R H) for H = sum w a b^T (R moves a onto b): Horn's quaternion solution."""
    Sxx, Sxy, Sxz, Syx, Syy, Syz, Szx, Szy, Szz = H.reshape(-1)
    N = np.array([[Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx],
                  [Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz],
                  [Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy],
                  [Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz]])
    vals, vecs = np.linalg.eigh(N)
    qw, qx, qy, qz = vecs[:, np.argmax(vals)]
    return np.array([[1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qz * qw), 2 * (qx * qz + qy * qw)],
                     [2 * (qx * qy + qz * qw), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qx * qw)],
                     [2 * (qx * qz - qy * qw), 2 * (qy * qz + qx * qw), 1 - 2 * (qx * qx + qy * qy)]])


def _norms(p):
    d = p[None, :, :] - p[:, None, :]  # d[i, j] = p_j - p_i
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


def compatibility(src, ref, noise_bound, cbar2=1.0):
    """-> (adjacency bool [C, C], the margin |difference - threshold| of the closest finite pair)."""
    src, ref = np.asarray(src, np.float32).astype(np.float64), np.asarray(ref, np.float32).astype(np.float64)
    C = len(src)
    thr = (2.0 * noise_bound) * np.sqrt(cbar2)
    fin = np.isfinite(src).all(1) & np.isfinite(ref).all(1)
    with np.errstate(invalid='ignore', over='ignore'):
        diff = np.abs(_norms(src) - _norms(ref))
        adj = diff <= thr
    ok = fin[:, None] & fin[None, :] & ~np.eye(C, dtype=bool)
    adj &= ok
    margin = np.abs(diff[ok] - thr).min() if ok.any() else np.inf
    return adj, margin


def core_numbers(adj):
    import networkx as nx
    G = nx.from_numpy_array(adj.astype(np.uint8))
    core = nx.core_number(G)
    return np.array([core[i] for i in range(len(adj))], np.int32).reshape(-1)


def maximum_cliques(adj):
    """Every maximum clique as an ascending tuple, sorted: [0] is the definition's."""
    import networkx as nx
    if len(adj) == 0:
        return []
    G = nx.from_numpy_array(adj.astype(np.uint8))
    cliques = [tuple(sorted(c)) for c in nx.find_cliques(G)]
    size = max(len(c) for c in cliques)
    return sorted(c for c in cliques if len(c) == size)


def select_rows(adj, inlier_selection='clique'):
    C = len(adj)
    if inlier_selection == 'none' or C == 0:
        return np.arange(C)
    if inlier_selection == 'kcore':
        core = core_numbers(adj)
        return np.nonzero(core == core.max())[0]
    assert inlier_selection == 'clique'
    return np.array(maximum_cliques(adj)[0])


def pair_rows(K):
    """(p, q) of every measurement pair p < q, in the order p K - p (p + 1) / 2 + q - p - 1."""
    return np.triu_indices(K, 1)


def residual2(R, a, b):
    dx = b[:, 0] - ((R[0, 0] * a[:, 0] + R[0, 1] * a[:, 1]) + R[0, 2] * a[:, 2])
    dy = b[:, 1] - ((R[1, 0] * a[:, 0] + R[1, 1] * a[:, 1]) + R[1, 2] * a[:, 2])
    dz = b[:, 2] - ((R[2, 0] * a[:, 0] + R[2, 1] * a[:, 1]) + R[2, 2] * a[:, 2])
    return (dx * dx + dy * dy) + dz * dz


def gnc_tls(a, b, n2, gnc_factor=1.4, max_iterations=100, cost_threshold=1e-12, order=None):
    """-> (R, weights, iterations).  order: a permutation of the pairs in which the sums are taken (the test's measure of the
    restatement's own spread); the weights come back in the given pair order."""
    if order is not None:
        a, b = a[order], b[order]
    w = np.ones(len(a))
    mu = prev_cost = None
    R = np.eye(3)
    iterations = 0
    for it in range(max_iterations):
        H = ((w[:, None] * a)[:, :, None] * b[:, None, :]).sum(0)
        R = horn_rotation(H)
        r2 = residual2(R, a, b)
        iterations = it + 1
        if it == 0:
            with np.errstate(divide='ignore'):
                mu = 1.0 / ((2.0 * r2.max()) / n2 - 1.0)
            if mu <= 0:
                break
        th1, th2 = ((mu + 1.0) / mu) * n2, (mu / (mu + 1.0)) * n2
        cost = (w * r2).sum()
        with np.errstate(divide='ignore', invalid='ignore'):
            mid = np.sqrt(((n2 * mu) * (mu + 1.0)) / r2) - mu
        w = np.where(r2 >= th1, 0.0, np.where(r2 <= th2, 1.0, mid))
        if it > 0 and abs(cost - prev_cost) < cost_threshold:
            break
        prev_cost = cost
        mu = mu * gnc_factor
    if order is not None:
        back = np.empty_like(w)
        back[order] = w
        w = back
    return R, w, iterations


def tls_axis(x, c):
    """-> (estimate, sorted distinct costs).  Empty consensus sets are skipped."""
    K = len(x)
    h = np.sort(np.concatenate([x - c, x + c]))
    mids = (h[:-1] + h[1:]) * 0.5
    best = (np.inf, 0.0)
    costs = []
    for m in mids:
        S = np.abs(x - m) <= c
        n = int(S.sum())
        if n == 0:
            continue
        est = x[S].sum() / n
        cost = ((x[S] - est) ** 2).sum() + (K - n) * (c * c)
        costs.append(cost)
        if cost < best[0]:  # ascending midpoints: equals keep the lowest
            best = (cost, est)
    return best[1], np.unique(costs)


class Restated:
    pass


def robust_registration(src, ref, noise_bound=0.01, cbar2=1.0, gnc_factor=1.4, max_iterations=100, cost_threshold=1e-12,
                        inlier_selection='clique', order=None):
    src32, ref32 = np.asarray(src, np.float32).reshape(-1, 3), np.asarray(ref, np.float32).reshape(-1, 3)
    s, r = src32.astype(np.float64), ref32.astype(np.float64)
    out = Restated()
    C = len(s)
    adj, out.threshold_margin = compatibility(src32, ref32, noise_bound, cbar2)
    out.adjacency = adj
    out.degree = adj.sum(1).astype(np.int32)
    out.edges = int(adj.sum()) // 2
    out.core = core_numbers(adj) if C else np.zeros(0, np.int32)
    out.selected = select_rows(adj, inlier_selection)
    K = out.K = len(out.selected)
    out.valid = int(K >= 3)
    out.transform = np.eye(4)
    out.iterations, out.weights, out.translation_inliers, out.cost_margin = 0, np.zeros(0), 0, np.inf
    if out.valid:
        out.transform, out.weights, out.iterations, out.translation_inliers, out.cost_margin = estimate_pose(
            s, r, out.selected, noise_bound, cbar2, gnc_factor, max_iterations, cost_threshold, order)
    return out


def estimate_pose(s, r, rows, noise_bound=0.01, cbar2=1.0, gnc_factor=1.4, max_iterations=100, cost_threshold=1e-12, order=None):
    """Stages 4 and 5 on the selected rows of the float64 clouds -> (transform, weights, iterations, translation inliers, the
    relative margin between the best and the next translation cost)."""
    p, q = pair_rows(len(rows))
    a, b = s[rows[q]] - s[rows[p]], r[rows[q]] - r[rows[p]]
    n2 = ((2.0 * noise_bound) * (2.0 * noise_bound)) * cbar2
    R, weights, iterations = gnc_tls(a, b, n2, gnc_factor, max_iterations, cost_threshold, order)
    c = noise_bound * np.sqrt(cbar2)
    ss, rr = s[rows], r[rows]
    x = np.stack([rr[:, k] - ((R[k, 0] * ss[:, 0] + R[k, 1] * ss[:, 1]) + R[k, 2] * ss[:, 2]) for k in range(3)])
    t, margin = np.zeros(3), np.inf
    for k in range(3):
        t[k], costs = tls_axis(x[k], c)
        if len(costs) > 1:
            margin = min(margin, (costs[1] - costs[0]) / costs[1])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T, weights, iterations, int((np.abs(x - t[:, None]) <= c).all(0).sum()), margin


def permutation_spread(src, ref, res, n=20, seed=1, **kw):
    """The restatement's own spread: the largest change of a rotation entry, a translation entry and a weight, and the set of
    iteration counts, over n random orders of the measurement pairs in the sums (res: the restated result in the stated
    order)."""
    s, r = np.asarray(src, np.float32).astype(np.float64), np.asarray(ref, np.float32).astype(np.float64)
    rng = np.random.default_rng(seed)
    dR = dt = dw = 0.0
    its = {res.iterations}
    for _ in range(n):
        T, w, it, _, _ = estimate_pose(s, r, res.selected, order=rng.permutation(len(res.weights)), **kw)
        dR = max(dR, np.abs(T[:3, :3] - res.transform[:3, :3]).max())
        dt = max(dt, np.abs(T[:3, 3] - res.transform[:3, 3]).max())
        dw = max(dw, np.abs(w - res.weights).max())
        its.add(it)
    return dR, dt, dw, its


# ---- fixtures -----------------------------------------------------------------------------------------------------------------

def random_pose(rng, max_translation=5.0):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, rng.uniform(-max_translation, max_translation, 3)
    return T


def make_fixture(C, n_in, noise_bound, seed=0, box=40.0, groups=1):
    """C rows in a +-box cube; `groups` disjoint sets of n_in rows (random positions) are each moved by a random pose of
    their own plus noise of norm <= 0.45 noise_bound, the other rows are random on both sides.
    -> (src f32, ref f32, [rows of group g], [pose of group g])."""
    rng = np.random.default_rng(seed)
    src = rng.uniform(-box, box, (C, 3))
    ref = rng.uniform(-box, box, (C, 3))
    perm = rng.permutation(C)
    rows, poses = [], []
    for g in range(groups):
        idx = np.sort(perm[g * n_in:(g + 1) * n_in])
        T = random_pose(rng)
        d = rng.normal(size=(n_in, 3))
        d *= (rng.uniform(0, 0.45 * noise_bound, n_in) / np.linalg.norm(d, axis=1))[:, None]
        ref[idx] = src[idx] @ T[:3, :3].T + T[:3, 3] + d
        rows.append(idx)
        poses.append(T)
    return src.astype(np.float32), ref.astype(np.float32), rows, poses


def check_fixture(res, unique_clique=True, adj_for_cliques=None):
    """The conditions of a fixture, on its restated result: no pair within MARGIN of the compatibility threshold, one maximum
    clique (unless the case is about ties), the best translation cost of every axis below the next one by more than MARGIN
    relative."""
    assert res.threshold_margin > MARGIN, res.threshold_margin
    if unique_clique:
        assert len(maximum_cliques(res.adjacency if adj_for_cliques is None else adj_for_cliques)) == 1
    if res.valid:
        assert res.cost_margin > MARGIN, res.cost_margin


def pose_error(T, gt):
    """-> (rotation error in degrees, translation error)."""
    c = (np.trace(T[:3, :3].T @ gt[:3, :3]) - 1.0) / 2.0
    return float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0)))), float(np.linalg.norm(T[:3, 3] - gt[:3, 3]))


def select_num_corr(scores, num_corr):
    """rdm_eval_pairs' own rule for --num_corr L: the first L rows in the order (score descending, row ascending), kept in row
    order; every row when L is None or >= C."""
    scores = np.asarray(scores)
    C = len(scores)
    if num_corr is None or C <= num_corr:
        return np.arange(C)
    order = sorted(range(C), key=lambda i: (-float(scores[i]), i))
    return np.array(sorted(order[:num_corr]))
