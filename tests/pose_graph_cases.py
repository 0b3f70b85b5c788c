"""Seeded pose graphs for the pose-graph tests (numpy float64; nothing here calls the code under test).

A case is a dict: truth [N, 4, 4], nodes [N, 4, 4] (the start), edges int64 [E, 2] rows (s, t), transforms [E, 4, 4]
(X_t^-1 X_s of the truth, computed in float64, plus noise where the case says so), informations [E, 6, 6] (random symmetric
positive definite), uncertain uint8 [E]."""
import numpy as np

import pose_graph_restatement as R

SCALE = 100.0  # metres


def random_pose(rng, scale=SCALE):
    w = rng.normal(size=3)
    w *= rng.uniform(0.0, 3.0) / np.linalg.norm(w)
    X = np.eye(4)
    X[:3, :3] = R.so3_exp(w)
    X[:3, 3] = rng.uniform(-0.5 * scale, 0.5 * scale, size=3)
    return X


def random_information(rng):
    A = rng.normal(size=(6, 6))
    L = A @ A.T + 0.5 * np.eye(6)
    return 0.5 * (L + L.T)


def perturbation(rng, angle, distance):
    w = rng.normal(size=3)
    w *= rng.uniform(0.0, angle) / np.linalg.norm(w)
    t = rng.normal(size=3)
    t *= rng.uniform(0.0, distance) / np.linalg.norm(t)
    return np.concatenate([w, t])


def inverse(X):
    Y = np.eye(4)
    Y[:3, :3] = X[:3, :3].T
    Y[:3, 3] = -X[:3, :3].T @ X[:3, 3]
    return Y


def make(truth, edges, rng, start_angle=0.1, start_distance=0.5, noise_angle=0.0, noise_distance=0.0, uncertain=None):
    truth = np.asarray(truth, dtype=np.float64)
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    nodes = truth.copy()
    for i in range(1, len(truth)):
        nodes[i] = R.retract(truth[i], perturbation(rng, start_angle, start_distance))
    transforms = np.zeros((len(edges), 4, 4))
    for e, (s, t) in enumerate(edges):
        T = inverse(truth[t]) @ truth[s]
        T[3] = (0.0, 0.0, 0.0, 1.0)
        if noise_angle > 0.0 or noise_distance > 0.0:
            T = R.retract(T, perturbation(rng, noise_angle, noise_distance))
        transforms[e] = T
    informations = np.stack([random_information(rng) for _ in edges]) if len(edges) else np.zeros((0, 6, 6))
    unc = np.zeros(len(edges), np.uint8) if uncertain is None else np.asarray(uncertain, np.uint8)
    return dict(truth=truth, nodes=nodes, edges=edges, transforms=transforms, informations=informations, uncertain=unc)


def ring_edges(n):
    return [(i + 1, i) for i in range(n - 1)] + [(0, n - 1)]


def chords(rng, n, count):
    out = []
    while len(out) < count:
        s, t = (int(v) for v in rng.integers(0, n, size=2))
        if abs(s - t) > 1 and (s, t) not in out:
            out.append((s, t))
    return out


def consistent(name):
    """The consistent graphs of the GPU tests: exact edges, starts up to 0.1 rad and 0.5 m from the truth."""
    seed = dict(pair=1, ring3=2, ring40=3, double=4, hub=5, big=6)[name]
    rng = np.random.default_rng(seed)
    if name == 'pair':
        n, edges = 2, [(1, 0)]
    elif name == 'ring3':
        n, edges = 3, ring_edges(3)
    elif name == 'ring40':
        n, edges = 40, ring_edges(40) + chords(rng, 40, 5)
    elif name == 'double':  # two edges between the same two nodes (one in each direction) in a 4-ring
        n, edges = 4, ring_edges(4) + [(2, 1), (1, 2)]
    elif name == 'hub':  # node 7 has 300 incident edges
        n = 301
        edges = [(i, 7) if i % 2 else (7, i) for i in range(n) if i != 7]
    elif name == 'big':  # more nodes than a workgroup has threads
        n, edges = 1100, ring_edges(1100) + chords(rng, 1100, 120)
    else:
        raise KeyError(name)
    return make([random_pose(rng) for _ in range(n)], edges, rng)


CONSISTENT = ('pair', 'ring3', 'ring40', 'double', 'hub', 'big')


def trajectory_truth(rng, n, step=2.0):
    """A drive: poses about `step` metres apart with gentle turns."""
    X = [np.eye(4)]
    for _ in range(n - 1):
        d = np.concatenate([rng.normal(scale=0.05, size=3), [step, 0.0, 0.0] + rng.normal(scale=0.1, size=3)])
        X.append(R.retract(X[-1], d))
    return X


def tree(n=50):
    """A chain started at the chained poses: cost 0 up to rounding."""
    rng = np.random.default_rng(7)
    truth = trajectory_truth(rng, n)
    return make(truth, [(i + 1, i) for i in range(n - 1)], rng, start_angle=0.0, start_distance=0.0, noise_angle=0.01,
                noise_distance=0.05)


def chained_start(case):
    """Nodes chained along the odometry edges (i + 1, i) of a case from node 0: X_{i+1} = X_i T."""
    nodes = case['truth'].copy()
    for e, (s, t) in enumerate(case['edges']):
        if s == t + 1:
            nodes[s] = nodes[t] @ case['transforms'][e]
    return nodes


def noisy(n=60, loops=10, gross=None):
    """Odometry plus loop edges (uncertain) with measurement noise 0.01 rad / 0.05 m, started at the chained odometry.
    gross: the index (among the loop edges) of one replaced by a gross error of 0.5 rad and 5 m."""
    rng = np.random.default_rng(8)
    truth = trajectory_truth(rng, n)
    odo = [(i + 1, i) for i in range(n - 1)]
    loop = [(int(s), int(s) - int(rng.integers(10, 30))) for s in rng.choice(np.arange(30, n), size=loops, replace=False)]
    case = make(truth, odo + loop, rng, start_angle=0.0, start_distance=0.0, noise_angle=0.01, noise_distance=0.05,
                uncertain=[0] * len(odo) + [1] * len(loop))
    if gross is not None:
        e = len(odo) + gross
        w = np.array([0.3, -0.3, 0.26])
        w *= 0.5 / np.linalg.norm(w)
        case['transforms'][e] = R.retract(case['transforms'][e], np.concatenate([w, [3.0, -4.0, 0.0]]))
        case['gross_edge'] = e
    case['nodes'] = chained_start(case)
    return case
