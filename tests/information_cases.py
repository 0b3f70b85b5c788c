"""Seeded inputs of tests/test_information_gpu.py, generated on the host so that tests/test_information.py can assert, without a
GPU, that every row is decided (information_restatement.assert_decided): float32 clouds in a 20 m box at r = 0.6 at every
size where the kernels take another path -- 64 rows per wavefront of the reduction, 256 per workgroup, the sweep's LDS tile of
1 024 target rows --, one case at 60-80 m coordinates, a pair exactly on the radius, an exact tie between two target rows.
A case is a dict: source, target, radius and, where set, s_transform, t_transform, boundary_rows, tie_rows, expect_C."""
import numpy as np

RADIUS = 0.6
N_Q = (0, 1, 63, 64, 65, 257)
N_S = (0, 1, 1025)


def rotation(axis, angle, t):
    k = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)
    T[:3, 3] = t
    return T


def cloud_pair(n_q, n_s, seed, lo=0.0, hi=20.0):
    """Every second source row lies within 0.3 m per axis of a target row, the others anywhere in the box."""
    rng = np.random.default_rng(seed)
    target = rng.uniform(lo, hi, size=(n_s, 3)).astype(np.float32)
    source = rng.uniform(lo, hi, size=(n_q, 3)).astype(np.float32)
    if n_s > 0:
        near = np.arange(0, n_q, 2)
        source[near] = target[rng.integers(0, n_s, size=len(near))] + rng.uniform(-0.3, 0.3, size=(len(near), 3)).astype(np.float32)
    return {'source': source, 'target': target, 'radius': RADIUS}


def sized(n_q, n_s):
    return lambda: cloud_pair(n_q, n_s, 1000 * n_q + n_s)


def path():
    """The 257 x 1025 pair with every source row inside the target's box [0, 20): with one cell over the target no source row lies
    outside the cell box (a row outside it is never settled by the cell search and would take the sweep at any cell edge)."""
    c = cloud_pair(257, 1025, 13)
    c['source'] = np.clip(c['source'], np.float32(0.0), np.float32(19.75))
    return c


def far():
    return cloud_pair(257, 1025, 7, 60.0, 80.0)


def moved_both():
    """Both transforms set (general rotations: the moved coordinates round), more than one workgroup of source rows."""
    c = cloud_pair(300, 1100, 11)
    S, T = rotation((1, 2, 3), 0.3, (0.5, -1.25, 2.0)), rotation((-2, 1, 0.5), -0.7, (3.0, 0.25, -1.0))
    # the target is stored as T^-1 of the cloud above, the source as S^-1: after moving, the pair is the overlapping one again
    inv = np.linalg.inv
    for key, M in (('source', inv(S)), ('target', inv(T))):
        p = c[key].astype(np.float64)
        c[key] = (p @ M[:3, :3].T + M[:3, 3]).astype(np.float32)
    c['s_transform'], c['t_transform'] = S, T
    return c


def one_transform():
    """moved_both with the target stored where its transform puts it (rounded to float32): Open3D's signature, one transform."""
    c = moved_both()
    T = c.pop('t_transform')
    p = c['target'].astype(np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    c['target'] = np.stack([((T[a, 0] * x + T[a, 1] * y) + T[a, 2] * z) + T[a, 3] for a in range(3)], axis=1).astype(np.float32)
    return c


def boundary():
    """r = 0.625: row 0 lies exactly on the radius (d2 = 0.390625 and its root are exact) and has no correspondence; row 1 is the
    same pair one float32 step nearer and has one; row 2 lies outside."""
    near = np.nextafter(np.float32(0.625), np.float32(0))
    return {'source': np.float32([[0, 0, 0], [0, 8, 0], [0, 16, 0]]),
            'target': np.float32([[0.625, 0, 0], [near, 8, 0], [0.75, 16, 0]]),
            'radius': 0.625, 'boundary_rows': (0,), 'expect_rows': [1], 'expect_C': 1}


def tie():
    """Source row 1 = (1, 2, 3) is equidistant (d2 = 0.25, exact) from the moved target rows 2 = (1.5, 2, 3) and 5 = (0.5, 2, 3); the
    target cloud is stored in front of an exact quarter turn and translation, so the tie is exact after moving as well."""
    T = np.array([[0, -1, 0, 0.5], [1, 0, 0, -1.25], [0, 0, 1, 2.0], [0, 0, 0, 1]], np.float64)  # T p = (-y + 0.5, x - 1.25, z + 2)
    rng = np.random.default_rng(5)
    target = rng.uniform(30.0, 40.0, size=(8, 3)).astype(np.float32)
    target[2], target[5] = (3.25, -1.0, 1.0), (3.25, 0.0, 1.0)
    source = np.float32([[-8.0, 35.0, 36.0], [1, 2, 3], [40, 40, 40]])
    source[0] = (-(target[0, 1]) + 0.5 + 0.25, target[0, 0] - 1.25, target[0, 2] + 2.0)  # 0.25 m from the moved row 0
    return {'source': source, 'target': target, 'radius': RADIUS, 't_transform': T, 'tie_rows': (1,), 'tie_targets': (2, 5),
            'expect_C': 2}


CASES = {f'{n_q}x{n_s}': sized(n_q, n_s) for n_q in N_Q for n_s in N_S}
CASES.update(path=path, far=far, moved_both=moved_both, one_transform=one_transform, boundary=boundary, tie=tie)

# path invariance (the `path` case): the automatic cell; an edge whose searched cube (at most 3 cells from the query) stays
# below every nearest distance, so that every row takes the sweep; an edge that makes the target one cell, which holds every
# source row as well
PATH_CASE = 'path'
PATH_CELLS = {'auto': None, 'sweep': 1e-4, 'one_cell': 1e5}
