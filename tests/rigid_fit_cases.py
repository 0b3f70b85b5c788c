"""Inputs, the one float64 reference and the criteria of the rigid-fit tests (test_rigid_fit.py, test_rigid_fit_gpu.py).

The solver under test is csrc/procrustes.h (Horn's quaternion by a float64 Jacobi) inside its five clients; the reference is
numpy's float64 SVD, R* = V diag(1, 1, d) U^T with d = sign det(V U^T), for H[a][b] = sum w (s - c_s)_a (r - c_r)_b as the
kernels define it, t* = c_r - R* c_s.  Two rules give the weights and centroids:

  plain    means over the rows, w = 1                                                   (ICP, RANSAC)
  scored   w = max(s, 0) / (sum max(s, 0) + 1e-5), centroids sum w p, NOT renormalised   (eval svd, LGR)

Criteria on a returned 3x4 transform (`out`: the client's output type, fp32 or fp64):

  A  always          max |R^T R - I| <= 1e-6 / 1e-13 and det R > 0.  (9 entries x 2^-24 rounding each, doubled; the same with
                     2^-53 and a margin of 100 for the Jacobi sweeps.)
  B  always          trace(R H) >= (s1 + s2 + d s3) - tau s1, tau = 1e-6 / 1e-13: the optimality that survives a non-unique
                     optimum (rounding nine entries changes the trace by at most 9 x 2^-24 s1).
  C  unique optimum  (s2 + d s3) / s1 >= 1e-3 (the rank threshold of check_pose with the reflection sign put in): the angle
                     between R and R*, measured as tie_aware.rre_rte does, <= 1e-3 deg / 1e-6 deg; max |t - t*| <= 1e-5 m /
                     1e-9 m.  Family `far` (coordinates of 1e4 m), fp32: two fp32 ulps of the largest |t*| component.
  D  H == 0 exactly  R is exactly the identity and t is c_r - c_s rounded to the output type (torch.svd and numpy's SVD of a
                     zero matrix give U = V = I).

Families (seeded; points are stored as float32: +-1 m of spread in a random basis around a centre within +-25 m, moved by a
random rotation and a shift within +-35 m, so every coordinate stays within 80 m).  Local coordinates sit on a jittered
lattice, which keeps the smallest spacing of a cloud above a quarter of a lattice cell (the ICP test needs every row to be
its own nearest neighbour):

  full, noisy (1 cm)   the controls                       coplanar        rank 2 (to the float32 rounding of the stored rows)
  near_coplanar        thickness 1e-6 of the spread        collinear       rank 1, the rotation about the line is free
  one_point            every row equal (plain: H == 0)     single, two     n = 1, n = 2
  half_turn            a turn by exactly pi about x        far             centre (1e4, -2e4, 3e3) m
  mirrored             ref is a mirror image of src plus 1 cm of noise: d = -1
  mirrored_flat        a slab of thickness 1e-3 mirrored in its own plane: d = -1 and still unique.  (Thickness 0 would leave
                       the sign of d to the rounding of a zero singular value; 1e-3 makes it a property of the data.)
  mirrored_tie         six rows on the 2^-6 grid with s2 == s3 and d = -1: Horn's largest eigenvalue is repeated, two
                       optima tie, only A and B apply
  exact*               rows on the 2^-4 grid, a 90-degree turn about z plus a dyadic shift: the data are free of rounding
                       (exact, exact_coplanar, exact_collinear, exact_one_point)
"""
import numpy as np

SIZES = (3, 4, 64, 65, 257)
UNIQUE = 1e-3
BOUNDS = {'fp32': {'ortho': 1e-6, 'trace': 1e-6, 'angle': 1e-3, 'trans': 1e-5},
          'fp64': {'ortho': 1e-13, 'trace': 1e-13, 'angle': 1e-6, 'trans': 1e-9}}
FAMILIES = ('full', 'noisy', 'coplanar', 'near_coplanar', 'collinear', 'one_point', 'single', 'two', 'half_turn', 'mirrored',
            'mirrored_flat', 'mirrored_tie', 'far', 'exact', 'exact_coplanar', 'exact_collinear', 'exact_one_point')
PATTERNS = ('uniform', 'negative', 'zero', 'tiny', 'one')
FAR_CENTRE = (1e4, -2e4, 3e3)
EXACT_TURN = np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])
EXACT_SHIFT = np.array([0.125, -0.0625, 0.03125])
_DIM = {'full': 3, 'noisy': 3, 'coplanar': 2, 'near_coplanar': 2, 'collinear': 1, 'one_point': 0, 'single': 3, 'two': 3,
        'half_turn': 3, 'mirrored': 3, 'mirrored_flat': 2, 'far': 3}
RANK = {'full': 3, 'noisy': 3, 'coplanar': 2, 'near_coplanar': 2, 'collinear': 1, 'one_point': 0, 'single': 0, 'two': 1,
        'half_turn': 3, 'mirrored': 3, 'mirrored_flat': 2, 'mirrored_tie': 3, 'far': 3, 'exact': 3, 'exact_coplanar': 2,
        'exact_collinear': 1, 'exact_one_point': 0}


# ---------------------------------------------------------------------------------------------------------- the reference
def solve(H):
    """-> (R* = V diag(1, 1, d) U^T, singular values s1 >= s2 >= s3, d) of the 3x3 covariance H in float64."""
    U, S, Vt = np.linalg.svd(np.asarray(H, np.float64))
    V = Vt.T
    d = 1.0 if np.linalg.det(V @ U.T) >= 0 else -1.0
    return V @ np.diag([1.0, 1.0, d]) @ U.T, S, d


def weights_of(n, rule, scores=None):
    if rule == 'plain':
        return np.ones(n), float(n)
    assert rule == 'scored'
    s = np.maximum(np.asarray(scores, np.float32).astype(np.float64), 0.0)
    return s, s.sum() + 1e-5


class Fit:
    """The reference's solution of one fit: H, centroids, R*, t*, singular values, d, and the class of the optimum."""

    def __init__(self, src, ref, rule, scores=None, family=''):
        s, r = np.asarray(src, np.float64).reshape(-1, 3), np.asarray(ref, np.float64).reshape(-1, 3)
        w, denom = weights_of(len(s), rule, scores)
        if rule == 'plain':
            self.cs, self.cr = s.sum(0) / denom, r.sum(0) / denom
        else:
            w = w / denom
            self.cs, self.cr = (w[:, None] * s).sum(0), (w[:, None] * r).sum(0)
        self.H = (s - self.cs).T @ (w[:, None] * (r - self.cr))
        self.R, self.S, self.d = solve(self.H)
        self.t = self.cr - self.R @ self.cs
        self.zero = not self.H.any()
        self.gap = (self.S[1] + self.d * self.S[2]) / self.S[0] if self.S[0] > 0 else 0.0
        self.unique = bool(self.gap >= UNIQUE)
        self.optimum = self.S[0] + self.S[1] + self.d * self.S[2]
        self.family, self.rule = family, rule

    @property
    def transform(self):
        return np.concatenate([self.R, self.t[:, None]], 1)


def angle_deg(R, G):
    """The angle between two rotations as tie_aware.rre_rte measures it (through ||G^T R - I||_F)."""
    E = np.asarray(G, np.float64).T @ np.asarray(R, np.float64)
    return float(np.degrees(2.0 * np.arcsin(min(1.0, np.linalg.norm(E - np.eye(3)) / (2.0 * np.sqrt(2.0))))))


def trans_bound(fit, out):
    if out == 'fp32' and fit.family == 'far':
        return 2.0 * float(np.spacing(np.float32(np.abs(fit.t).max())))
    return BOUNDS[out]['trans']


def measure(T, fit, out):
    """The criteria's figures of a returned transform (3x4 or 4x4, any float type) -> dict; `applies` names the criteria."""
    T = np.asarray(T, np.float64)
    R, t = T[:3, :3], T[:3, 3]
    m = {'ortho': float(np.abs(R.T @ R - np.eye(3)).max()), 'det': float(np.linalg.det(R)),
         'trace': float((fit.optimum - np.trace(R @ fit.H)) / fit.S[0]) if fit.S[0] > 0 else 0.0, 'applies': 'AB'}
    if fit.unique:
        m.update(angle=angle_deg(R, fit.R), trans=float(np.abs(t - fit.t).max()), applies='ABC')
    if fit.zero:
        kind = np.float32 if out == 'fp32' else np.float64
        m.update(identity=bool(np.array_equal(R, np.eye(3))), shift=bool(np.array_equal(t, (fit.cr - fit.cs).astype(kind).astype(np.float64))),
                 applies='ABD')
    return m


def check(T, fit, out, where='', worst=None):
    """Assert A, B and whichever of C and D applies; `worst` (dict) collects the largest figure per criterion."""
    m = measure(T, fit, out)
    b = BOUNDS[out]
    if worst is not None:
        for k in ('ortho', 'trace', 'angle', 'trans'):
            if k in m:
                worst[k] = max(worst.get(k, 0.0), m[k])
    assert m['ortho'] <= b['ortho'] and m['det'] > 0, (where, 'A', m)
    assert m['trace'] <= b['trace'], (where, 'B', m)
    if 'angle' in m:
        assert m['angle'] <= b['angle'] and m['trans'] <= trans_bound(fit, out), (where, 'C', m, trans_bound(fit, out))
    if fit.zero:
        assert m['identity'] and m['shift'], (where, 'D', m, T)
    return m


# ---------------------------------------------------------------------------------------------------------------- families
def rotation(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def lattice(rng, n, dim):
    """n local points in [-1, 1]^dim x {0}^(3 - dim): distinct cells of a lattice, each point within a quarter cell of its
    cell's centre, so two points are at least half a cell apart."""
    out = np.zeros((n, 3))
    if dim == 0:
        return out
    m = 1
    while m ** dim < n:
        m += 1
    cells = rng.permutation(m ** dim)[:n]
    cell = 2.0 / m
    for a in range(dim):
        out[:, a] = -1.0 + cell * ((cells // m ** a) % m + 0.5 + rng.uniform(-0.25, 0.25, n))
    return out


class Case:
    def __init__(self, family, n, src, ref, motion=None):
        self.family, self.n, self.src, self.ref, self.motion = family, n, np.ascontiguousarray(src, np.float32), np.ascontiguousarray(ref, np.float32), motion
        self.name = f'{family}/{n}'

    def fit(self, rule, scores=None, rows=None):
        rows = slice(None) if rows is None else rows
        return Fit(self.src[rows], self.ref[rows], rule, None if scores is None else np.asarray(scores)[rows], self.family)


def _seed(family, n):
    return 1000 * FAMILIES.index(family) + n


WELL_SPREAD = ('full', 'noisy', 'coplanar', 'near_coplanar', 'half_turn', 'far', 'mirrored', 'mirrored_flat', 'exact', 'exact_coplanar')


def make(family, n, seed=None):
    """The case of a family and size.  Families whose optimum is meant to be unique redraw (next seed) until their gap
    (s2 + d s3) / s1 is at least 0.02 -- three or four random rows can be a sliver -- so no case sits near the class boundary."""
    seed = _seed(family, n) if seed is None else seed
    while True:
        case = _make(family, n, np.random.default_rng(seed))
        if family not in WELL_SPREAD or (family == 'mirrored' and case.n < 4) or case.fit('plain').gap >= 0.02:
            return case
        seed += 100003


def exact_case(family, n, rng):
    """Rows on the 2^-4 grid within +-25 m, distinct, ref = Rz(90 deg) src + (1/8, -1/16, 1/32): no rounding anywhere."""
    base = rng.integers(-300, 300, 3)
    if family == 'exact_collinear':
        p = np.outer(rng.permutation(33)[:n] - 16 if n <= 33 else rng.permutation(801)[:n] - 400, [1, 2, -1])
    elif family == 'exact_one_point':
        p = np.tile(rng.integers(-16, 17, 3), (n, 1))
    else:  # n distinct cells of the 33^3 (33^2: coplanar) grid
        cells = rng.permutation(33 ** (2 if family == 'exact_coplanar' else 3))[:n]
        p = np.stack([cells % 33 - 16, cells // 33 % 33 - 16, cells // 1089 - 16 if family == 'exact' else 0 * cells], 1)
    src = (p + base) / 16.0
    ref = src @ EXACT_TURN.T + EXACT_SHIFT
    motion = np.eye(4)
    motion[:3, :3], motion[:3, 3] = EXACT_TURN, EXACT_SHIFT
    assert np.array_equal(src.astype(np.float32), src) and np.array_equal(ref.astype(np.float32), ref)
    return Case(family, n, src, ref, motion)


def tie_case(offset=(0.0, 0.0, 0.0)):
    """+-u1, +-u2, +-u3 with u1 = (3, 4, 0) / 8, u2 = (-4, 3, 0) / 16, u3 = (0, 0, 5) / 16 (orthogonal, |u2| == |u3|); ref
    mirrors u3 and turns by 90 degrees about x.  H = 2 sum u u'^T exactly: s1 = 2 |u1|^2, s2 == s3 = 2 |u2|^2, d = -1."""
    u = np.array([[3, 4, 0], [-4, 3, 0], [0, 0, 5]]) / np.array([[8.0], [16.0], [16.0]])
    src = np.concatenate([u, -u])
    Q = np.array([[1.0, 0, 0], [0, 0, -1], [0, 1, 0]])
    ref = (src * [1, 1, -1]) @ Q.T
    off = np.asarray(offset, np.float64)
    c = Case('mirrored_tie', 6, src + off, ref + off @ Q.T + EXACT_SHIFT)
    assert np.array_equal(c.src.astype(np.float64), src + off)
    return c


def _make(family, n, rng):
    if family.startswith('exact'):
        return exact_case(family, n, rng)
    if family == 'mirrored_tie':
        return tie_case()
    n = {'single': 1, 'two': 2}.get(family, n)
    B, R = rotation(rng), rotation(rng)
    local = lattice(rng, n, _DIM[family])
    if family == 'one_point':
        local[:] = rng.uniform(-1, 1, 3)
    if family in ('near_coplanar', 'mirrored_flat'):  # a slab: the lattice in the plane, the thickness across it
        local[:, 2] = rng.uniform(-1, 1, n) * (1e-6 if family == 'near_coplanar' else 1e-3)
    centre = np.asarray(FAR_CENTRE) if family == 'far' else rng.uniform(-25, 25, 3)
    src = (local @ B.T + centre).astype(np.float32)
    t = rng.uniform(-35, 35, 3)
    if family == 'half_turn':
        R = np.diag([1.0, -1.0, -1.0])
    if family == 'mirrored':
        u = rng.normal(size=3)
        R = R @ (np.eye(3) - 2.0 * np.outer(u, u) / (u @ u))
    if family == 'mirrored_flat':  # mirror the first in-plane axis, about the centre; no rotation on top, so the optimum is the half turn about the second
        R = np.eye(3) - 2.0 * np.outer(B[:, 0], B[:, 0])
        t = t + centre - R @ centre
    ref = src.astype(np.float64) @ R.T + t
    if family in ('noisy', 'mirrored'):
        ref = ref + rng.normal(size=ref.shape) * 0.01
    motion = None
    if family not in ('mirrored', 'mirrored_flat'):
        motion = np.eye(4)
        motion[:3, :3], motion[:3, 3] = R, t
    return Case(family, n, src, ref, motion)


def sizes_of(family):
    return {'single': (1,), 'two': (2,), 'mirrored_tie': (6,)}.get(family, SIZES)


def scores_of(pattern, n, seed=0):
    """The `scored` rule's weight patterns, float32 [n]."""
    rng = np.random.default_rng(7000 + 10 * n + seed)
    s = rng.uniform(0.05, 1.0, n).astype(np.float32)
    if pattern == 'negative':
        s[int(rng.integers(n))] = np.float32(-0.5)
    elif pattern == 'zero':
        s[:] = 0
    elif pattern == 'tiny':  # sum s = 1e-5 (to float32 rounding): the weights are halved and the centroids with them
        s = (s.astype(np.float64) * (1e-5 / s.astype(np.float64).sum())).astype(np.float32)
    elif pattern == 'one':
        s[:] = 0
        s[int(rng.integers(n))] = np.float32(1.0)
    else:
        assert pattern == 'uniform'
    return s


# ----------------------------------------------------------------------------------------------- RANSAC's minimal samples
def sample_class(rows, src):
    """Class of one minimal sample (row indices, with repetitions) -> 'fit' (>= 3 distinct non-collinear rows), 'line' (two
    distinct rows or more on one line) or 'point' (one row)."""
    p = np.unique(np.asarray(src, np.float64)[np.unique(rows)], axis=0)
    if len(p) == 1:
        return 'point'
    d = p[1:] - p[0]
    return 'line' if np.linalg.matrix_rank(d, tol=1e-9 * np.abs(d).max()) == 1 else 'fit'


def rows_on_line(rows, src):
    """How many rows of `src` lie on the line through the (collinear) sample."""
    s = np.asarray(src, np.float64)
    p = np.unique(s[np.unique(rows)], axis=0)
    u = (p[1] - p[0]) / np.linalg.norm(p[1] - p[0])
    off = (s - p[0]) - np.outer((s - p[0]) @ u, u)
    return int((np.linalg.norm(off, axis=1) <= 1e-9).sum())


def recount(R, t, src, ref, threshold):
    """Inliers of (R, t) in float64, and the distance of the nearest residual to the threshold."""
    s, r = np.asarray(src, np.float64), np.asarray(ref, np.float64)
    res = np.linalg.norm(s @ np.asarray(R, np.float64).T + t - r, axis=1)
    thr = float(np.float32(threshold))
    return int((res < thr).sum()), float(np.abs(res - thr).min())
