"""The exact restatements of tests/exact_matching.py checked on the CPU: fma32 bit for bit against rational arithmetic
(the GPU tests of the index kernels stand on it), and the small restatements against plain statements of their rules."""
from fractions import Fraction

import numpy as np

import exact_matching as em

F32 = np.float32


def round_f32(x):
    """Round a Fraction to the nearest fp32 (ties to even), subnormals included; finite results only."""
    if x == 0:
        return F32(0.0)
    ax = abs(x)
    e = ax.numerator.bit_length() - ax.denominator.bit_length()  # 2^e <= |x| < 2^(e+2)
    if ax < Fraction(2) ** e:
        e -= 1
    elif ax >= Fraction(2) ** (e + 1):
        e += 1
    q = Fraction(2) ** (max(e, -126) - 23)                          # spacing of fp32 values at |x|
    r = round(ax / q) * q                                           # round() of a Fraction: half to even
    assert r < Fraction(2) ** 128
    return F32(float(r) if x > 0 else -float(r))


def fma_exact(a, b, c):
    """fp32 fmaf by rational arithmetic, with IEEE 754's sign of an exact zero (round to nearest)."""
    x = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    if x == 0:
        p_neg = (np.signbit(a) != np.signbit(b))
        both_neg = p_neg and np.signbit(c) and (a == 0 or b == 0) and c == 0
        return F32(-0.0) if both_neg else F32(0.0)
    return round_f32(x)


def bits(v):
    return np.asarray(v, F32).view(np.uint32)


def planted_cases(rng):
    a, b, c = [], [], []

    def add(x, y, z):
        a.append(x), b.append(y), c.append(z)

    one = 2.0 ** -23
    # exact midpoints: (1 + i 2^-12)(1 + j 2^-12) with i, j odd has a set 2^-24 bit below the last fp32 bit of [1, 2)
    for i in (1, 3, 5, 255, 1023, 2047):
        for j in (1, 7, 1001, 2047):
            x, y = 1 + i * 2.0 ** -12, 1 + j * 2.0 ** -12
            for z in (0.0, -0.0, 2.0 ** -60, -2.0 ** -60, 2.0 ** -149, -2.0 ** -149, 1.0, -1.0, 0.5, -4.0):
                add(x, y, z)
                add(-x, y, z)
    # midpoints made by c: y * 1 + ulp(y)/2, on either side, at several binades (and the power-of-two boundary below y)
    for y in (1.0, 1 + one, 1.5, 2 - one, 80.0, 79.99, 3.0e-30, 6.0e4, 1.0e-38):
        u = float(np.spacing(F32(y)))
        for z in (u / 2, -u / 2, u / 4, -u / 4, 3 * u / 2):
            if np.float32(z) == z:
                add(y, 1.0, z)
                add(-y, 1.0, -z)
    # c far below a*b (sticky bit only) and a*b far below c
    for x, y in ((1 + one, 1 - one), (3.0, 1 / 3), (80.0, 80.0), (1e10, 1e10), (1e-20, 1e-20)):
        for z in (1e-30, -1e-30, 1e-45, -1e-45):
            add(x, y, z)
            add(z, z, x * y)
    # cancellation: a*b + c == 0 exactly, and c = -fl32(a*b) leaving the (tiny, possibly subnormal) product error
    for _ in range(300):
        x, y = F32(rng.uniform(-2, 2) * 2.0 ** rng.integers(-70, 30)), F32(rng.uniform(-2, 2) * 2.0 ** rng.integers(-70, 30))
        add(x, y, -(x * y))
        xs = F32(rng.integers(-2 ** 11, 2 ** 11) * 2.0 ** rng.integers(-60, 10))   # 12-bit: the product is fp32-exact
        ys = F32(rng.integers(-2 ** 11, 2 ** 11) * 2.0 ** rng.integers(-60, 10))
        add(xs, ys, -F32(float(xs) * float(ys)))
    # products and sums in the subnormal range
    for _ in range(300):
        x = F32(rng.uniform(1, 2) * 2.0 ** rng.integers(-90, -60))
        y = F32(rng.uniform(1, 2) * 2.0 ** rng.integers(-90, -60) * rng.choice([-1, 1]))
        add(x, y, F32(rng.uniform(-1, 1) * 2.0 ** rng.integers(-149, -120)))
    # 80 m coordinates: the terms of ref_sq_dist at the distances of a KITTI scan
    for _ in range(300):
        x, y = F32(rng.uniform(60, 80)), F32(rng.uniform(60, 80) + rng.integers(-5, 5) * 1e-3)
        add(x, y, F32(rng.uniform(60, 80)) * F32(rng.uniform(60, 80)))
        add(x, -y, F32(x) * F32(y))
    return (np.array(v, F32) for v in (a, b, c))


def random_cases(rng, n):
    a = (rng.uniform(-2, 2, n) * 2.0 ** rng.integers(-40, 40, n)).astype(F32)
    b = (rng.uniform(-2, 2, n) * 2.0 ** rng.integers(-40, 40, n)).astype(F32)
    c = (rng.uniform(-2, 2, n) * 2.0 ** rng.integers(-90, 90, n)).astype(F32)
    near = rng.uniform(size=n) < 0.5  # half of them: c close to -a*b, so the sum cancels to a few bits
    pert = F32(1) + (rng.integers(-64, 64, n) * 2.0 ** -23).astype(F32)
    c[near] = -(a[near] * b[near]) * pert[near]
    return a, b, c


def test_fma32_matches_rational_arithmetic():
    rng = np.random.default_rng(2026)
    pa, pb, pc = planted_cases(rng)
    ra, rb, rc = random_cases(rng, 100_000)
    a, b, c = np.concatenate([pa, ra]), np.concatenate([pb, rb]), np.concatenate([pc, rc])
    got = em.fma32(a, b, c)
    want = np.array([fma_exact(x, y, z) for x, y, z in zip(a, b, c)], F32)
    bad = np.flatnonzero(bits(got) != bits(want))
    assert bad.size == 0, [(a[i], b[i], c[i], got[i], want[i]) for i in bad[:5]]
    # the planted set really holds ties: numpy's fp32 (a*b)+c (two roundings) differs from the fma on some of them
    assert (bits((pa * pb) + pc) != bits(em.fma32(pa, pb, pc))).sum() > 50
    # ... and fp64 p + c rounded once more to fp32 (without the round-to-odd step) is wrong on some of them
    naive = (pa.astype(np.float64) * pb + pc).astype(F32)
    assert (bits(naive) != bits(em.fma32(pa, pb, pc))).sum() > 50


def test_ref_sq_dist_matches_rational_fma():
    """The vectorised distance equals the formula evaluated term by term with the rational fma."""
    rng = np.random.default_rng(5)
    x = (rng.uniform(60, 80, (7, 3)) * rng.choice([-1, 1], (7, 3))).astype(F32)
    y = (x[rng.integers(0, 7, 40)] + rng.integers(-3, 4, (40, 3)) * 1e-3).astype(F32)
    d = em.ref_sq_dist(x, y)
    for i in range(7):
        xn = (x[i, 0] * x[i, 0] + x[i, 1] * x[i, 1]) + x[i, 2] * x[i, 2]
        for j in range(40):
            xy = fma_exact(x[i, 2], y[j, 2], fma_exact(x[i, 1], y[j, 1], x[i, 0] * y[j, 0]))
            yn = (y[j, 0] * y[j, 0] + y[j, 1] * y[j, 1]) + y[j, 2] * y[j, 2]
            want = max((xn - F32(2) * xy) + yn, F32(1e-12))
            assert bits(d[i, j]) == bits(want)
    assert (d == F32(1e-12)).any()  # the clamp is reached at these coordinates


def test_nms_restatement():
    # a path 0-1-2-3-4 keeps the even nodes; the lower-link property check agrees
    idx = np.array([[0, 1, 5], [0, 1, 2], [1, 2, 3], [2, 3, 4], [3, 4, 5]])
    keep = em.nms(idx)
    assert keep.tolist() == [True, False, True, False, True]
    assert em.nms_lower_links_ok(idx, keep) == (True, True)
    assert em.nms_lower_links_ok(idx, ~keep) == (True, False)     # 1 and 3 are independent, 0 is dropped for nothing
    assert em.nms_lower_links_ok(idx, np.ones(5, bool)) == (False, True)
    assert em.nms(idx, width=0).all()              # no column read: every node is kept
    star = np.array([[0, 5], [1, 0], [2, 0], [3, 0], [4, 0]])  # every node links node 0 in its second column
    assert em.nms(star).tolist() == [True, False, False, False, False]
    assert em.nms(star, width=1).all()             # column 0 (the node itself) only


def test_point_to_node_restatement_tie_rules():
    nodes = np.array([[1, 0, 0], [-1, 0, 0], [5, 5, 5]], F32)
    pts = np.array([[0, 1, 0], [0, 0, 2], [1, 0, 0], [1, 0, 0], [-0.5, 0, 0], [0, 0, 0]], F32)
    nm, knn, km, status, counts = em.point_to_node(pts, nodes, 4)
    # points on the bisector go to node 0 (first minimum); equal distances sort by point index
    assert counts.tolist() == [5, 1, 0] and nm.tolist() == [1, 1, 0] and status == 0
    assert knn[0].tolist() == [2, 3, 5, 0] and km[0].tolist() == [1, 1, 1, 1]
    assert knn[1].tolist() == [4, 6, 6, 6] and km[1].tolist() == [1, 0, 0, 0]
    assert knn[2].tolist() == [6] * 4 and km[2].tolist() == [0] * 4


def test_coarse_topk_restatement():
    s = np.array([[0.5, -1, 0.7], [0.7, 0.5, -1]], F32)
    r, c, v = em.topk(s, 10)
    assert list(zip(r.tolist(), c.tolist())) == [(0, 2), (1, 0), (0, 0), (1, 1)] and v.tolist() == [s[0, 2], s[1, 0], 0.5, 0.5]
    f = np.eye(3, dtype=F32)
    s64 = em.coarse_scores64(f, f, np.array([1, 0, 1]), np.array([1, 1, 1]), dual=False)
    assert (s64[1] == -1).all() and np.isclose(s64[0, 0], np.exp(-1e-12)) and np.isclose(s64[0, 1], np.exp(-2))
