"""GPU parity of the index kernels of matching.hip -- NMS (a10), the point-to-node partition (a11) and the superpoint
matching with its global top-k (a12) -- called through rdmnet_amd.ops, against the exact CPU restatements of
tests/exact_matching.py, on inputs chosen to break them: long dependency chains, the width cap, padded strides, exact
ties and duplicates, cancelling 60-80 m coordinates, the 4096-point patch capacity, every documented size limit and the
sizes past 64 KB of dynamic LDS.  Index outputs are compared bit for bit; the one tolerance of each float comparison is
derived next to its assert."""
import functools

import numpy as np
import pytest
import torch

import exact_matching as em

pytestmark = pytest.mark.gpu

F32 = np.float32
U32 = 2.0 ** -24   # fp32 unit roundoff
U64 = 2.0 ** -53   # fp64 unit roundoff


def gamma(n, u):
    """The classical bound of n roundings: n u / (1 - n u)."""
    return n * u / (1 - n * u)


@pytest.fixture(scope='module')
def ops():
    from rdmnet_amd import ops
    return ops


# --------------------------------------------------------------------------------------------------------------- NMS
def table_from_edges(n, edges, h):
    """Symmetric neighbour table [n, h] of an undirected edge list, the node itself in column 0 (as the radius search
    lists it), then its neighbours in ascending order; rows padded with n, truncated at h."""
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    e = e[e[:, 0] != e[:, 1]]
    src = np.concatenate([np.arange(n), e[:, 0], e[:, 1]])
    dst = np.concatenate([np.arange(n), e[:, 1], e[:, 0]])
    key = np.unique(src * (n + 2) + np.where(src == dst, 0, dst + 1))  # the node itself sorts first in its row
    src, col = key // (n + 2), key % (n + 2)
    dst = np.where(col == 0, src, col - 1)
    start = np.searchsorted(src, np.arange(n))
    rank = np.arange(src.size) - start[src]
    t = np.full((n, h), n, np.int64)
    keep = rank < h
    t[src[keep], rank[keep]] = dst[keep]
    return t


def radius_graph(rng, n, radius, h=60):
    """Points in clusters of varying density, linked within `radius` (degree 1 .. h with the node itself)."""
    centers = rng.uniform(0, 40, (max(1, n // 200), 3))
    pts = centers[rng.integers(0, len(centers), n)] + rng.normal(0, 1, (n, 3)) * rng.uniform(0.3, 3, (n, 1))
    edges = []
    for i0 in range(0, n, 1024):
        d = ((pts[i0:i0 + 1024, None, :] - pts[None, :, :]) ** 2).sum(-1)
        a, b = np.nonzero(d < radius * radius)
        edges.append(np.stack([a + i0, b], 1))
    return table_from_edges(n, np.concatenate(edges), h)


def run_nms(ops, table, width=None, extra=0, poison=None):
    """The kernel on `table` ([n, h]), held in a buffer of row stride h + extra whose columns past h (and past `width`)
    hold `poison`; width (int) goes in as the device word.  Returns keep (bool)."""
    n, h = table.shape
    buf = np.full((max(n, 1), h + extra), n if poison is None else poison, np.int64)
    buf[:n, :h] = table
    if width is not None and poison is not None:
        buf[:n, width:h] = poison
    dev = torch.from_numpy(buf).cuda()[:n, :h]
    assert dev.stride(0) == h + extra
    w = None if width is None else torch.tensor([width], dtype=torch.int32, device='cuda')
    return ops.nms(dev, w).cpu().numpy().astype(bool), buf[:n, :h]


def assert_nms(ops, table, **kw):
    keep, given = run_nms(ops, table, **kw)
    want = em.nms(given, kw.get('width'))
    assert keep.shape == want.shape and np.array_equal(keep, want), f'{int((keep != want).sum())} nodes differ'
    assert em.nms_lower_links_ok(given, keep, kw.get('width')) == (True, True)
    return keep


@pytest.mark.parametrize('n,radius', [(1000, 0.4), (3000, 1.0), (3000, 2.5)])
def test_nms_radius_graphs(ops, n, radius):
    rng = np.random.default_rng(n + int(radius * 10))
    t = radius_graph(rng, n, radius)
    deg = (t < n).sum(1)
    assert deg.min() == 1 or radius > 1  # isolated nodes at the small radius, full rows at the large one
    keep = assert_nms(ops, t)
    assert 0 < keep.sum() < n


def test_nms_two_clouds_stacked(ops):
    """The engine's table: both clouds' nodes stacked, each linked within its own cloud, one shadow index n_ref + n_src."""
    rng = np.random.default_rng(3)
    a, b = radius_graph(rng, 1500, 1.2, 40), radius_graph(rng, 900, 1.2, 40)
    n = 2400
    t = np.full((n, 40), n, np.int64)
    t[:1500] = np.where(a < 1500, a, n)
    t[1500:] = np.where(b < 900, b + 1500, n)
    assert_nms(ops, t)


@pytest.mark.parametrize('kind', ['ascending', 'descending', 'lower_only', 'upper_only'])
def test_nms_chains(ops, kind):
    """A path of 20 000 nodes in index order: every node depends on the one before it, the longest dependency chain
    (one link resolved per round).  Columns in ascending or descending order; or only the lower (upper) link listed."""
    n = 20000
    i = np.arange(n)
    lo, hi = np.where(i > 0, i - 1, n), np.where(i < n - 1, i + 1, n)
    t = {'ascending': np.stack([lo, i, hi], 1), 'descending': np.stack([hi, i, lo], 1),
         'lower_only': lo[:, None], 'upper_only': hi[:, None]}[kind]
    keep = assert_nms(ops, t)
    assert keep.sum() == (n if kind == 'upper_only' else n // 2)


def test_nms_cliques_stars_isolated(ops):
    n, h = 0, 60
    edges = []
    for size in (60, 7, 2):                               # cliques: only the lowest index survives
        edges += [(n + a, n + b) for a in range(size) for b in range(size)]
        n += size
    for centre, leaves in ((0, 50), (25, 50), (50, 50)):  # stars whose centre sits first, inside, last among its leaves
        ids = n + np.arange(leaves + 1)
        edges += [(ids[centre], x) for x in ids if x != ids[centre]]
        n += leaves + 1
    n += 40                                               # isolated nodes
    t = table_from_edges(n, edges, h)
    keep = assert_nms(ops, t)
    assert keep[-40:].all()


@pytest.mark.parametrize('width', [0, 1, 3, 7])
def test_nms_width_cap_and_stride(ops, width):
    """Columns at and past the device width hold index 0 -- node 0 is always kept, so any read of them would suppress
    the node -- and so does the padding of a row stride larger than h."""
    rng = np.random.default_rng(width)
    n = 4000
    t = table_from_edges(n, rng.integers(0, n, (4 * n, 2)), 12)
    keep = assert_nms(ops, t, width=width, extra=5, poison=0)
    if width <= 1:
        assert keep.all()


def test_nms_stride_larger_than_h(ops):
    rng = np.random.default_rng(9)
    n = 3000
    assert_nms(ops, table_from_edges(n, rng.integers(0, n, (3 * n, 2)), 9), extra=7, poison=0)


def test_nms_single_and_empty(ops):
    assert run_nms(ops, np.array([[0]]))[0].tolist() == [True]
    assert run_nms(ops, np.array([[1, 1]]))[0].tolist() == [True]
    keep = ops.nms(torch.empty((0, 8), dtype=torch.int64, device='cuda'), None)  # returns before any launch
    assert keep.numel() == 0


@pytest.mark.parametrize('n', [65000, 70000, 150000])
def test_nms_large(ops, n):
    """Sparse random graphs up to the documented limit: n bytes of LDS state, past 64 KB from 65 537 nodes on."""
    rng = np.random.default_rng(n)
    near = rng.integers(0, n, 2 * n)
    edges = np.stack([near, np.clip(near + rng.integers(-40, 40, 2 * n), 0, n - 1)], 1)
    assert_nms(ops, table_from_edges(n, edges, 8))


def test_nms_over_the_limit_raises(ops):
    idx = torch.zeros((150001, 1), dtype=torch.int64, device='cuda')
    with pytest.raises(RuntimeError, match='150000'):
        ops.nms(idx, None)


# ------------------------------------------------------------------------------------------------------ point-to-node
def p2n_compare(got, want, status, where=''):
    """got: (node_mask, knn, knn_mask) device tensors; want: em.point_to_node's result.  Rows of nodes owning more than
    4096 points are unspecified (only the status flag is) and are skipped."""
    nm, knn, km = (t.cpu().numpy() for t in got)
    w_nm, w_knn, w_km, w_status, counts = want
    ok = counts <= 4096
    assert np.array_equal(nm, w_nm), f'{where} node_mask'
    assert np.array_equal(knn[ok], w_knn[ok]), f'{where} knn_idx: {int((knn[ok] != w_knn[ok]).any(1).sum())} rows differ'
    assert np.array_equal(km[ok], w_km[ok]), f'{where} knn_mask'
    assert int(status) == w_status, f'{where} status'


@functools.lru_cache(maxsize=None)
def cloud(kind, n, m, seed=0):
    """Synthetic (points, nodes), fp32."""
    rng = np.random.default_rng(seed)
    if kind == 'random':       # nodes near a subset of the points, a few far away (they own nothing)
        pts = rng.uniform(-20, 20, (n, 3))
        nodes = pts[rng.permutation(n)[:m]] + rng.normal(0, 0.05, (m, 3))
        nodes[rng.permutation(m)[:max(1, m // 50)]] += 500
    elif kind == 'duplicates':  # every point three times: equal distances, ordered by index
        base = rng.uniform(-5, 5, (n // 3, 3))
        pts = np.concatenate([base, base, base])[rng.permutation(3 * (n // 3))]
        nodes = base[:m] + 0.01
    elif kind == 'equidistant':  # mirrored node pairs c +- e, points on the bisecting plane through c (exact in fp32)
        c = np.array([[0, 0, 0], [20, 0, 0], [0, 20, 0], [0, 0, 20]], np.float64)
        e = np.eye(3)[[0, 1, 2, 0]]
        sign = np.array([1, -1, 1, -1])[:, None]  # which of the pair comes first alternates
        nodes = np.concatenate([np.stack([c + sign * e, c - sign * e], 1).reshape(8, 3), [[0, 0, -100]]])[:m]
        g = rng.integers(0, 4, n)
        q = rng.integers(-8, 9, (n, 3)) * 0.25
        q[e[g] == 1] = 0
        pts = c[g] + q
    elif kind == 'far':          # 60-80 m from the origin at millimetre spacing: the formula cancels and clamps
        c = np.array([70.0, -65.0, 1.5])
        pts = c + rng.integers(-40, 40, (n, 3)) * 1e-3
        nodes = c + rng.integers(-40, 40, (m, 3)) * 1e-3
    return pts.astype(F32), nodes.astype(F32)


@functools.lru_cache(maxsize=None)
def cloud_parts(kind, n, m, seed=0):
    """em.partition of cloud(...), computed once per cloud (the distance matrix dominates the restatement's cost)."""
    return em.partition(*cloud(kind, n, m, seed))


def ref_p2n(key, k):
    return em.point_to_node(*cloud(*key), k, parts=cloud_parts(*key))


def run_p2n(ops, key, k):
    pts, nodes = cloud(*key)
    status = torch.zeros(1, dtype=torch.int32, device='cuda')
    got = ops.point_to_node(torch.from_numpy(pts).cuda(), torch.from_numpy(nodes).cuda(), k, status)
    want = ref_p2n(key, k)
    p2n_compare(got, want, status)
    return want


@pytest.mark.parametrize('k', [1, 64, 128, 200])
@pytest.mark.parametrize('kind', ['random', 'duplicates', 'equidistant', 'far'])
def test_point_to_node(ops, kind, k):
    n, m = {'random': (3000, 200), 'duplicates': (3000, 150), 'equidistant': (2000, 9), 'far': (3000, 300)}[kind]
    pts, nodes = cloud(kind, n, m)
    nm, knn, km, status, counts = run_p2n(ops, (kind, n, m), k)
    assert status == 0
    if kind == 'random':
        assert (counts == 0).any()                              # nodes that own no point: row n, mask 0
    if kind == 'equidistant':
        d = em.ref_sq_dist(nodes, pts)
        assert ((d == d.min(0)).sum(0) == 2).all()                # every point ties between the nodes of its pair ...
        assert (counts[1::2] == 0).all() and counts[:8:2].all()   # ... and goes to the lower index
    if kind == 'far':
        assert (em.ref_sq_dist(nodes, pts) == F32(1e-12)).any()   # clamped: the index decides


@pytest.mark.parametrize('n,m,k', [(1, 1, 64), (500, 1, 64), (50, 4, 128), (7, 7, 1), (300, 40, 200)])
def test_point_to_node_small(ops, n, m, k):
    run_p2n(ops, ('random', n, m, n + m), k)


@pytest.mark.parametrize('owned', [4096, 4097])
def test_point_to_node_capacity(ops, owned):
    """A node owning exactly 4096 points: flag clear, row exact; 4097: flag set, every other row still exact."""
    rng = np.random.default_rng(owned)
    crowd = rng.uniform(-1, 1, (owned, 3))
    rest = rng.uniform(-20, 20, (3000, 3)) + 40
    pts = np.concatenate([rest[:1000], crowd, rest[1000:]]).astype(F32)
    nodes = np.concatenate([[[0, 0, 0]], rest[rng.permutation(3000)[:100]] + 0.01]).astype(F32)
    want = em.point_to_node(pts, nodes, 128)
    assert want[4][0] == owned and want[4][1:].max() <= 4096
    status = torch.zeros(1, dtype=torch.int32, device='cuda')
    p2n_compare(ops.point_to_node(torch.from_numpy(pts).cuda(), torch.from_numpy(nodes).cuda(), 128, status), want, status)
    assert int(status) == (owned > 4096)


@pytest.mark.parametrize('m', [4096, 4097, 8192])
def test_point_to_node_many_nodes(ops, m):
    """16 m bytes of dynamic LDS: 64 KB at 4096 nodes, past it at 4097 and 8192 (the limit)."""
    run_p2n(ops, ('random', m + 1500, m, m), 64)


def test_point_to_node_over_the_limit_raises(ops):
    pts, nodes = cloud('random', 9000, 8193, seed=1)
    status = torch.zeros(1, dtype=torch.int32, device='cuda')
    with pytest.raises(RuntimeError, match='bad sizes'):
        ops.point_to_node(torch.from_numpy(pts).cuda(), torch.from_numpy(nodes).cuda(), 64, status)
    with pytest.raises(RuntimeError, match='bad sizes'):
        ops.point_to_node_pair(torch.from_numpy(pts[:100]).cuda(), torch.from_numpy(nodes[:10]).cuda(),
                               torch.from_numpy(pts).cuda(), torch.from_numpy(nodes).cuda(), 64, status)


@pytest.mark.parametrize('a,b,k', [(('random', 3000, 200, 0), ('far', 5000, 300, 0), 128),
                                   (('duplicates', 2400, 100, 0), ('random', 8192 + 1500, 8192, 8192), 64),
                                   (('random', 8192 + 1500, 8192, 8192), ('equidistant', 900, 9, 0), 200)])
def test_point_to_node_pair(ops, a, b, k):
    """The pair form against the restatement itself, m_a != m_b and n_a != n_b, one side at 8192 nodes."""
    (pa, na), (pb, nb) = cloud(*a), cloud(*b)
    status = torch.zeros(1, dtype=torch.int32, device='cuda')
    ga, gb = ops.point_to_node_pair(*(torch.from_numpy(x).cuda() for x in (pa, na, pb, nb)), k, status)
    wa, wb = ref_p2n(a, k), ref_p2n(b, k)
    p2n_compare(ga, wa, status, 'a:')
    p2n_compare(gb, wb, status, 'b:')


# ---------------------------------------------------------------------------------------------- coarse matching (fp64)
def unit_rows(rng, m, d, dup=0):
    f = rng.normal(size=(m, d))
    if dup and m > 1:  # planted duplicate rows: exactly tied scores
        src = rng.integers(0, m, dup)
        f[rng.integers(0, m, dup)] = f[src]
    return (f / np.linalg.norm(f, axis=1, keepdims=True)).astype(F32)


def features(rng, m, n, d, dup):
    """ref rows and src rows that are noisy copies of ref rows (high scores exist), both L2-normalised in fp32."""
    r = unit_rows(rng, m, d, dup)
    s = r[rng.integers(0, m, n)].astype(np.float64) + 0.4 * rng.normal(size=(n, d)) / np.sqrt(d)
    if dup and n > 1:
        s[rng.integers(0, n, dup)] = s[rng.integers(0, n, dup)]
    if d == 1:
        s = np.sign(s) + (s == 0)
    return r, (s / np.linalg.norm(s, axis=1, keepdims=True)).astype(F32)


def make_mask(rng, size, kind):
    if kind == 'all':
        return np.ones(size, np.uint8)
    if kind == 'none':
        return np.zeros(size, np.uint8)
    mk = (rng.uniform(size=size) < 0.8).astype(np.uint8)
    mk[rng.integers(0, size)] = 1
    return mk


def strided_rows(f, extra, fill):
    """[m, d] -> device view with row stride pad4(d) + extra, the bytes past d holding `fill`."""
    m, d = f.shape
    ld = (d + 3) // 4 * 4 + extra
    buf = torch.full((m, ld), fill, dtype=torch.float32)
    buf[:, :d] = torch.from_numpy(f)
    return buf.cuda()[:, :d]


def fp64_bound(d, m, n, dual):
    """Relative distance between two fp64 evaluations of one score that sum in different orders (the kernel's and
    the restatement's), first order in U64:
      * a dot product of d terms with |a| = |b| = 1 (fp32-normalised: <= 1 + 1e-6): each evaluation is within
        gamma_d |a||b| of the exact value -> 2 gamma_d (1 + 1e-6)^2 apart;
      * 2 - 2 xy: doubled, plus one rounding of a value <= 4 in each -> absolute 2 * that + 8 U64;
      * exp: a relative change equal to the absolute change of its argument, plus 2 ulp (4 U64) in each of the two
        exp implementations -> dx = the line above + 8 U64;
      * dual: row / column sums of positive terms carry dx plus gamma_n / gamma_m in each evaluation, the two
        quotients and the product one rounding each in each -> 4 dx + 2 gamma_n + 2 gamma_m + 6 U64."""
    dx = 4 * gamma(d, U64) * (1 + 1e-6) ** 2 + 8 * U64 + 8 * U64
    b = 4 * dx + 2 * gamma(n, U64) + 2 * gamma(m, U64) + 6 * U64 if dual else dx
    return b * 1.01  # second-order terms


OBSERVED = {}


def note(key, value):
    OBSERVED[key] = max(OBSERVED.get(key, 0.0), float(value))
    print(f'matching-observed {key} = {OBSERVED[key]:.3g}')


FP64_CASES = [
    # m,    n,    d,   k,    dual,  masks (ref, src), ld extra, planted duplicates
    (1, 1, 1, 1, True, ('all', 'all'), 0, 0),
    (1, 17, 100, 1024, True, ('all', 'random'), 3, 0),
    (17, 1, 448, 1, False, ('random', 'all'), 0, 0),
    (17, 17, 256, 1024, True, ('random', 'random'), 0, 4),     # k > valid pairs
    (17, 333, 100, 256, True, ('random', 'random'), 5, 8),
    (333, 17, 448, 1024, False, ('random', 'all'), 1, 8),
    (333, 333, 256, 256, True, ('random', 'random'), 0, 30),
    (333, 333, 1, 1024, True, ('random', 'random'), 0, 0),     # d = 1: scores take two values before normalisation
    (333, 333, 1, 256, False, ('all', 'random'), 2, 0),
    (1000, 333, 100, 1, True, ('random', 'random'), 0, 20),
    (333, 1000, 448, 1024, True, ('random', 'random'), 4, 40),
    (1000, 1000, 256, 1024, True, ('random', 'random'), 0, 50),
    (1000, 1000, 448, 256, False, ('random', 'random'), 0, 50),
    (1000, 1000, 256, 1024, False, ('all', 'all'), 0, 0),
    (17, 333, 256, 256, True, ('none', 'random'), 0, 0),       # a fully masked side: count 0
    (333, 17, 100, 64, False, ('random', 'none'), 0, 0),
]


@pytest.mark.parametrize('m,n,d,k,dual,masks,extra,dup', FP64_CASES)
def test_coarse_matching_features(ops, m, n, d, k, dual, masks, extra, dup):
    """rdm_coarse_matching_features == the fp64 restatement rounded to fp32, then its top-k, bit for bit.  The one
    exception is computed, not assumed: a score whose fp64 value lies within fp64_bound (relative) of an fp32 rounding
    boundary may round to either neighbour in the kernel; the result must then be the exact top-k of a matrix whose
    entries all take one of their allowed fp32 values."""
    rng = np.random.default_rng(m * 7 + n * 3 + d + k + dual)
    fr, fs = features(rng, m, n, d, dup)
    rm, cm = make_mask(rng, m, masks[0]), make_mask(rng, n, masks[1])
    poison = 3.0  # in the row padding: read, it changes every score
    ri, si, sc, cnt = ops.coarse_matching_features(strided_rows(fr, extra, poison), strided_rows(fs, extra, poison),
                                                   torch.from_numpy(rm).cuda(), torch.from_numpy(cm).cuda(), k, dual)
    c = int(cnt)
    valid = int(rm.sum()) * int(cm.sum())
    assert c == min(k, valid)
    ri, si, sc = ri.cpu().numpy()[:c], si.cpu().numpy()[:c], sc.cpu().numpy()[:c]
    s64 = em.coarse_scores64(fr, fs, rm, cm, dual)
    b = fp64_bound(d, m, n, dual)
    lo = np.where(s64 >= 0, (s64 * (1 - b)).astype(F32), F32(-1))
    hi = np.where(s64 >= 0, (s64 * (1 + b)).astype(F32), F32(-1))
    assert (lo <= s64.astype(F32)).all() and (s64.astype(F32) <= hi).all()
    got_ok = (sc == lo[ri, si]) | (sc == hi[ri, si])
    assert got_ok.all(), f'{int((~got_ok).sum())} scores off their allowed fp32 values'
    allowed = lo.copy()
    allowed[ri, si] = sc
    wr, wc, wv = em.topk(allowed, k)
    assert np.array_equal(ri, wr) and np.array_equal(si, wc) and np.array_equal(sc, wv)
    # observed: entries within the bound of a boundary, and how many of the returned ones the kernel rounded the other way
    if c:
        note('fp64 path: returned scores rounded across a boundary', int((sc != s64[ri, si].astype(F32)).sum()))
        note('fp64 path: entries within the bound of a boundary (per case)', int((lo != hi).sum()))
    note('fp64 path: derived bound (relative)', b)


def test_coarse_matching_features_width_limit(ops):
    rng = np.random.default_rng(0)
    f = unit_rows(rng, 4, 449)
    mk = torch.ones(4, dtype=torch.uint8, device='cuda')
    with pytest.raises(RuntimeError, match='bad sizes'):
        ops.coarse_matching_features(strided_rows(f, 0, 0), strided_rows(f, 0, 0), mk, mk, 8)


# ------------------------------------------------------------------------------------- coarse matching (fp32, dual)
def fp32_dual_bound(m, n):
    """Relative error of the fp32 path's score against the fp64 formula on the same fp32 GEMM output, first order in U32:
      * 2 - 2 s: one rounding of a value <= 4 -> absolute 4 U32, a relative 4 U32 after exp; expf itself <= 2 ulp
        (4 U32) -> dx = 8 U32 per score;
      * the row sum adds n positive terms (any order: gamma_n), the column sum m terms in sequence (gamma_m), each also
        carrying dx;
      * two divisions (correctly rounded) and the product -> 3 U32:
        B = 4 dx + gamma_n + gamma_m + 3 U32."""
    dx = 8 * U32
    return (4 * dx + gamma(n, U32) + gamma(m, U32) + 3 * U32) * 1.01


@pytest.mark.parametrize('m,n,d,k', [(17, 333, 100, 256), (333, 333, 256, 256), (333, 1000, 256, 1024),
                                     (1000, 1000, 448, 1024), (1000, 17, 256, 1)])
def test_coarse_matching_fp32_dual(ops, m, n, d, k):
    """rdm_coarse_matching (dual) on the fp32 GEMM of unit-norm features against the fp64 formula on that GEMM output:
    each returned score within B of its fp64 value, a pair missing or extra only within 2B of the k-th fp64 score,
    and position by position the fp64 scores within 2B (order differs only inside groups tied to 2B)."""
    rng = np.random.default_rng(m + n + k)
    fr, fs = features(rng, m, n, d, dup=0)
    rm, cm = make_mask(rng, m, 'random'), make_mask(rng, n, 'random')
    sim = ops.gemm(torch.from_numpy(fr).cuda(), torch.from_numpy(fs).cuda(), d, n, trans_b=True)
    sim_in = sim.cpu().numpy().copy()
    ri, si, sc, cnt = ops.coarse_matching(sim, torch.from_numpy(rm).cuda(), torch.from_numpy(cm).cuda(), k, dual=True)
    left = sim.cpu().numpy()
    c = int(cnt)
    assert c == min(k, int(rm.sum()) * int(cm.sum()))
    # -1 exactly at the masked entries, and nowhere else
    masked = (rm[:, None] == 0) | (cm[None, :] == 0)
    assert (left[masked] == -1).all() and (left[~masked] > 0).all()
    s64 = em.coarse_scores64(None, None, rm, cm, dual=True, sim=sim_in)
    flat = s64.reshape(-1)
    elig = np.flatnonzero(flat >= 0)
    want = elig[np.lexsort((elig, -flat[elig]))][:c]
    got = ri.cpu().numpy()[:c] * n + si.cpu().numpy()[:c]
    sc = sc.cpu().numpy()[:c].astype(np.float64)
    B = fp32_dual_bound(m, n)
    err = np.abs(sc - flat[got]) / flat[got]
    assert err.max() <= B, f'score error {err.max():.3g} > {B:.3g}'
    t = flat[want[-1]]
    moved = np.setxor1d(got, want)
    gap = np.abs(flat[moved] - t) / t if moved.size else np.zeros(1)
    assert gap.max() <= 2 * B, f'a pair crossed the cut {gap.max():.3g} from the k-th score (> {2 * B:.3g})'
    pos = np.abs(flat[got] - flat[want]) / flat[want]
    assert pos.max() <= 2 * B, f'positions differ across a score gap of {pos.max():.3g} (> {2 * B:.3g})'
    note('fp32 dual: score error / B', err.max() / B)
    note('fp32 dual: pairs swapped at the cut', moved.size)
    note('fp32 dual: positional gap / 2B', pos.max() / (2 * B))


# -------------------------------------------------------------------------------------------------- top-k edges
def topk_check(ops, sim, rm, cm, k):
    s = torch.from_numpy(sim).cuda()
    ri, si, sc, cnt = ops.coarse_matching(s, torch.from_numpy(rm).cuda(), torch.from_numpy(cm).cuda(), k, dual=False)
    v = s.cpu().numpy()
    wr, wc, wv = em.topk(v, k)
    c = int(cnt)
    assert c == wr.size == min(k, int(rm.sum()) * int(cm.sum()))
    assert np.array_equal(ri.cpu().numpy()[:c], wr) and np.array_equal(si.cpu().numpy()[:c], wc)
    assert np.array_equal(sc.cpu().numpy()[:c].view(np.uint32), wv.view(np.uint32))
    masked = (rm[:, None] == 0) | (cm[None, :] == 0)
    assert (v[masked] == -1).all() and (v[~masked] >= 0).all()
    return v, wr * sim.shape[1] + wc


@pytest.mark.parametrize('m,n,k', [(333, 333, 1024), (333, 333, 1), (2000, 1500, 256), (2000, 1500, 1024),
                                   (3, 5, 64), (1, 1, 1024)])
def test_topk_edges(ops, m, n, k):
    rng = np.random.default_rng(m * n + k)
    sim = rng.uniform(-1, 1, (m, n)).astype(F32)
    sim[rng.integers(0, m, 50), rng.integers(0, n, 50)] = sim.max()  # exact ties at the top
    topk_check(ops, sim, make_mask(rng, m, 'random'), make_mask(rng, n, 'random'), k)


@pytest.mark.parametrize('m,n', [(60, 60), (100, 100), (333, 333)])
def test_topk_all_scores_equal(ops, m, n):
    """Every eligible score identical: one histogram bin, the candidate list overflows, the single-workgroup fallback
    runs (with up to 4096 equal entries listed, past that the ordered scan): the first k eligible flat indices."""
    rng = np.random.default_rng(m)
    rm, cm = make_mask(rng, m, 'random'), make_mask(rng, n, 'random')
    _, got = topk_check(ops, np.full((m, n), 0.25, F32), rm, cm, 1024)
    elig = np.flatnonzero((rm[:, None] * cm[None, :]).reshape(-1))
    assert np.array_equal(got, elig[:1024])
