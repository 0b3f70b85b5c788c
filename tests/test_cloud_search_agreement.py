"""The three cloud searches share one cell index (rdmnet_amd/csrc/cell_index.h): on the same clouds they must give one answer.
With (j, d2) = the exact nearest neighbour (ops._nearest),
  ops.icp_correspondences returns (j, d2) where d2 < r2 and (-1, -1.0) elsewhere (open ball),
  ops._ball_count's min_d2 is d2 where d2 <= r2 and -1.0 elsewhere (closed ball),
at r = 0.5, whose square is exact in fp32, so ICP's float-rounded r2 and the ball query's double r2 coincide.

The expectation comes from tests/nearest_restatement.py (blocked brute force in float64).  The CPU half checks that
tests/icp_restatement.py and tests/pair_overlap_restatement.py agree with it on these inputs, and that every input really holds
the edge it was built for; the GPU half compares every query row of the three kernels with it, bit for bit.

Inputs are on the 2^-6 grid where a tie or d2 == r2 is planted (differences, squares and their sums are then exact), and sit
where the shared lookup can go wrong: cell-edge multiples, queries outside the box by less than, exactly and more than a cell on
every axis and side, a flat box (dims[2] == 1), a single cell, a column of 65 records (one more than a wavefront walks at once)."""
import functools

import numpy as np
import pytest
import torch

import icp_restatement
import nearest_restatement
import pair_overlap_restatement
from rdmnet_amd import ops

R = 0.5
R2 = 0.25                  # exact in fp32 and in double
H = R * (1.0 + 1e-6)       # the cell edge of both radius searches
FAR = np.float32(10.0)     # where the isolated support row of the d2 == r2 pair sits

# name: (support rows, layout)
CASES = {
    'one_point': (1, 'single'),
    'box_63': (63, 'box'),
    'flat_64': (64, 'flat'),
    'one_cell_65': (65, 'single'),
    'column_257': (257, 'column'),
}


def grid(rng, n, lo, hi):
    """n points with coordinates on the 2^-6 grid in [lo, hi)"""
    return (rng.integers(int(lo * 64), int(hi * 64), size=(n, 3)) / 64.0).astype(np.float32)


def support(name):
    """-> (s float32 [m, 3], planted: the rows of the tie pair (or None) and the row of the d2 == r2 pair)"""
    m, layout = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name) + 1)
    if layout == 'single':  # every row in the cell [0, h)^3; the row with the largest x is alone there
        s = grid(rng, m, 0.03125, 0.40625)
        edge = m - 1 if m == 1 else m // 2
        s[edge] = (0.46875, 0.25, 0.25)
    else:
        s = grid(rng, m, 0.0, 2.0)
        if layout == 'flat':
            s[:, 2] = 0.75
        if layout == 'column':  # rows 100..164: one cell column (x, y), over three cells in z
            s[100:165, :2] = grid(rng, 65, 1.03125, 1.40625)[:, :2]
            s[100:165, 2] = grid(rng, 65, 0.0, 1.5)[:, 2]
        edge = 1
        s[edge] = (FAR, FAR, s[0, 2] if layout == 'flat' else FAR)
    tie = None
    if m > 1:  # rows 0 and m - 1 at one grid step on either side of a centre
        centre = np.array([0.25, 0.25, 0.25] if layout == 'single' else [1.0, 1.0, 0.75], np.float32)
        step = np.array([1.0 / 64.0, 0, 0], np.float32)
        s[0], s[m - 1] = centre + step, centre - step
        s[(s == centre).all(1)] += 2 * step  # (nothing at the centre itself)
        tie = (0, m - 1, centre)
    return s, tie, edge


def queries(s, tie, edge, rng):
    cells = np.floor(s.astype(np.float64) / H)
    lo, hi = cells.min(0), cells.max(0)
    box_lo, box_hi = lo * H, (hi + 1) * H
    out = [grid(rng, 84, box_lo.min() - 1.75, min(box_hi.max(), 2.5) + 1.75)]
    ks = rng.integers(-3, 8, size=(24, 3))
    out.append((ks * R).astype(np.float32))                  # multiples of r
    on_edge = (ks * H).astype(np.float32)                    # multiples of the cell edge, and the fp32 values next to them
    out += [on_edge, np.nextafter(on_edge, np.float32(-np.inf)), np.nextafter(on_edge, np.float32(np.inf))]
    inside = s[rng.integers(0, len(s), size=18)].astype(np.float64)
    k = 0
    for a in range(3):  # outside the box by less than a cell, by exactly a cell, by more than two cells
        for side in (-1, 1):
            for dist in (0.25 * H, H, 2.5 * H):
                inside[k, a] = box_lo[a] - dist if side < 0 else box_hi[a] + dist
                k += 1
    out.append(inside.astype(np.float32))
    out.append(s[edge][None] + np.array([[R, 0, 0]], np.float32))  # exactly r from its nearest row
    if tie is not None:
        out.append(tie[2][None])
    return np.concatenate(out).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(name):
    """The clouds of a case and the one answer, computed once."""
    s, tie, edge = support(name)
    q = queries(s, tie, edge, np.random.default_rng(100 + len(s)))
    d2, j = nearest_restatement.nearest(q, s)
    for x in (q, s, d2, j):
        x.setflags(write=False)
    return dict(q=q, s=s, tie=tie, edge=edge, d2=d2, j=j,
                icp_j=np.where(d2 < R2, j, -1), icp_d2=np.where(d2 < R2, d2, -1.0), ball_d2=np.where(d2 <= R2, d2, -1.0))


@pytest.mark.parametrize('name', sorted(CASES))
def test_inputs_hold_their_edges(name):
    c = case(name)
    q, s, d2, j = c['q'], c['s'], c['d2'], c['j']
    m, layout = CASES[name]
    assert s.shape == (m, 3) and 195 <= len(q) <= 205
    assert np.float64(np.float32(R * R)) == R2 == np.float64(R) * np.float64(R)
    cells = np.floor(s.astype(np.float64) / H).astype(np.int64)
    dims = cells.max(0) - cells.min(0) + 1
    if layout == 'single':
        assert (dims == 1).all()
    if layout == 'flat':
        assert dims[2] == 1 and dims[0] > 1 and dims[1] > 1
    if m >= 65:
        _, per_column = np.unique(cells[:, :2], axis=0, return_counts=True)
        assert per_column.max() >= 65
    # the last-but-one query (or the last without a tie) is exactly r from its nearest row: in for the ball, out for ICP
    e = len(q) - (2 if c['tie'] else 1)
    assert d2[e] == R2 and j[e] == c['edge'] and c['ball_d2'][e] == R2 and c['icp_j'][e] == -1
    if c['tie']:
        low, high, _ = c['tie']
        all_d2 = nearest_restatement.sq_dists(nearest_restatement.moved(q[-1:], None), nearest_restatement.moved(s, None))[0]
        assert all_d2[low] == all_d2[high] == d2[-1] and j[-1] == low and low < high
    # outside the box on every axis and side by less than one, exactly one and more than two cells
    qc = np.floor(q.astype(np.float64) / H).astype(np.int64)
    for a in range(3):
        below, above = cells[:, a].min() - qc[:, a], qc[:, a] - cells[:, a].max()
        for off in (below, above):
            assert (off == 1).any() and (off >= 3).any()
    # some rows are in, some out, for both rules
    if m > 1:
        assert (d2 < R2).any() and (d2 > R2).any()


@pytest.mark.parametrize('name', sorted(CASES))
def test_restatements_agree(name):
    c = case(name)
    idx, d2, _ = icp_restatement.Target(c['s'], R).correspondences(c['q'].astype(np.float64))
    assert np.array_equal(idx, c['icp_j']) and np.array_equal(d2, c['icp_d2'])
    ball = pair_overlap_restatement.ball_query(c['q'], c['s'], None, R)
    assert np.array_equal(ball['ref_min_d2'], c['d2'])
    assert np.array_equal(ball['counts'] > 0, c['d2'] <= R2)


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(CASES))
def test_three_searches_one_answer(name):
    c = case(name)
    q, s = torch.tensor(c['q']).cuda(), torch.tensor(c['s']).cuda()
    n = len(c['q'])
    j, d2, _ = ops._nearest(q, s)
    assert np.array_equal(j.cpu().numpy(), c['j']) and np.array_equal(d2.cpu().numpy(), c['d2'])
    icp_j, icp_d2 = ops.icp_correspondences(q.double(), s, R)
    assert np.array_equal(icp_j.cpu().numpy(), c['icp_j']), np.nonzero(icp_j.cpu().numpy() != c['icp_j'])[0][:8]
    assert np.array_equal(icp_d2.cpu().numpy(), c['icp_d2'])
    _, _, ball_d2, _, _ = ops._ball_count(q, s, None, R, 'radius', want_min=True)
    assert np.array_equal(ball_d2[:n].cpu().numpy(), c['ball_d2']), np.nonzero(ball_d2[:n].cpu().numpy() != c['ball_d2'])[0][:8]
