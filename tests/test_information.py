"""CPU: the float64 restatement of rdm_information_matrix (tests/information_restatement.py) -- the literal sum of g g^T against the
closed form the kernel uses, the structure of the matrix, the strict radius against the reference's compute_overlap as recorded in
tests/golden/nearest.npz -- the generators of tests/test_information_gpu.py (every row decided), and the library's exports."""
import os

import numpy as np
import pytest

import information_cases as cases
import information_restatement as I
from rdmnet_amd import _lib, ops

U = 2.0 ** -53


@pytest.fixture(scope='module')
def fx(golden_dir):
    z = np.load(os.path.join(golden_dir, 'nearest.npz'))
    return {k: z[k] for k in z.files}


@pytest.fixture(scope='module')
def pairs(golden_dir):
    z = np.load(os.path.join(golden_dir, 'synthetic_pairs.npz'))
    return {k: z[k] for k in z.files}


def test_closed_form_equals_the_row_form_and_the_matrix_has_its_structure():
    rng = np.random.default_rng(0)
    for n, scale, shift in ((0, 1.0, 0.0), (1, 1.0, 0.0), (37, 10.0, 0.0), (500, 10.0, 70.0)):
        p = rng.uniform(-scale, scale, size=(n, 3)) + shift
        info, magnitude = I.row_form(p)
        closed = I.closed_form(p)
        # both are correctly rounded sums of the same terms up to the closed form's own products and two additions
        assert (np.abs(info - closed) <= 4 * U * magnitude).all(), n
        assert np.array_equal(info, info.T) and np.array_equal(closed, closed.T)
        assert np.array_equal(info[3:, 3:], n * np.eye(3))
        sx, sy, sz = info[2, 4], info[0, 5], info[1, 3]  # [s]x above the diagonal blocks
        assert np.array_equal(info[:3, 3:], np.array([[0, -sz, sy], [sz, 0, -sx], [-sy, sx, 0]]) + 0.0)
        assert np.array_equal(info[3:, :3], info[:3, 3:].T)
        if n > 0:
            assert abs(sx - p[:, 0].sum()) <= 1e-12 * np.abs(p[:, 0]).sum()
            assert (np.linalg.eigvalsh(info) >= -1e-9 * info[0, 0]).all()  # a sum of g g^T
    one, _ = I.row_form([[1.0, 2.0, 3.0]])
    assert one.tolist() == [[13, -2, -3, 0, -3, 2], [-2, 10, -6, 3, 0, -1], [-3, -6, 5, -2, 1, 0],
                            [0, 3, -2, 1, 0, 0], [-3, 0, 1, 0, 1, 0], [2, -1, 0, 0, 0, 1]]
    assert np.array_equal(I.closed_form([[1.0, 2.0, 3.0]]), one)


def test_strict_radius_counts_the_rows_the_reference_calls_overlapping(fx, pairs):
    """Pair 0 under its ground-truth pose at 0.6 m, the direction the fixture stores (ref rows against the moved src cloud), every
    8th row (a row does not depend on the other rows)."""
    ref, src, T = pairs['ref0'], pairs['src0'], fx['p0/gt/est']
    got = I.information(ref[::8], src, 0.6, None, T)
    marked = fx['p0/gt/dist'][::8] < 0.6
    assert got['C'] == int(marked.sum()) and 0 < got['C'] < len(marked)
    assert np.array_equal(got['corr'][:, 0], np.nonzero(marked)[0])
    assert np.array_equal(got['corr'][:, 1], fx['p0/gt/idx'][::8][marked].astype(np.int64))
    assert round(float(fx['p0/gt/overlap0.6']) * len(ref)) == int((fx['p0/gt/dist'] < 0.6).sum())  # (compute_overlap's own count)
    info = got['information']
    assert np.array_equal(info, info.T) and np.array_equal(info[3:, 3:], got['C'] * np.eye(3))
    assert got['fitness'] == got['C'] / len(marked) and 0 < got['inlier_rmse'] < 0.6


@pytest.mark.parametrize('name', sorted(cases.CASES))
def test_every_row_of_the_generated_cases_is_decided(name):
    c = cases.CASES[name]()
    I.assert_decided(c['source'], c['target'], c['radius'], c.get('s_transform'), c.get('t_transform'),
                     c.get('boundary_rows', ()), c.get('tie_rows', ()))
    want = I.information(c['source'], c['target'], c['radius'], c.get('s_transform'), c.get('t_transform'))
    if 'expect_C' in c:
        assert want['C'] == c['expect_C'], name
    if len(c['source']) >= 63 and len(c['target']) >= 1025:
        assert 0 < want['C'] < len(c['source']), name  # the radius separates rows


def test_path_case_lies_inside_one_cell_and_beyond_the_small_cells_reach():
    c = cases.CASES[cases.PATH_CASE]()
    h = cases.PATH_CELLS['one_cell']
    for cloud in (c['source'], c['target']):  # cell 0 of the large edge holds both clouds: the cell search settles every row
        assert (np.floor(cloud.astype(np.float64) / h) == 0).all()
    d2, _ = I.R.nearest(c['source'], c['target'])
    assert np.sqrt(d2.min()) > 4 * cases.PATH_CELLS['sweep']  # beyond the cube of 5^3 small cells: nothing settles there
    assert (c['source'] != cases.cloud_pair(257, 1025, 13)['source']).any()  # (the clipping moved rows: some lay outside)


def test_boundary_and_tie_cases_are_what_they_claim():
    b = cases.boundary()
    q, s = I.R.moved(b['source'], None), I.R.moved(b['target'], None)
    d2 = I.R.sq_dists(q, s)
    r = b['radius']
    assert d2[0].min() == r * r and np.sqrt(d2[0].min()) == r  # exactly on the radius: excluded
    assert r - 1e-7 < np.sqrt(d2[1].min()) < r  # one float32 step of the coordinate nearer
    assert np.nextafter(r, 1.0) > np.sqrt(d2[0].min())  # (with the next double as the radius row 0 is inside: the GPU test asks)
    want = I.information(b['source'], b['target'], r)
    assert want['corr'][:, 0].tolist() == b['expect_rows']
    t = cases.tie()
    d2 = I.R.sq_dists(I.R.moved(t['source'], None), I.R.moved(t['target'], t['t_transform']))
    row = t['tie_rows'][0]
    lo, hi = t['tie_targets']
    assert d2[row, lo] == d2[row, hi] == d2[row].min() and lo < hi
    moved = I.R.moved(t['target'], t['t_transform'])
    assert not np.array_equal(moved[lo], moved[hi])
    want = I.information(t['source'], t['target'], t['radius'], None, t['t_transform'])
    assert [lo] == [j for i, j in want['corr'].tolist() if i == row]
    other = want['corr'].copy()
    other[other[:, 0] == row, 1] = hi
    assert not np.array_equal(I.row_form(moved[other[:, 1]])[0], want['information'])  # the matrix tells the two apart


def test_library_exports_and_result_arithmetic():
    L = _lib.lib()
    for name in ('rdm_information_workspace_bytes', 'rdm_information_matrix', 'rdm_engine_information_matrix'):
        assert hasattr(L, name) and name in _lib.SIGNATURES
    assert L.rdm_information_workspace_bytes(16000, 16000) > L.rdm_nearest_workspace_bytes(16000, 16000)
    assert L.rdm_information_workspace_bytes(0, 0) > 0
    host = [float(k) for k in range(36)] + [2.0, 0.5, 7.0, 0.0]
    info, c, sum_d2, swept, corr = ops.information_result(host, None)
    assert info.shape == (6, 6) and info.dtype.is_floating_point and info[1, 2] == 8.0 and (c, sum_d2, swept, corr) == (2, 0.5, 7, None)
    assert ops.INFORMATION_WIDTH == 40
    res = ops.RegistrationResult(np.eye(4), 0.5, 0.1, 3, 0)
    assert res.correspondence_set is None and res.history is None
