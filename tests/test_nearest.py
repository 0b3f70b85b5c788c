"""CPU: the float64 restatement of nearest.hip (tests/nearest_restatement.py) against the reference's recorded outputs
(tests/golden/nearest.npz), its tie rule, the library's exports and the arithmetic of the quality dict."""
import math
import os

import numpy as np
import pytest

import nearest_restatement as R
from rdmnet_amd import _lib, ops


@pytest.fixture(scope='module')
def fx(golden_dir):
    z = np.load(os.path.join(golden_dir, 'nearest.npz'))
    return {k: z[k] for k in z.files}


@pytest.fixture(scope='module')
def pairs(golden_dir):
    z = np.load(os.path.join(golden_dir, 'synthetic_pairs.npz'))
    return {k: z[k] for k in z.files}


def test_fixture_holds_what_the_tests_expect(fx):
    assert fx['pairs'].tolist() == [0, 3] and fx['radii'].tolist() == [0.3, 0.6]
    assert float(fx['closest_relative']) > 1e-9  # every stored row is decided
    for p in (0, 3):
        for name in ('gt', 'off'):
            assert fx[f'p{p}/{name}/dist'].dtype == np.float64 and fx[f'p{p}/{name}/idx'].dtype == np.int32
            assert fx[f'p{p}/{name}/dist'].shape == fx[f'p{p}/{name}/idx'].shape == (16000,)
        assert float(fx[f'p{p}/gt/rmse']) == 0.0 and float(fx[f'p{p}/off/rmse']) > 0.2
    assert 'scans/dist' not in fx and float(fx['scans/chamfer']) > 0


def test_restatement_equals_the_reference_rows(fx, pairs):
    """Every 8th row of every case (a row does not depend on the other rows): indices equal, distances within 1e-9 m."""
    for p in fx['pairs']:
        ref, src = pairs[f'ref{p}'], pairs[f'src{p}']
        for name in ('gt', 'off'):
            tag = f'p{p}/{name}'
            dist, idx = R.get_nearest_neighbor(ref[::8], src, True, s_transform=fx[f'{tag}/est'])
            assert np.array_equal(idx, fx[f'{tag}/idx'][::8].astype(np.int64)), tag
            assert np.abs(dist - fx[f'{tag}/dist'][::8]).max() <= 1e-9, tag


def test_restatement_equals_the_reference_scalars(fx, pairs):
    ref, src, tag = pairs['ref0'], pairs['src0'], 'p0/off'
    gt, est = fx[f'{tag}/gt'], fx[f'{tag}/est']
    for r in fx['radii']:
        assert R.compute_overlap(ref, src, est, float(r)) == float(fx[f'{tag}/overlap{r}'])
    assert abs(R.compute_registration_rmse(src, gt, est) - float(fx[f'{tag}/rmse'])) <= 1e-9
    assert abs(R.compute_registration_rmse(pairs['src3'], fx['p3/off/gt'], fx['p3/off/est']) - float(fx['p3/off/rmse'])) <= 1e-9
    assert abs(R.compute_modified_chamfer_distance(ref, ref, src, gt, est) - float(fx[f'{tag}/chamfer'])) <= 1e-9


def test_restatement_takes_the_lowest_index_among_equal_distances():
    s = np.float32([[1, 0, 0], [0, 1, 0], [1, 0, 0], [-1, 0, 0], [0, 1, 0]])
    d2, idx = R.nearest(np.float32([[0, 0, 0], [1, 0, 0], [0, 2, 0]]), s)
    assert idx.tolist() == [0, 0, 1] and d2.tolist() == [1.0, 0.0, 1.0]
    d2, idx = R.nearest(np.zeros((2, 3), np.float32), np.zeros((0, 3), np.float32))
    assert np.isinf(d2).all() and idx.tolist() == [0, 0]
    T = np.array([[0, -1, 0, 1.0], [1, 0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float64)
    d2, idx = R.nearest(np.float32([[1, 1, 0]]), s, s_transform=T)  # T s = {(1,1,0), (0,0,0), ...}
    assert idx.tolist() == [0] and d2.tolist() == [0.0]
    assert R.nearest(np.float32([[1, 0, 0]]), s, q_transform=T)[1].tolist() == [0]  # T q = (1, 1, 0): rows 0, 1, 2, 4 at d2 = 1


def test_library_exports_and_workspace_sizes():
    L = _lib.lib()
    for name in ('rdm_nearest_workspace_bytes', 'rdm_nearest', 'rdm_realign_error', 'rdm_engine_alignment_quality'):
        assert hasattr(L, name) and name in _lib.SIGNATURES
    small, large = L.rdm_nearest_workspace_bytes(0, 0), L.rdm_nearest_workspace_bytes(16000, 16000)
    assert 0 < small < large
    assert L.rdm_nearest_workspace_bytes(16000, 16000) == large
    assert L.rdm_nearest_workspace_bytes(16000, 0) < large and L.rdm_nearest_workspace_bytes(0, 16000) < large


def test_quality_dict_arithmetic():
    q = ops.quality_dict([3.0, 0.75, 5.0, 0.0, 0.0, 8.0, 4.0, 2.0])
    assert q == {'fitness_ref': 0.75, 'inlier_rmse_ref': 0.5, 'fitness_src': 0.0, 'inlier_rmse_src': 0.0, 'chamfer': 5.0 / 4 + 8.0 / 2,
                 'n_ref': 4, 'n_src': 2}
    assert set(ops.QUALITY_KEYS) < set(q) and len(ops.QUALITY_KEYS) == 5
    empty = ops.quality_dict([0.0] * 8)
    assert empty['fitness_ref'] == 0.0 and empty['inlier_rmse_src'] == 0.0 and math.isnan(empty['chamfer'])
