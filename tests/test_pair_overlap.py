"""CPU: the float64 restatement of the ball query (tests/pair_overlap_restatement.py) against the reference's recorded
get_correspondences / compute_overlap (tests/golden/pair_overlap.npz), the new C symbols, and the argument errors that need no GPU.
The fixture's generator asserts that no pair lies within 1e-9 relative of the radius, so equality is exact."""
import os

import numpy as np
import pytest
import torch

import pair_overlap_restatement as R
from rdmnet_amd import _lib, engine, ops, prepare


@pytest.fixture(scope='module')
def fx(golden_dir):
    z = np.load(os.path.join(golden_dir, 'pair_overlap.npz'))
    return {k: z[k] for k in z.files}


@pytest.fixture(scope='module')
def pairs(golden_dir):
    z = np.load(os.path.join(golden_dir, 'synthetic_pairs.npz'))
    return {k: z[k] for k in z.files}


def test_restatement_equals_the_reference(fx, pairs):
    assert len(fx['pairs']) >= 2 and fx['closest_relative'] > 1e-9
    for p in fx['pairs']:
        ref, src, T = pairs[f'ref{p}'], pairs[f'src{p}'], pairs[f'T{p}']
        assert list(fx['radii']) == sorted(fx['radii'], reverse=True)
        widest = R.ball_query(ref, src, T, fx['radii'][0])  # (one brute-force pass per pair: the narrower lists are its subsets)
        for r in fx['radii']:
            q = R.narrowed(widest, r)
            want = fx[f'p{p}/r{r}/corr']
            assert want.dtype == np.int32 and np.array_equal(q['corr'], want.astype(np.int64)), (p, r)
            assert np.array_equal(q['counts'], np.bincount(want[:, 0], minlength=len(ref)))
            assert R._fraction(q['ref_min_d2'], r) == float(fx[f'p{p}/r{r}/overlap']), (p, r)
            # the src side against the reference's call with the roles swapped (its own rounding of the inverse transform;
            # the generator asserts that no nearest distance is within 1e-9 relative of r)
            assert R._fraction(q['src_min_d2'], r) == float(fx[f'p{p}/r{r}/overlap_src']), (p, r)


def test_two_point_case_pins_closed_ball_and_strict_overlap(fx):
    ref, src, r = fx['two_point/ref'], fx['two_point/src'], float(fx['two_point/radius'])
    assert fx['two_point/corr'].tolist() == [[0, 0]] and float(fx['two_point/overlap']) == 0.0  # the reference's own answers
    assert R.get_correspondences(ref, src, None, r).tolist() == [[0, 0]]
    assert R.compute_overlap(ref, src, None, r, both=True) == (0.0, 0.0)
    assert R.compute_overlap(ref, src, None, np.nextafter(r, 1.0), both=True) == (1.0, 1.0)


def test_restatement_of_empty_clouds():
    a, e = np.zeros((3, 3), np.float32), np.zeros((0, 3), np.float32)
    for ref, src in ((a, e), (e, a), (e, e)):
        assert R.get_correspondences(ref, src, None, 1.0).shape == (0, 2)
        assert R.compute_overlap(ref, src, None, 1.0, both=True) == (0.0, 0.0)


def test_new_symbols_are_exported():
    L = _lib.lib()
    for name in ('rdm_ball_workspace_bytes', 'rdm_ball_count', 'rdm_ball_fill', 'rdm_engine_gt_point_correspondences_count',
                 'rdm_engine_gt_point_correspondences_fill'):
        assert hasattr(L, name) and name in _lib.SIGNATURES, name
    small, large = L.rdm_ball_workspace_bytes(0, 0), L.rdm_ball_workspace_bytes(16000, 16000)
    assert 0 < small < large
    assert L.rdm_ball_workspace_bytes(16000, 16000) == large  # the count and the fill call carve the same layout


def test_argument_errors_need_no_gpu():
    a = torch.zeros((4, 3))
    for radius in (None, 0, -0.5, float('nan')):
        with pytest.raises(ValueError, match='matching_radius must be > 0'):
            ops.get_correspondences(a, a, None, radius)
        with pytest.raises(ValueError, match='positive_radius must be > 0'):
            ops.compute_overlap(a, a, None, radius)
        with pytest.raises(ValueError, match='radius must be > 0'):
            ops.overlap_labels(a, a, None, radius)
    with pytest.raises(ValueError, match='float32 CUDA tensor'):
        ops.get_correspondences(a, a, None, 0.6)  # (a host tensor is not silently computed on the host)
    with pytest.raises(ValueError, match='4x4'):
        ops._transform_arg(np.eye(3), 'get_correspondences')
    assert sorted(engine.POINT_LEVELS) == ['coarse', 'fine', 'input']


def test_prepare_overlap_command_line(tmp_path):
    assert prepare.format_overlap_line(3, 14, 0.5, 0.25, 7) == '3 14 0.500000 0.250000 7\n'
    with pytest.raises(SystemExit):
        prepare.main(['overlap', '--dataset-root', str(tmp_path), '--radius', '0'])
    with pytest.raises(SystemExit):
        prepare.main(['overlap', '--dataset-root', str(tmp_path), '--workers', '17'])
    with pytest.raises(FileNotFoundError, match='no pair lists'):
        prepare.main(['overlap', '--dataset-root', str(tmp_path)])
