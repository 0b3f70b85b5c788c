"""CPU: the float64 brute-force restatement of the descriptor protocol (tests/feature_match_restatement.py) against the
reference's recorded outputs (tests/golden/feature_match.npz, gen_feature_match_golden.py), and the harness / evaluator plumbing
of `infer --feature-match` and `eval --method ransac_featurematch` that needs no GPU."""
import os

import numpy as np
import pytest

import feature_match_restatement as R
from rdmnet_amd import eval as cli, evaluation

MODES = {'nearest': {}, 'mutual': {'mutual': True}, 'bilateral': {'bilateral': True}}


@pytest.fixture(scope='module')
def fx(golden_dir):
    z = np.load(os.path.join(golden_dir, 'feature_match.npz'))
    return {k: z[k] for k in z.files}


def test_fixture_holds_the_three_cases(fx):
    assert [str(n) for n in fx['names']] == ['crop9', 'small', 'random']
    assert fx['random/ref_feats'].shape == (300, 86) and fx['random/src_feats'].shape == (257, 86)
    for tag in ('crop9', 'small'):
        assert fx[f'{tag}/ref_feats'].shape[1] == 256 and fx[f'{tag}/ref_feats'].dtype == np.float32
    assert all(float(fx[f'{n}/min_gap']) > 0 for n in fx['names'])  # no exact tie: cKDTree's answer is defined


@pytest.mark.parametrize('tag', ['crop9', 'small', 'random'])
@pytest.mark.parametrize('mode', list(MODES))
def test_restatement_equals_the_reference_indices(fx, tag, mode):
    ri, si = R.corr_indices(fx[f'{tag}/ref_feats'], fx[f'{tag}/src_feats'], **MODES[mode])
    assert ri.dtype == si.dtype == np.int64
    assert np.array_equal(ri, fx[f'{tag}/{mode}/ref_corr_indices']) and np.array_equal(si, fx[f'{tag}/{mode}/src_corr_indices'])


@pytest.mark.parametrize('tag', ['crop9', 'small', 'random'])
@pytest.mark.parametrize('mode', ['nearest', 'mutual'])
def test_restatement_equals_the_reference_correspondences(fx, tag, mode):
    rc, sc, dist = R.correspondences(fx[f'{tag}/ref_points'], fx[f'{tag}/src_points'], fx[f'{tag}/ref_feats'], fx[f'{tag}/src_feats'],
                                     mutual=mode == 'mutual', return_feat_dist=True)
    assert np.array_equal(rc, fx[f'{tag}/{mode}/ref_corr_points']) and np.array_equal(sc, fx[f'{tag}/{mode}/src_corr_points'])
    ulps = R.ulp_diff(dist, fx[f'{tag}/{mode}/feat_dists'])
    print(tag, mode, 'distance vs np.linalg.norm: max ulp', int(ulps.max()), 'rows off by one', int((ulps == 1).sum()), 'of', len(ulps))
    assert dist.dtype == np.float32 and ulps.max() <= 1


def test_fast_restatement_equals_the_brute_force_one(fx):
    a, b = fx['random/ref_feats'], fx['random/src_feats'].copy()
    b[200] = b[7]  # an exact tie: the lowest index
    a[3] = b[7]
    for x, y in ((a, b), (b, a)):
        i0, d0 = R.nearest(x, y)
        i1, d1 = R.nearest_fast(x, y)
        assert np.array_equal(i0, i1) and R.ulp_diff(d0, d1).max() <= 1
    assert R.nearest(a, b)[0][3] == 7


def test_eval_command_line_takes_ransac_featurematch(capsys):
    a = cli.make_parser(own_methods=True).parse_args(['--features-root', 'x', '--method', 'ransac_featurematch', '--num_corr', '100'])
    assert (a.method, a.num_corr) == ('ransac_featurematch', 100)
    assert cli.OWN_METHODS == ('ransac_featurematch',) and cli.KERNEL_METHOD['ransac_featurematch'] == 'ransac'
    for method in cli.METHODS:  # the reference's methods as before
        assert cli.make_parser(own_methods=True).parse_args(['--features-root', 'x', '--method', method]).method == method
    with pytest.raises(SystemExit):
        cli.make_parser(own_methods=True).parse_args(['--features-root', 'x', '--method', 'teaser'])
    assert 'teaser' in capsys.readouterr().err


def test_eval_main_takes_the_method_and_names_a_missing_key(tmp_path):
    """`python -m rdmnet_amd.eval --method ransac_featurematch` gets past the parser; on a pair file without the feat_* keys it
    fails while reading, before any GPU work, with the key and the flag that writes it."""
    _pair_file(tmp_path, False, test_py=True)
    with pytest.raises(KeyError, match=r"feat_ref_corr_points.*--feature-match"):
        cli.main(['--features-root', str(tmp_path), '--method', 'ransac_featurematch'])


def _pair_file(tmp_path, with_features, test_py=False):
    rng = np.random.default_rng(1)
    keys = evaluation.TEST_NPZ_KEYS if test_py else evaluation.NPZ_KEYS
    out = {k: rng.standard_normal((5, 3)).astype(np.float32) for k in keys}
    out['ref_node_corr_indices'] = out['src_node_corr_indices'] = np.arange(3)
    out['gt_node_corr_indices'] = np.zeros((2, 2), np.int64)
    item = {'seq_id': 0, 'ref_frame': 1, 'src_frame': 2, 'transform': np.eye(4, dtype=np.float32)}
    extra = None
    if with_features:
        fm = dict(ref_corr_indices=np.arange(4), src_corr_indices=np.arange(4)[::-1].copy(),
                  ref_corr_points=rng.standard_normal((4, 3)).astype(np.float32),
                  src_corr_points=rng.standard_normal((4, 3)).astype(np.float32), feat_dists=np.array([.3, .1, .2, .4], np.float32))
        extra = evaluation.feature_match_arrays(fm)
    if test_py:
        return evaluation.save_pair_test_npz(str(tmp_path), item, out, extra=extra), extra
    return evaluation.save_pair_npz(str(tmp_path), item, out, extra=extra), extra


@pytest.mark.parametrize('test_py', [False, True])
def test_pair_file_keys_with_and_without_feature_match(tmp_path, test_py):
    (tmp_path / 'a').mkdir()
    plain, _ = _pair_file(tmp_path / 'a', False, test_py)
    base = set(np.load(plain).files)
    want = (set(evaluation.TEST_NPZ_KEYS) | {'transform'}) if test_py else (set(evaluation.NPZ_KEYS) | {'estimated_transform_ransac', 'transform'})
    assert base == want  # without the flag: what the harness has always written
    (tmp_path / 'b').mkdir()
    with_fm, extra = _pair_file(tmp_path / 'b', True, test_py)
    z = np.load(with_fm)
    assert set(z.files) == base | set(evaluation.FEATURE_MATCH_KEYS) and len(evaluation.FEATURE_MATCH_KEYS) == 5
    for k in evaluation.FEATURE_MATCH_KEYS:
        assert np.array_equal(z[k], extra[k])


def test_eval_reads_the_descriptor_rows_and_names_a_missing_key(tmp_path):
    (tmp_path / 'a').mkdir()
    (tmp_path / 'b').mkdir()
    with_fm, extra = _pair_file(tmp_path / 'a', True, test_py=True)
    d = cli.load_pair(with_fm, 'ransac_featurematch')
    assert np.array_equal(d['ref_corr_points'], extra['feat_ref_corr_points'])
    assert np.array_equal(d['src_corr_points'], extra['feat_src_corr_points'])
    assert np.array_equal(d['corr_scores'], -extra['feat_corr_dists']) and d['corr_scores'].dtype == np.float32
    assert np.array_equal(cli.load_pair(with_fm)['ref_corr_points'], np.load(with_fm)['ref_corr_points'])  # other methods: as before
    plain, _ = _pair_file(tmp_path / 'b', False, test_py=True)
    with pytest.raises(KeyError, match=r"feat_ref_corr_points.*--feature-match"):
        cli.load_pair(plain, 'ransac_featurematch')
    cli.load_pair(plain)
