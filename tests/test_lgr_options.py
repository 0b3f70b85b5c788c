"""CPU: cfg.fine_matching's options (topk, mutual, use_dustbin, confidence_threshold, use_global_score, correspondence_limit) --
the config check, the host-side size functions of the C-ABI, and tests/lgr_options_restatement.py against the reference's
LocalGlobalRegistration recorded in tests/golden/lgr_options.npz (gen_lgr_options_golden.py), so that the restatement the
GPU tests lean on is itself pinned where no GPU is present."""
import ctypes
import os

import numpy as np
import pytest
import torch

import lgr_options_restatement as R
from rdmnet_amd import _lib, config

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
ENTRIES = R.fixture_entries(GOLDEN)


# ------------------------------------------------------------------------------------------------ config
def test_default_fine_matching_options_are_none():
    cfg = config.make_cfg()
    assert config.fine_matching_options(cfg) is None
    cfg.fine_matching.confidence_threshold = 0.05  # not read with the dustbin: still the shipped behaviour
    assert config.fine_matching_options(cfg) is None
    for k in R.OPTION_KEYS:  # a missing key means its shipped value
        del cfg.fine_matching[k]
    assert config.fine_matching_options(cfg) is None


@pytest.mark.parametrize('key,value', [('topk', 3), ('mutual', True), ('use_dustbin', False), ('use_global_score', True),
                                       ('correspondence_limit', 300)])
def test_a_changed_option_is_returned(key, value):
    cfg = config.make_cfg()
    cfg.fine_matching[key] = value
    o = config.fine_matching_options(cfg)
    assert o is not None and set(o) == set(R.OPTION_KEYS) and o[key] == value
    want = dict(config.FINE_MATCHING_DEFAULTS, **{key: value})
    assert o == want
    _lib.FineMatchingOptions.of(**o)  # the keyword arguments of the binding


def test_topk_may_reach_the_line_length():
    cfg = config.make_cfg()
    cfg.fine_matching.topk = 129  # K + 1 with the dustbin
    assert config.fine_matching_options(cfg)['topk'] == 129
    cfg.fine_matching.use_dustbin = False
    with pytest.raises(ValueError, match='topk'):
        config.fine_matching_options(cfg)
    cfg.fine_matching.topk = 128
    assert config.fine_matching_options(cfg)['topk'] == 128


@pytest.mark.parametrize('key,value', [
    ('topk', 0), ('topk', -1), ('topk', 130), ('topk', 2.0), ('topk', None), ('topk', True), ('topk', '3'),
    ('confidence_threshold', -0.01), ('confidence_threshold', float('nan')), ('confidence_threshold', None),
    ('confidence_threshold', '0.05'),
    ('correspondence_limit', 0), ('correspondence_limit', -5), ('correspondence_limit', 2.5), ('correspondence_limit', True),
    ('mutual', 1), ('use_dustbin', None), ('use_global_score', 'yes')])
def test_rejected_values_raise_a_value_error_naming_the_key(key, value):
    cfg = config.make_cfg()
    cfg.fine_matching[key] = value
    with pytest.raises(ValueError, match=rf'cfg\.fine_matching\.{key}\b'):
        config.fine_matching_options(cfg)


def test_negative_threshold_is_rejected_without_the_dustbin_too():
    cfg = config.make_cfg()
    cfg.fine_matching.use_dustbin = False
    cfg.fine_matching.confidence_threshold = -1e-3
    with pytest.raises(ValueError, match='confidence_threshold'):
        config.fine_matching_options(cfg)


# ------------------------------------------------------------------------------------------------ C-ABI, host side
def test_options_struct_and_size_functions():
    L = _lib.lib()
    assert ctypes.sizeof(_lib.FineMatchingOptions) == 24
    d = _lib.FineMatchingOptions.of()
    assert L.rdm_lgr_options_capacity(256, 128, ctypes.byref(d)) == 256 * 2 * 128
    assert L.rdm_lgr_options_workspace_bytes(256, 128, ctypes.byref(d)) == L.rdm_lgr_workspace_bytes(256)
    k3 = _lib.FineMatchingOptions.of(topk=3)
    assert L.rdm_lgr_options_capacity(256, 128, ctypes.byref(k3)) == 256 * 6 * 128  # min(2 k K, K K)
    assert L.rdm_lgr_options_capacity(2, 4, ctypes.byref(k3)) == 2 * 16
    lim = _lib.FineMatchingOptions.of(topk=3, correspondence_limit=300)
    assert (L.rdm_lgr_options_workspace_bytes(256, 128, ctypes.byref(lim)) - L.rdm_lgr_options_workspace_bytes(256, 128, ctypes.byref(k3))
            >= 300 * 7 * 4)  # the verification set
    for bad in (_lib.FineMatchingOptions.of(topk=0), _lib.FineMatchingOptions.of(topk=130),
                _lib.FineMatchingOptions.of(topk=129, use_dustbin=False), _lib.FineMatchingOptions.of(confidence_threshold=-1.0),
                _lib.FineMatchingOptions.of(confidence_threshold=float('nan')), _lib.FineMatchingOptions.of(correspondence_limit=-1)):
        assert L.rdm_lgr_options_capacity(256, 128, ctypes.byref(bad)) == 0
        assert L.rdm_lgr_options_workspace_bytes(256, 128, ctypes.byref(bad)) == 0


# ------------------------------------------------------------------------------------------------ the restatement
def test_restatement_keeps_the_lowest_index_among_ties():
    rp, sp, rm, sm, ms, gs = R.tie_patch()
    fm = config.make_cfg().fine_matching
    run = R.lgr(rp, sp, rm, sm, ms, gs, fm, R.options(topk=2, mutual=True))
    got = {tuple(r[1:]) for r in run['indices'].tolist()}
    # row 0 keeps columns 1 and 3 (not 4); column 5 keeps rows 2 and 4 (not 5); mutual needs both sides
    assert (0, 1) in got and (0, 3) in got and (0, 4) not in got
    assert (2, 5) in got and (4, 5) in got and (5, 5) not in got
    run = R.lgr(rp, sp, rm, sm, ms, gs, fm, R.options(topk=2, correspondence_limit=3))
    s = run['corr_scores']
    top = float(s.max())
    tied = [i for i in range(len(s)) if float(s[i]) == top]
    assert len(tied) > 3 and run['verification'].tolist() == tied[:3]  # the lowest positions among the tied best scores


@pytest.mark.parametrize('case,name', ENTRIES)
def test_restatement_reproduces_the_reference(case, name):
    """Correspondences by the fixture's rule (exact, or tie-aware within the undecided set and its 2 % cap), scores bit for
    bit on the common entries, and the reference's pose: with the verification set in the reference's order the
    restatement runs the reference's arithmetic, so the bounds are the LGR pose bounds of test_reference_goldens_gpu.py
    (1e-3 deg; 1e-5 m on the crops, 1e-4 m at full size) -- from the reference's own hypothesis or, where inlier counts tie
    within one, from one of the near-tied ones (tie_aware.py)."""
    from oracle import forward as ofw
    opt, f = R.fixture_entry(GOLDEN, case, name)
    inputs = R.golden_inputs(GOLDEN, case)
    fm = config.make_cfg().fine_matching
    run = R.lgr(*inputs, fm, opt)
    R.compare_correspondences(run['indices'].numpy(), f)
    want = {tuple(r): s for r, s in zip(f['indices'].astype(np.int64).tolist(), f['corr_scores'].tolist())}
    got = {tuple(r): s for r, s in zip(run['indices'].tolist(), run['corr_scores'].tolist())}
    assert all(got[k] == want[k] for k in got.keys() & want.keys())
    if opt['correspondence_limit'] is not None:
        assert len(want) > opt['correspondence_limit'] and len(run['verification']) == opt['correspondence_limit']
        assert float(f['limit_gap']) > 10 * R.UNDECIDED
    if 'inlier_counts' in f:
        assert np.array_equal(run['inlier_counts'].numpy(), f['inlier_counts']) and run['best'] == int(f['best'])
    bound_t = 1e-5 if case in ('small', 'crop9') else 1e-4
    errs = []
    for h in f['alt_hypotheses'].tolist():
        T = R.lgr(*inputs, fm, opt, force_best=None if h < 0 else h, by_score=True)['transform'].numpy()
        errs.append(ofw.rre_rte(T, f['transform']))
    assert any(rre <= 1e-3 and rte <= bound_t for rre, rte in errs), errs
