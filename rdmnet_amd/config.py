"""Configuration of the inference path.  Mirrors the constants the reference reads from its
EasyDict (experiments/config.py:84-161); only keys used by inference are kept."""
import numbers

import numpy as np


class Cfg(dict):
    """Attribute-style dict (the reference uses easydict.EasyDict the same way)."""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e

    def __setattr__(self, k, v):
        self[k] = v


def make_cfg():
    c = Cfg()
    c.backbone = Cfg(num_stages=5, init_voxel_size=0.3, kernel_size=15, base_radius=4.25, base_sigma=2.0,
                     group_norm=32, input_dim=1, init_dim=64, output_dim=256)
    c.backbone.init_radius = c.backbone.base_radius * c.backbone.init_voxel_size  # config.py:91
    c.backbone.init_sigma = c.backbone.base_sigma * c.backbone.init_voxel_size    # config.py:92
    c.model = Cfg(num_points_in_patch=128, num_sinkhorn_iterations=100, n2p_score_threshold=0.1,
                  p2p_score_threshold=0.1)
    c.coarse_matching = Cfg(num_correspondences=256, dual_normalization=True)
    c.thdroformer = Cfg(input_dim=2048, hidden_dim=128, output_dim=256, num_heads=4, num_layers=4,
                        input_dim2=256, num_layers2=4, k2=None,
                        attention_bf16=False)  # True: BASELINE.json configs[3] (bf16 QK^T / PV, fp32 softmax)
    c.Vote = Cfg(model_use_vote=True, inference_use_vote=True, MAX_TRANSLATE_RANGE=[3.0, 3.0, 3.0],
                 MLPS=[512, 256], NMS_radius=2.4)
    c.fine_matching = Cfg(acceptance_radius=0.6, mutual=False, topk=1, confidence_threshold=0,
                          use_dustbin=True, use_global_score=False, correspondence_threshold=3,
                          correspondence_limit=None, num_refinement_steps=5)
    c.test = Cfg(vis=False)
    c.neighbor_limits = [65, 63, 69, 70, 81]  # calibrated on the bundled pairs (utils/data.py:195-220)
    return c


def topk_fractions(cfg):
    """cfg.thdroformer.k2 checked and read: None when every self layer of transformer #2 is dense (k2 None, or None in each
    of the first num_layers2 entries), else one float per self layer, -1.0 for a dense one (the encoding of
    rdm_engine_set_attention_topk).  A layer keeps int(n * f) keys of a cloud of n superpoints (thdroformer.py:20-40).
    Raises ValueError naming the key for: a k2 that is not a sequence; fewer than num_layers2 entries (an IndexError in the
    reference); an entry that is not None or a real number in [0, 1] (the reference also runs 1 < f while int(n * f) <= n,
    which depends on the data: rejected up front here); k2 together with attention_bf16 (no top-k variant of that mode).
    Entries past num_layers2 are ignored, as in the reference."""
    t = cfg.thdroformer
    k2 = t.get('k2', None)
    if k2 is None:
        return None
    if isinstance(k2, (str, bytes)) or not hasattr(k2, '__len__') or not hasattr(k2, '__getitem__'):
        raise ValueError(f'cfg.thdroformer.k2 must be None or a sequence of per-layer fractions, got {k2!r}')
    n = int(t.num_layers2)
    if len(k2) < n:
        raise ValueError(f'cfg.thdroformer.k2 has {len(k2)} entries; transformer #2 has num_layers2 = {n} self layers')
    fracs = []
    for i in range(n):
        f = k2[i]
        if f is None:
            fracs.append(-1.0)
            continue
        if isinstance(f, (bool, np.bool_)) or not isinstance(f, numbers.Real):
            raise ValueError(f'cfg.thdroformer.k2[{i}] must be None or a real number in [0, 1], got {f!r}')
        if not 0.0 <= float(f) <= 1.0:  # (also rejects NaN)
            raise ValueError(f'cfg.thdroformer.k2[{i}] = {f!r} is outside [0, 1]')
        fracs.append(float(f))
    if all(f < 0 for f in fracs):
        return None
    if t.get('attention_bf16', False):
        raise ValueError('cfg.thdroformer.k2 cannot be combined with cfg.thdroformer.attention_bf16 (no top-k variant of '
                         'bf16 attention)')
    return fracs


FINE_MATCHING_DEFAULTS = dict(topk=1, mutual=False, use_dustbin=True, confidence_threshold=0.0, use_global_score=False,
                              correspondence_limit=None)


def check_fine_matching(values, points_in_patch, where='cfg.fine_matching.'):
    """The six options in `values` (a missing one means its shipped value) checked and normalised -> dict.  Raises ValueError
    naming the offending key, prefixed with `where`: a topk that is not an integer in [1, K] ([1, K + 1] with use_dustbin), K =
    points_in_patch (torch.topk raises beyond that); a confidence_threshold that is not a real number >= 0 (also NaN: in the
    reference a negative threshold matches every zero entry of the scattered matrix); a correspondence_limit that is neither
    None nor an integer >= 1; a flag that is not a bool."""
    o = {k: values.get(k, v) for k, v in FINE_MATCHING_DEFAULTS.items()}
    for k in ('mutual', 'use_dustbin', 'use_global_score'):
        if not isinstance(o[k], (bool, np.bool_)):
            raise ValueError(f'{where}{k} must be a bool, got {o[k]!r}')
        o[k] = bool(o[k])
    side = int(points_in_patch) + (1 if o['use_dustbin'] else 0)
    k = o['topk']
    if isinstance(k, (bool, np.bool_)) or not isinstance(k, numbers.Integral) or not 1 <= int(k) <= side:
        raise ValueError(f'{where}topk must be an integer in [1, {side}], got {k!r}')
    o['topk'] = int(k)
    t = o['confidence_threshold']
    if isinstance(t, (bool, np.bool_)) or not isinstance(t, numbers.Real) or not float(t) >= 0.0:  # (also rejects NaN)
        raise ValueError(f'{where}confidence_threshold must be a real number >= 0, got {t!r}')
    o['confidence_threshold'] = float(t)
    lim = o['correspondence_limit']
    if lim is not None:
        if isinstance(lim, (bool, np.bool_)) or not isinstance(lim, numbers.Integral) or int(lim) < 1:
            raise ValueError(f'{where}correspondence_limit must be None or an integer >= 1, got {lim!r}')
        o['correspondence_limit'] = int(lim)
    return o


def fine_matching_options(cfg):
    """cfg.fine_matching.{topk, mutual, use_dustbin, confidence_threshold, use_global_score, correspondence_limit} checked and
    read (local_global_registration.py:11-47; the other three keys travel in the engine configuration): None when all six hold
    the values the reference ships -- the registration then runs its k = 1 / dustbin / non-mutual kernel -- else a dict of the
    six (the keyword arguments of ops.lgr and _lib.FineMatchingOptions.of).  A missing key means its shipped value.
    Raises the ValueErrors of check_fine_matching, each naming its key."""
    o = check_fine_matching(cfg.fine_matching, cfg.model.num_points_in_patch)
    # (confidence_threshold is not read with the dustbin: any valid value is the shipped behaviour then)
    same = all(o[k] == v for k, v in FINE_MATCHING_DEFAULTS.items() if not (k == 'confidence_threshold' and o['use_dustbin']))
    return None if same else o
