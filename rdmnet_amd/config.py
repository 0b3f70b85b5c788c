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
