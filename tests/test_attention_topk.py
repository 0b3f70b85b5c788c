"""CPU: the host side of top-k attention (cfg.thdroformer.k2) -- the kept count int(n * f), the configuration checks, and
that a dense k2 (None, or None in every used entry) configures the engine exactly as before."""
import contextlib
import ctypes
import types

import numpy as np
import pytest
import torch

from rdmnet_amd import _lib, config, model

FRACS = [0.0, 0.07, 0.1, 0.3, 0.57, 0.7, 0.9, 1.0]


def test_topk_count_is_pythons_int_of_the_double_product():
    L = _lib.lib()
    below = 0
    for f in FRACS:
        for n in range(0, 10001):
            want = int(n * f)
            assert L.rdm_topk_count(n, f) == want, (n, f)
            below += want != round(n * f) and abs(n * f - round(n * f)) < 1e-9
    assert L.rdm_topk_count(100, 0.57) == 56  # the product is 56.99999999999999 in double
    assert L.rdm_topk_count(213, 57 / 213) == 56  # the golden's round-down case
    assert below > 100  # the sweep does cover products just below an integer


def cfg_with(k2, **kw):
    c = config.make_cfg()
    c.thdroformer.k2 = k2
    for k, v in kw.items():
        c.thdroformer[k] = v
    return c


@pytest.mark.parametrize('k2, what', [
    ([0.5, 0.5, 0.5], 'k2 has 3 entries'),
    ([], 'k2 has 0 entries'),
    (0.5, 'sequence'),
    ('0.5', 'sequence'),
    ([0.5, 0.5, 1.5, 0.5], 'k2[2]'),
    ([0.5, -0.1, 0.5, 0.5], 'k2[1]'),
    ([0.5, 0.5, 0.5, float('nan')], 'k2[3]'),
    ([0.5, 0.5, '0.5', 0.5], 'k2[2]'),
    ([True, 0.5, 0.5, 0.5], 'k2[0]'),
])
def test_bad_k2_is_a_value_error_naming_the_key(k2, what):
    c = cfg_with(k2)
    with pytest.raises(ValueError, match='k2') as ei:
        config.topk_fractions(c)
    assert what in str(ei.value)
    with pytest.raises(ValueError, match='k2'):
        model.create_model(c)
    with pytest.raises(ValueError, match='k2'):
        model.create_eval_model(c)


def test_k2_with_bf16_attention_is_rejected():
    c = cfg_with([0.5, 0.5, 0.5, 0.5], attention_bf16=True)
    with pytest.raises(ValueError, match='attention_bf16'):
        model.create_model(c)
    assert config.topk_fractions(cfg_with([None] * 4, attention_bf16=True)) is None  # dense: nothing to reject


def test_valid_k2_is_read_per_self_layer():
    assert config.topk_fractions(cfg_with([0.3, None, 57 / 213, 1, 'ignored', None])) == [0.3, -1.0, 57 / 213, 1.0]
    assert config.topk_fractions(cfg_with((0, 0.5, np.float32(0.25), 1.0))) == [0.0, 0.5, 0.25, 1.0]
    assert model.create_model(cfg_with([0.3, 0.5, 0.7, 1.0])).topk2 == [0.3, 0.5, 0.7, 1.0]


class _RecordingLib:
    """Stands in for librdmnet_hip.so: records every entry point called, every call succeeds."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


def engine_calls(monkeypatch, k2):
    from rdmnet_amd import engine
    fake = _RecordingLib()
    monkeypatch.setattr(_lib, 'lib', lambda: fake)
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: True)
    monkeypatch.setattr(torch.cuda, 'device', lambda d: contextlib.nullcontext())
    engine.Engine(cfg_with(k2), None, device='cuda:0', share_with=types.SimpleNamespace(_h=ctypes.c_void_p(1)))
    return fake.calls


@pytest.mark.parametrize('k2', [None, [None] * 4, [None, None, None, None, 0.5]])
def test_dense_k2_makes_no_topk_call(monkeypatch, k2):
    calls = engine_calls(monkeypatch, k2)
    assert [n for n, _ in calls] == [n for n, _ in engine_calls(monkeypatch, None)]
    assert not any('topk' in n for n, _ in calls)


def test_k2_configures_the_engine(monkeypatch):
    calls = engine_calls(monkeypatch, [0.3, None, 0.7, 1.0])
    (n_layers, fracs), = [a[1:] for n, a in calls if n == 'rdm_engine_set_attention_topk']
    assert n_layers == 4 and list(fracs) == [0.3, -1.0, 0.7, 1.0]
