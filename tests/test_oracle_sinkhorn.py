"""CPU: the Sinkhorn restatement (oracle/forward.py: sinkhorn) where a whole side of a patch is masked.  The reference's
LearnableLogOptimalTransport (modules/sinkhorn/learnable_sinkhorn.py:13-66), run in fp32, gives there:
  no valid row (nr = 0):     after >= 1 iteration the dustbin column [:, n] is -inf, masked rows included (log_nu[n] =
                             log 0 + norm), the valid entries of the dustbin row are 0.0, everything else fl(-1e12);
  no valid column (nc = 0):  the mirror image (dustbin row -inf, valid entries of the dustbin column 0.0);
  neither (nr = nc = 0):     norm = -log 0 = +inf: every entry is -inf without iterations and NaN after one.
With iters = 0 and one non-empty side the output is Z - norm, finite everywhere.  rdm_sinkhorn reproduces these
(tests/test_heads_gpu.py); this file pins the restatement it is checked against, in fp32 and in fp64."""
import pytest
import torch

from oracle import forward as ofw

M, N = 11, 9


def assert_masked(x, dtype):
    """fp32: exactly fl(-1e12), the reference's value; fp64: -1e12 plus the O(10) potentials, which fp32 rounds away."""
    if dtype == torch.float32:
        assert torch.equal(x, torch.full_like(x, -1e12))
    else:
        assert (x + 1e12).abs().max() <= 1e3


def case(nr, nc, dtype, alpha, iters):
    g = torch.Generator().manual_seed(nr * 100 + nc)
    s = (torch.randn(1, M, N, generator=g) * 3).to(dtype)
    rm, cm = torch.zeros(1, M, dtype=torch.bool), torch.zeros(1, N, dtype=torch.bool)
    rm[0, torch.randperm(M, generator=g)[:nr]] = True   # scattered, not a prefix
    cm[0, torch.randperm(N, generator=g)[:nc]] = True
    out = ofw.sinkhorn(s, rm, cm, torch.tensor(alpha, dtype=dtype), iters)
    assert out.dtype == dtype
    return out[0], rm[0], cm[0]


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
@pytest.mark.parametrize('alpha', [-5.0, 1.0, 8.0])
@pytest.mark.parametrize('iters', [1, 100])
def test_no_valid_row(dtype, alpha, iters):
    o, _, cm = case(0, 5, dtype, alpha, iters)
    assert torch.isneginf(o[:, N]).all()                               # the whole dustbin column, masked rows included
    dust = o[M, :N][cm]
    if dtype == torch.float32:
        assert torch.equal(dust, torch.zeros_like(dust))                 # the reference's fp32: exactly 0.0
    else:
        assert dust.abs().max() <= 1e-14 * (abs(alpha) + 10)             # 0 up to fp64 rounding of alpha + log(nc + 1) terms
    assert_masked(o[M, :N][~cm], dtype)
    assert_masked(o[:M, :N], dtype)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
@pytest.mark.parametrize('alpha', [-5.0, 1.0, 8.0])
@pytest.mark.parametrize('iters', [1, 100])
def test_no_valid_column(dtype, alpha, iters):
    o, rm, _ = case(7, 0, dtype, alpha, iters)
    assert torch.isneginf(o[M, :]).all()
    dust = o[:M, N][rm]
    if dtype == torch.float32:
        assert torch.equal(dust, torch.zeros_like(dust))
    else:
        assert dust.abs().max() <= 1e-14 * (abs(alpha) + 10)
    assert_masked(o[:M, N][~rm], dtype)
    assert_masked(o[:M, :N], dtype)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_no_valid_row_or_column(dtype):
    assert torch.isnan(case(0, 0, dtype, 1.0, 1)[0]).all()
    assert torch.isnan(case(0, 0, dtype, 1.0, 100)[0]).all()
    assert torch.isneginf(case(0, 0, dtype, 1.0, 0)[0]).all()


@pytest.mark.parametrize('nr,nc', [(0, 5), (7, 0)])
def test_one_empty_side_without_iterations_is_z_minus_norm(nr, nc):
    o, rm, cm = case(nr, nc, torch.float32, 8.0, 0)
    assert torch.isfinite(o).all()
    want = torch.tensor(8.0) - (-torch.log(torch.tensor(float(nr + nc))))   # alpha - norm, rounded once in fp32
    dust = o[M, :N][cm] if nr == 0 else o[:M, N][rm]
    assert torch.equal(dust, want.expand_as(dust)) and o[M, N] == want
    assert_masked(o[:M, :N], torch.float32)
