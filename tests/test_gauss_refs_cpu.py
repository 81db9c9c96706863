"""Pins tests/gauss_refs.py without a GPU: the float64 restatement of gcpx_gauss_nll_bwd's outputs against torch autograd over the
oracle's own gaussian likelihood (oracle/gcp_model_oracle.py:551-553) composed with tanh and the NCHW -> pixel-record layout; the
derived bounds against a float32 restatement of the kernel's operation chain (they hold) and against planted mistakes (they do not)."""
import math

import pytest
import torch

import gauss_refs as G


def _autograd(y, x, w, ls, scale, pitch):
    """d (scale sum_r w_r NLL_r) / d y and / d log_sigma by autograd in float64; y = the head's pre-tanh output [rows][C][npix]"""
    y = y.clone().requires_grad_(True)
    lsv = torch.tensor(ls, dtype=torch.float64, requires_grad=True)
    mu = torch.tanh(y)
    err = 0.5 * ((x - mu) / torch.exp(lsv)) ** 2 + lsv + 0.5 * math.log(2 * math.pi)          # the oracle's expression
    nll = err.sum((1, 2))
    total = scale * (nll * w).sum()
    gy, gls = torch.autograd.grad(total, [y, lsv])
    rows, C, npix = y.shape
    dy = torch.zeros(rows, npix, pitch, dtype=torch.float64)
    dy[:, :, :C] = gy.permute(0, 2, 1)
    return mu.detach(), dy, float(gls), nll.detach()


@pytest.mark.parametrize("ls", G.LOG_SIGMAS)
def test_restatement_is_the_autograd_gradient(ls):
    g = torch.Generator().manual_seed(3)
    rows, C, npix, pitch = 4, 3, 64, 16
    y = 1.5 * torch.randn(rows, C, npix, generator=g, dtype=torch.float64)
    x = 2 * torch.rand(rows, C, npix, generator=g, dtype=torch.float64) - 1
    w = torch.tensor([1.0, 0.0, 0.37, 1.0], dtype=torch.float64)
    scale = 1.0 / (2 * 20 * C * npix)
    mu, dy, gls, nll = _autograd(y, x, w, ls, scale, pitch)
    r = G.reference(mu, x, w, ls, scale, pitch)
    assert float((r["dy"] - dy).abs().max()) <= 1e-12 * float(dy.abs().max())
    assert bool((r["dy"][:, :, C:] == 0).all()) and bool((r["dy"][1] == 0).all())
    assert float((r["colsum"] - dy.sum(1)).abs().max()) <= 1e-12 * float(dy.abs().sum(1).max())
    assert float((r["nll"] - nll).abs().max()) <= 1e-12 * float(nll.abs().max())
    assert abs(float(r["dls"].sum()) - gls) <= 1e-12 * float(r["dls_abs"].sum())
    assert abs(gls) > 1e-4                                # (a gradient of log_sigma that could not be told from none proves nothing)


@pytest.mark.parametrize("npix", G.NPIX)
@pytest.mark.parametrize("ls", G.LOG_SIGMAS)
def test_bounds_hold_for_f32_and_catch_planted_mistakes(npix, ls):
    c = G.case(npix, ls)
    args = (c["mu"], c["x"], c["w"], c["ls"], c["scale"], c["pitch"])
    ref, tol = G.reference(*args), G.tolerances(*args)
    # the inputs are what the docstring of case() says
    assert bool((c["mu"].abs() == 1).any()) and bool((c["mu"] == c["x"]).any())
    assert float(c["w"][G.ZERO_ROW]) == 0 and 0 < float(c["w"][G.SCALED_ROW]) < 1
    sat = (c["mu"].abs() == 1).permute(0, 2, 1)
    assert bool((ref["dy"][:, :, :G.CH][sat] == 0).all()), "saturated tanh: gradient exactly 0"
    got = G.kernel_f32(*args)
    for k in ("dy", "colsum", "nll", "dls"):
        err = (got[k] - ref[k]).abs()
        assert bool((err <= tol[k]).all()), (k, float((err / tol[k].clamp_min(1e-300)).max()))
    # the bounds are tight enough to see each mistake ('exp2' is invisible at log_sigma = 0: the factor is 1)
    for drop, key in (("exp2", "dy"), ("tanh", "dy"), ("sign", "dy"), ("weight", "dy"), ("ls_const", "dls")):
        if drop == "exp2" and ls == 0.0:
            continue
        bad = G.kernel_f32(*args, drop=drop)
        assert bool(((bad[key] - ref[key]).abs() > tol[key]).any()), drop


def test_sum_depth():
    assert G.sum_depth(1, 64) == 1 + 8 and G.sum_depth(3, 1024) == 12 + 8 and G.sum_depth(3, 4096) == 48 + 8
