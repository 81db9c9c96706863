"""FLOAT64 restatement, rounding bounds and the shared input sets of the gaussian likelihood-gradient kernel gcpx_gauss_nll_bwd
(tests/test_gpu_gauss_kernel.py runs the kernel on them, tests/test_gauss_refs_cpu.py pins everything here without a GPU).

The restatement is plain torch in float64 of what include/gcpx.h states for the kernel's five outputs; it is no transcription of
csrc/loss.hip.  Every sum comes with its abs-terms: the same expression with every term replaced by its absolute value.

The bounds follow tests/loss_refs.py: eps = 2^-24 (f32 unit roundoff), nothing measured.  Form:
        eps x (k_elem x abs-terms of the elements + depth x sum |elements|)
  k_elem  the f32 roundings one element goes through as the kernel performs them; expf is TAKEN as <= 2 ulp = 4 eps relative
          (loss_refs.TRANSC);
  depth   the longest chain of additions a value passes through (sum_depth).
The counts stand beside the code that uses them."""
import math

import numpy as np
import torch

from loss_refs import EPS, TRANSC, f32

HALF_LOG_2PI = 0.5 * math.log(2 * math.pi)


def reference(mu, x, w, ls, scale, pitch):
    """mu, x [rows][C][npix], w [rows], ls and scale numbers -> dict of float64 tensors:
      dy [rows][npix][pitch]   slot c < C: scale w_row (mu - x) exp(-2 ls) (1 - mu^2), slots >= C: 0
      colsum [rows][pitch]     sums of dy over the pixels,                       colsum_abs: of |dy|
      nll [rows]               sum over the row of 0.5 d^2 + ls + 0.5 log(2 pi), d = (x - mu) exp(-ls)   (every row, whatever its weight)
      nll_abs [rows]           sum of 0.5 d^2 + |ls| + 0.5 log(2 pi)
      dls [rows]               scale w_row sum over the row of (1 - d^2),        dls_abs [rows]: |scale w_row| sum of (1 + d^2), dls_mag: |scale w_row| sum |1 - d^2|"""
    mu, x, w = mu.double(), x.double(), w.double()
    rows, C, npix = mu.shape
    ls = float(ls)
    g = scale * w[:, None, None] * (mu - x) * math.exp(-2 * ls) * (1 - mu * mu)
    dy = torch.zeros(rows, npix, pitch, dtype=torch.float64)
    dy[:, :, :C] = g.permute(0, 2, 1)
    d2 = ((x - mu) * math.exp(-ls)) ** 2
    sw = (scale * w).abs()
    return dict(dy=dy, colsum=dy.sum(1), colsum_abs=dy.abs().sum(1),
                nll=(0.5 * d2 + ls + HALF_LOG_2PI).sum((1, 2)), nll_abs=(0.5 * d2 + abs(ls) + HALF_LOG_2PI).sum((1, 2)),
                dls=scale * w * (1 - d2).sum((1, 2)), dls_abs=sw * (1 + d2).sum((1, 2)), dls_mag=sw * (1 - d2).abs().sum((1, 2)))


def sum_depth(per_pixel, npix):
    """additions a value of a row sum passes through: a lane of gauss_nll_bwd_kernel adds `per_pixel` terms for each of its
    ceil(npix / 256) pixels in turn, the wavefront's butterfly has 6 levels, the four wavefronts combine in 2.  (gauss_nll_kernel, which
    nll_out is also compared with: ceil(C npix / 256) serial terms per thread and the 8 levels of its 256-thread tree — the same count.)"""
    return per_pixel * -(-npix // 256) + 6 + 2


# dy element: k = (scale * w) * expf(-2 ls): 2 roundings + expf; (mu - x): 1; fmaf(-mu, mu, 1): 1 (the product inside is exact);
# k * (mu - x) * (1 - mu^2): 2.  Every factor's error is relative to the factor, so they add: 6 + TRANSC, and 1 for the second-order
# terms of ten compounded roundings.  A saturated mu = +-1 gives fmaf(-1, 1, 1) = 0 exactly, and mu == x gives 0 exactly: bound 0.
K_DY = 6 + TRANSC + 1
# nll element, abs-terms m = 0.5 d^2 + |ls| + c: d = (x - mu) * expf(-ls): 2 roundings + expf = 6 relative to d, so 12 to d^2, 1 for the
# product d * d (the halving is exact): 13 x 0.5 d^2; the f32 constant c is off by <= 1 eps c; "+ ls" and "+ c" round a value <= m each.
K_NLL = 13 + 1 + 2
# d log_sigma element, abs-terms a = 1 + d^2: fmaf(-d, d, 1) rounds once (<= a) a value whose d^2 carries the 12 eps of d above;
# behind the sum, scale * w and the product with the total: 2 roundings relative to the total (<= sum a).
K_DLS = 12 + 1 + 2


def tolerances(mu, x, w, ls, scale, pitch):
    """bounds on |kernel - reference| for dy (element-wise), colsum [rows][pitch], nll [rows], dls [rows]"""
    r = reference(mu, x, w, ls, scale, pitch)
    C, npix = mu.shape[1], mu.shape[2]
    return dict(dy=EPS * K_DY * r["dy"].abs(),
                colsum=EPS * (K_DY + sum_depth(1, npix)) * r["colsum_abs"],
                nll=EPS * (K_NLL * r["nll_abs"] + sum_depth(C, npix) * r["nll_abs"]),
                dls=EPS * (K_DLS * r["dls_abs"] + sum_depth(C, npix) * r["dls_mag"]))


ROWS, CH, PITCH = 5, 3, 16
NPIX = (64, 1024)                      # 8 x 8 (one wavefront has work, three idle) and 32 x 32 (every wavefront, four trips)
LOG_SIGMAS = (0.0, -2.5, 1.5)
ZERO_ROW, SCALED_ROW = 1, 2            # rows of weight 0 and of weight 0.37


def case(npix, ls, seed=0):
    """rows = 5, C = 3, pitch = 16.  mu = tanh of N(0, 1.5^2) in f32 with every 7th element exactly +1 or -1 (saturated tanh) and
    every 11th target equal to its mu; targets uniform over [-1, 1]; row 1 weighs 0, row 2 weighs 0.37; scale = w_rec / (B T C npix) at
    B = 2, T = 20 rounded to f32 as the C ABI passes it."""
    g = torch.Generator().manual_seed(1000 * seed + npix + int(10 * (ls + 5)))
    mu = torch.tanh(1.5 * torch.randn(ROWS, CH, npix, generator=g, dtype=torch.float64)).float()
    flat = mu.view(-1)
    flat[0::7] = torch.where(torch.arange(flat[0::7].numel()) % 2 == 0, 1.0, -1.0)
    x = (2 * torch.rand(ROWS, CH, npix, generator=g) - 1).float()
    x.view(-1)[3::11] = flat[3::11]
    w = torch.ones(ROWS)
    w[ZERO_ROW], w[SCALED_ROW] = 0.0, 0.37
    return dict(mu=mu, x=x, w=w, ls=f32(ls), scale=f32(1.0 / (2 * 20 * CH * npix)), pitch=PITCH, npix=npix)


def kernel_f32(mu, x, w, ls, scale, pitch, drop=None):
    """the operation chain of gauss_nll_bwd_kernel restated in float32 numpy (sums in float64: the bound's depth term stays unused), to
    show on the CPU that the element bounds hold for f32 arithmetic and that planted mistakes (`drop`) do not pass:
    'exp2' no exp(-2 ls) factor, 'tanh' no (1 - mu^2), 'sign' x - mu, 'weight' the row weight ignored, 'ls_const' d log_sigma without the 1"""
    F = np.float32
    mu, x, w = mu.numpy().astype(F), x.numpy().astype(F), w.numpy().astype(F)
    ls, scale = F(ls), F(scale)
    rows, C, npix = mu.shape
    inv = np.exp(-ls, dtype=F)
    wk = np.ones_like(w) if drop == "weight" else w
    k = (scale * wk) * (F(1) if drop == "exp2" else np.exp(F(-2) * ls, dtype=F))
    diff = (x - mu) if drop == "sign" else (mu - x)
    tanh_d = F(1) if drop == "tanh" else (F(1) - mu.astype(np.float64) ** 2).astype(F)          # (fmaf: one rounding)
    g = (k[:, None, None] * diff).astype(F) * tanh_d
    dy = np.zeros((rows, npix, pitch), F)
    dy[:, :, :C] = g.transpose(0, 2, 1)
    dy[w == 0] = 0
    d = ((x - mu) * inv).astype(F)
    nll = (F(0.5) * d * d + ls + F(0.9189385332)).astype(np.float64).sum((1, 2))
    one = F(0) if drop == "ls_const" else F(1)
    dls_e = (one - d.astype(np.float64) ** 2).astype(F)
    dls = ((scale * wk) * dls_e.astype(np.float64).sum((1, 2)).astype(F)).astype(F)
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))
    return dict(dy=t(dy), colsum=t(dy.astype(np.float64).sum(1)), nll=t(nll), dls=t(dls))
