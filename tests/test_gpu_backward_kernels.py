"""-m gpu: each backward kernel of the training step against torch.autograd in FLOAT64 of the formula it differentiates, at the
edges where such kernels go wrong (saturated targets and clamps, masked frames, border taps, the last partial block of rows, padding
columns, strided destinations).  The whole-model gradient tests compare at 1e-3 of a tensor's max-abs after every error has flowed
through a conv into a weight gradient; these compare every element a kernel writes.

Conventions of every test here:
  * the kernel is called through video_gcp_amd.runtime with the argument conventions of its call site in the planner (cited);
  * every output starts as NaN: elements the kernel must write are checked finite (and against the reference), elements it must leave
    alone still hold the NaN;
  * a tolerance is stated with its derivation.  eps = 2^-24 (f32 unit roundoff).  "abs-terms" of a quantity = the same expression with
    every term replaced by its absolute value, in float64: a sum of n f32 terms is within n eps x abs-terms of the exact sum
    (the deterministic summation orders here are serial or shallower), a product chain of k roundings within k eps relative."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
NAN = float("nan")


@pytest.fixture(scope="module")
def env():
    from video_gcp_amd import runtime as rt, packing as pk
    lib = rt.load_library()
    assert torch.cuda.is_available()
    return rt, pk, lib, torch.device("cuda")


def _st():
    return torch.cuda.current_stream().cuda_stream


def _nan(*shape, dev="cuda"):
    return torch.full(shape, NAN, device=dev)


def _within(got, ref, tol, name):
    """|got - ref| <= tol element-wise (tol a tensor or a number); got must be finite.  Returns the worst error / tolerance."""
    got, ref = got.double(), ref.double().to(got.device)
    tol = torch.as_tensor(tol, dtype=torch.float64, device=got.device).expand_as(ref)
    assert bool(torch.isfinite(got).all()), f"{name}: {int((~torch.isfinite(got)).sum())} elements not written (or not finite)"
    err = (got - ref).abs()
    bad = err > tol
    if bool(bad.any()):
        i = int(torch.nonzero(bad.flatten())[0])
        raise AssertionError(f"{name}: {int(bad.sum())}/{bad.numel()} elements outside the bound; first at flat index {i}: got "
                             f"{float(got.flatten()[i])} want {float(ref.flatten()[i])} tol {float(tol.flatten()[i]):.3e}; "
                             f"worst err/tol {float((err / tol.clamp_min(1e-300)).max()):.3g}")
    return float((err / tol.clamp_min(1e-300)).max())


def _untouched(t, name):
    assert bool(torch.isnan(t).all()), f"{name}: {int((~torch.isnan(t)).sum())} elements written that the kernel must leave alone"


# ------------------------------------------------------------------------------------------------------------------------------
# a. conv-block backward chain: gcpx_act_bwd / gcpx_act_skip_bwd -> gcpx_bn_bwd_finalize -> gcpx_bn_bwd_apply
# ------------------------------------------------------------------------------------------------------------------------------
# (C, H, F, up, fsum, add, ldc, c_off, accumulate, skip (Cs, rpb) or None)
_CHAIN = [
    (16, 4, 3, 1, 1, False, 32, 16, 0, None),          # 4 x 4 -> 8 x 8: every low-resolution pixel is a border pixel
    (32, 4, 1, 0, 1, True, 32, 0, 1, None),             # count 16: a one-sample error in the BatchNorm count is 6 %
    (64, 8, 4, 0, 3, True, 128, 32, 1, None),           # skip broadcast: three frames summed per output frame
    (128, 8, 2, 1, 2, False, 256, 128, 0, None),        # upsampled and summed over frames
    (16, 32, 5, 1, 1, True, 48, 4, 1, None),
    (128, 64, 1, 0, 1, True, 128, 0, 0, None),
    (16, 64, 2, 1, 1, True, 32, 0, 1, (16, 2)),         # act_skip_bwd: skip half summed over rpb = 2 frames
    (32, 8, 6, 1, 1, False, 96, 0, 0, (32, 3)),
    (64, 4, 8, 1, 1, True, 192, 64, 1, (64, 4)),
]


def _chain_case(env, C_, H, Fr, up, fsum, with_add, ldc, c_off, acc, skip, mean_off=0.5, seed=0):
    rt, pk, lib, dev = env
    g = torch.Generator(device=dev).manual_seed(1000 + seed + C_ + H + Fr)
    Hd = 2 * H if up else H
    Cs, rpb = skip if skip else (0, 1)
    c_off_s = (c_off + C_) if skip else 0
    if skip:
        ldc = max(ldc, c_off_s + Cs)
    # raw conv output with batch statistics away from 0 (mean_off) and per-channel spread; the affine in front of the LeakyReLU
    r = (torch.randn(Fr, H, H, C_, device=dev, generator=g) * (torch.rand(C_, device=dev, generator=g) + 0.5) + mean_off)
    gamma = torch.rand(C_, device=dev, generator=g) + 0.5
    beta = torch.randn(C_, device=dev, generator=g) * 0.3
    da = torch.randn(Fr * fsum, Hd, Hd, ldc, device=dev, generator=g)
    add = torch.randn(Fr, H, H, C_, device=dev, generator=g) if with_add else None
    eps_bn = 1e-5
    r64 = r.double()
    mean64 = r64.mean((0, 1, 2))
    var64 = r64.var((0, 1, 2), unbiased=False)
    rstd64 = 1.0 / torch.sqrt(var64 + eps_bn)
    mean, rstd = mean64.float(), rstd64.float()
    scale = gamma * rstd                                        # what the forward's BatchNorm hands the backward (bn["scale"], bn["shift"])
    shift = beta - mean * scale
    nb = lib.gcpx_act_bwd_blocks()
    dy = _nan(Fr, H, H, C_)
    st = _nan(nb, 2, C_)
    coef = _nan(3, C_)
    pre_g, pre_b = torch.randn(C_, device=dev, generator=g), torch.randn(C_, device=dev, generator=g)
    dgam, dbet = pre_g.clone(), pre_b.clone()
    if not acc:
        dgam.fill_(NAN)
        dbet.fill_(NAN)
    a = rt.ActBwdArgs()                                          # backward_ops.py:255-268
    a.da, a.add, a.r = da.data_ptr(), rt.ptr(add), r.data_ptr()
    a.scale, a.shift, a.mean, a.rstd = scale.data_ptr(), shift.data_ptr(), mean.data_ptr(), rstd.data_ptr()
    a.dy, a.stats_partial, a.ldc, a.c_off, a.up, a.fsum, a.act = dy.data_ptr(), st.data_ptr(), ldc, c_off, up, fsum, rt.ACT_LRELU
    a.F, a.H, a.W, a.C = Fr, H, H, C_
    ds = None
    if skip:
        ds = _nan(Fr // rpb, H, H, Cs)
        rt.check(lib.gcpx_act_skip_bwd(C.byref(a), ds.data_ptr(), c_off_s, Cs, rpb, _st()), "act_skip_bwd")
    else:
        rt.check(lib.gcpx_act_bwd(C.byref(a), _st()), "act_bwd")
    count = float(Fr * H * H)                                    # backward_ops.py:275-284
    rt.check(lib.gcpx_bn_bwd_finalize(st.data_ptr(), nb, C_, C.c_double(count), gamma.data_ptr(), rstd.data_ptr(), coef.data_ptr(),
                                      dgam.data_ptr(), dbet.data_ptr(), acc, _st()), "bn_bwd_finalize")
    rt.check(lib.gcpx_bn_bwd_apply(dy.data_ptr(), r.data_ptr(), mean.data_ptr(), rstd.data_ptr(), coef.data_ptr(), Fr * H * H * C_, C_,
                                   _st()), "bn_bwd_apply")
    torch.cuda.synchronize()

    # float64 reference: r -> batch-stat BatchNorm -> affine -> LeakyReLU(0.2) -> bilinear x2 -> channel slice of an ldc-wide tensor,
    # summed over fsum frames, plus the `add` term.  The LeakyReLU's side of its kink is the f32 forward's: sign(r * scale + shift)
    # evaluated exactly (the product of two f32 is exact in float64; the kernel's fmaf rounds once, which keeps the sign) — a unit
    # within rounding of the kink has two defensible derivatives, and this picks the one the training step's forward computed.
    pos = (r64 * scale.double() + shift.double()) > 0
    x = r64.permute(0, 3, 1, 2).clone().requires_grad_(True)
    gam64, bet64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    xh = (x - x.mean((0, 2, 3), keepdim=True)) / torch.sqrt(x.var((0, 2, 3), unbiased=False, keepdim=True) + eps_bn)
    y = xh * gam64[None, :, None, None] + bet64[None, :, None, None]
    act = torch.where(pos.permute(0, 3, 1, 2), y, 0.2 * y)
    upd = F.interpolate(act, scale_factor=2, mode="bilinear", align_corners=False) if up else act
    dsl = da[..., c_off:c_off + C_].double().permute(0, 3, 1, 2).reshape(Fr, fsum, C_, Hd, Hd)
    loss = (upd[:, None] * dsl).sum()
    if add is not None:
        loss = loss + (act * add.double().permute(0, 3, 1, 2)).sum()
    dr_ref, dg_ref, db_ref = torch.autograd.grad(loss, (x, gam64, bet64))
    dr_ref = dr_ref.permute(0, 2, 3, 1)
    # abs-terms: the gradient reaching the activation (16 taps x fsum frames + add, each a product of positive weights)
    dsa = dsl.abs().sum(1)
    ta = act.new_zeros(act.shape).requires_grad_(True)
    tu = F.interpolate(ta, scale_factor=2, mode="bilinear", align_corners=False) if up else ta
    (gabs,) = torch.autograd.grad((tu * dsa).sum(), ta)
    with torch.no_grad():
        if add is not None:
            gabs = gabs + add.double().permute(0, 3, 1, 2).abs()
        gdy = gabs * torch.where(pos.permute(0, 3, 1, 2), 1.0, 0.2)                      # |dL/dy| bound, per element
        xh_d = xh.detach()
        k = (gamma.double() * rstd64)[None, :, None, None]
        m1a = gdy.mean((0, 2, 3), keepdim=True)
        m2a = (gdy * xh_d.abs()).mean((0, 2, 3), keepdim=True)
        absterm = (k * (gdy + m1a + xh_d.abs() * (m1a + m2a))).permute(0, 2, 3, 1)
        dg_abs, db_abs = (gdy * xh_d.abs()).sum((0, 2, 3)), gdy.sum((0, 2, 3))
    # Bound on dr: the activation gradient sums 16 fsum + 1 products (dy: (16 fsum + 3) eps of its abs-terms); the two channel means
    # are f32 sums over count C / 2^20 elements per thread (2^18 threads, C / 4 channel groups), <= 64 threads per channel within a
    # workgroup, then float64: (count C / 2^20 + 64) eps of their abs-terms; x_hat carries the rounding of the stored f32 mean relative
    # to the spread, |mean| rstd eps absolute (hence the |x_hat| m1 term of the abs-terms); the apply step rounds 4 times.
    # tol = (16 fsum + count C / 2^20 + 96 + 2 |mean| rstd) eps x abs-terms of dr.
    mr = float((mean64.abs() * rstd64).max())
    n_sum = count * C_ / 2.0 ** 20 + 64
    n_term = 16 * fsum + n_sum + 32 + 2 * mr
    w1 = _within(dy, dr_ref, n_term * EPS * absterm, "dr (act_bwd -> bn_bwd_finalize -> bn_bwd_apply)")
    # d gamma / d beta: the same channel sums, undivided (plus the x_hat shift of the stored mean, |mean| rstd eps x sum |dy|)
    tsum = (n_sum + 4) * EPS
    base_g = pre_g.double() if acc else 0.0
    base_b = pre_b.double() if acc else 0.0
    w2 = _within(dgam, dg_ref + base_g, tsum * dg_abs + (2 * mr + 2) * EPS * db_abs +
                 2 * EPS * (dg_ref.abs() + (pre_g.double().abs() if acc else 0)), "d gamma")
    w3 = _within(dbet, db_ref + base_b, tsum * db_abs + 2 * EPS * (db_ref.abs() + (pre_b.double().abs() if acc else 0)), "d beta")
    assert bool(torch.isfinite(coef).all()) and bool(torch.isfinite(st).all())
    w4 = 0.0
    if skip:
        # skip half: ds[b] = sum over the rpb frames of the sequence of the transposed bilinear x2 of channels c_off_s .. + Cs
        s = torch.zeros(Fr, Cs, H, H, dtype=torch.float64, device=dev, requires_grad=True)
        su = F.interpolate(s, scale_factor=2, mode="bilinear", align_corners=False)
        dsk = da[..., c_off_s:c_off_s + Cs].double().permute(0, 3, 1, 2)
        (gs,) = torch.autograd.grad((su * dsk).sum(), s)
        (gsa,) = torch.autograd.grad((su * dsk.abs()).sum(), s)
        ds_ref = gs.reshape(Fr // rpb, rpb, Cs, H, H).sum(1).permute(0, 2, 3, 1)
        ds_abs = gsa.reshape(Fr // rpb, rpb, Cs, H, H).sum(1).permute(0, 2, 3, 1)
        w4 = _within(ds, ds_ref, (16 * rpb + 2) * EPS * ds_abs, "ds (skip half)")
    return max(w1, w2, w3, w4)


@pytest.mark.parametrize("C_,H,Fr,up,fsum,with_add,ldc,c_off,acc,skip", _CHAIN)
def test_act_bn_chain_vs_float64(env, C_, H, Fr, up, fsum, with_add, ldc, c_off, acc, skip):
    """The conv block's backward chain as backward_ops._bn_bwd issues it (backward_ops.py:255-284): gcpx_act_bwd (or
    gcpx_act_skip_bwd with the skip connection's half, rpb > 1) -> gcpx_bn_bwd_finalize (accumulate 0 / 1 into prefilled d gamma /
    d beta) -> gcpx_bn_bwd_apply, against autograd in float64 of batch-stat BatchNorm -> affine -> LeakyReLU(0.2) -> optional
    bilinear x2 -> channel slice [c_off, c_off + C) of an ldc-wide tensor, summed over fsum frames, plus `add`.  Compared: dr, d gamma,
    d beta (and ds).  Tolerance: (16 fsum + count C / 2^20 + 96 + 2 |mean| rstd) eps of dr's abs-terms, derivation in the body;
    (count C / 2^20 + 68) eps of the abs-terms for the parameter sums; ds (16 rpb + 2) eps of its abs-terms."""
    w = _chain_case(env, C_, H, Fr, up, fsum, with_add, ldc, c_off, acc, skip)
    print(f"act/bn chain C={C_} H={H} up={up} fsum={fsum} skip={skip}: worst err / tol {w:.3f}")


def test_act_bn_chain_decoder_block_count(env):
    """The chain at the pixel count of a c2 decoder block (F H W = 1024 x 64 x 64 = 4.2M per channel, the partial sums of every
    workgroup full) with a batch mean 12 standard deviations from 0: x_hat = (r - mean) rstd is then formed from two close numbers and
    the BatchNorm sums of dy x_hat cancel.  Same reference and bounds as test_act_bn_chain_vs_float64 (the bound grows with count C / 2^20
    and with |mean| rstd, both stated there)."""
    w = _chain_case(env, 16, 64, 1024, 0, 1, True, 32, 16, 1, None, mean_off=12.0, seed=7)
    print(f"act/bn chain at 4.2M pixels per channel: worst err / tol {w:.3f}")


# ------------------------------------------------------------------------------------------------------------------------------
# b. / c. the mixture head's likelihood and mean backward (csrc/scalar_f32.hip)
# ------------------------------------------------------------------------------------------------------------------------------
def _inv_perm(pk):
    perm = torch.tensor(pk.dlm_channel_perm(10))
    slots = torch.nonzero(perm >= 0)[:, 0]
    inv = torch.empty(100, dtype=torch.long)
    inv[perm[slots]] = slots
    return perm, inv


def _dlm_params(rows, S, g, dev, edges=True):
    """canonical head output l [rows, 100, S, S] (PixelCNN++ order) with the edges of the likelihood: sharp and flat logits, log-scales
    far below the -7 clamp and exactly at it, narrow bins far from the target (vanishing bin probability: the log-pdf branch),
    saturated colour coefficients"""
    nm = 10
    l = torch.empty(rows, 100, S, S, device=dev)
    l[:, :nm] = torch.randn(rows, nm, S, S, device=dev, generator=g)
    rest = l[:, nm:].view(rows, 3, 3 * nm, S, S)
    rest[:, :, :nm] = torch.rand(rows, 3, nm, S, S, device=dev, generator=g) * 1.6 - 0.8          # means
    rest[:, :, nm:2 * nm] = torch.rand(rows, 3, nm, S, S, device=dev, generator=g) * 3 - 4.5       # log-scales in [-4.5, -1.5]
    rest[:, :, 2 * nm:] = torch.randn(rows, 3, nm, S, S, device=dev, generator=g)                  # raw colour coefficients
    if edges:
        h = S // 4
        l[0::4, :nm] *= 25.0                                        # sharp mixture logits
        l[1::4, :nm] *= 0.01                                        # flat
        rest[2::4, :, 2 * nm:] *= 12.0                               # saturated tanh coefficients
        rest[:, 1, nm:2 * nm, :h, :h] = -9.0                         # green log-scales far below the clamp: no gradient through it
        rest[:, 2, nm:2 * nm, h:2 * h, :h] = -7.0                    # blue log-scales AT the clamp: torch's inclusive rule passes the gradient
        rest[:, :, nm:2 * nm, 2 * h:3 * h, :h] = -5.5                 # narrow bins ...
        rest[:, :, :nm, 2 * h:3 * h, :h] = -0.45                      # ... far from the targets set below: cdf_delta <= 1e-5
    return l


def _dlm_targets(rows, S, g, dev):
    """targets on the loader's 256 levels (k / 255 * 2 - 1, data_loader.py:220), with saturated blocks at -1 / +1 and the
    neighbouring levels +-(1 - 2/255)"""
    k = torch.randint(0, 256, (rows, 3, S, S), device=dev, generator=g).float()
    x = k / 255.0 * 2.0 - 1.0
    h = S // 4
    x[:, :, :h, h:2 * h] = -1.0
    x[:, :, h:2 * h, h:2 * h] = 1.0
    x[:, :, 3 * h:, :h] = -(1.0 - 2.0 / 255.0)
    x[:, :, 3 * h:, h:2 * h] = 1.0 - 2.0 / 255.0
    x[:, :, 2 * h:3 * h, :h] = 0.5 + torch.randint(0, 2, (rows, 3, h, h), device=dev, generator=g).float() * 0.3   # far from the -0.45 means
    return x


def _to_kernel(l, perm):
    """canonical [rows, 100, S, S] -> the head's memory layout [rows, S*S, 112] (empty slots 0)"""
    rows, _, S, _ = l.shape
    out = torch.zeros(rows, S * S, len(perm), device=l.device, dtype=l.dtype)
    pt = perm.to(l.device)
    sl = torch.nonzero(pt >= 0)[:, 0]
    out[:, :, sl] = l.permute(0, 2, 3, 1).reshape(rows, S * S, 100)[:, :, pt[sl]]
    return out


def _tail_bound(l, x, g, row_coef, hp):
    """Per-element bound [rows, 100, S, S] (canonical order) of the f32 cancellation in the likelihood's middle branch, float64: a bin's
    probability sigmoid(plus) - sigmoid(minus) is known to ~8 eps absolute (each sigmoid rounds against 1 in the far tail), so the
    terms of mixture k carry e_k = sum over colours of 8 eps / cdf_delta relative error (1 where cdf_delta is within 10 % of the
    branch threshold: f32 may take the other branch); the responsibilities w shift by w_k (e_k + sum_j w_j e_j).  Bound: (e_k + 2
    sum_j w_j e_j) x |gradient| for the mixture's parameters (x row_coef w_k for its logit), plus the absolute error of the
    derivatives themselves, row_coef w_k e_kc x inv (means, colour coefficients) or x (|plus| + |minus| + 1) (log-scales)."""
    from oracle import gcp_model_oracle as O
    with torch.no_grad():
        nm = hp.n_mixtures
        lg, means, ls, cf = O.dlm_split(l, hp)
        xr, xg = x[:, 0:1], x[:, 1:2]
        m = torch.stack([means[:, 0], means[:, 1] + cf[:, 0] * xr, means[:, 2] + cf[:, 1] * xr + cf[:, 2] * xg], 1)
        xx = x[:, :, None].expand_as(m)
        xc, inv = xx - m, torch.exp(-ls)
        plus, minus, mid_in = inv * (xc + 1 / 255.0), inv * (xc - 1 / 255.0), inv * xc
        cdf = torch.sigmoid(plus) - torch.sigmoid(minus)
        inner = torch.where(cdf > 1e-5, torch.log(cdf.clamp_min(1e-12)), mid_in - ls - 2 * F.softplus(mid_in) - math.log(127.5))
        lp = torch.where(xx < -0.999, plus - F.softplus(plus), torch.where(xx > 0.999, -F.softplus(minus), inner))
        w = torch.softmax(lp.sum(1) + torch.log_softmax(lg, 1), 1)                      # responsibilities [rows, nm, S, S]
        inner_x = xx.abs() <= 0.999
        mid = inner_x & (cdf > 1e-5)
        near = inner_x & ((cdf - 1e-5).abs() < 1e-6)            # within f32 reach of the branch threshold: either branch
        e_c = torch.where(mid, 8 * EPS / cdf.clamp_min(1e-30), torch.zeros_like(cdf)) + near.double()    # [rows, 3, nm, S, S]
        e = e_c.sum(1)
        rel = e + 2 * (w * e).sum(1, keepdim=True)                                      # [rows, nm, S, S]
        cw = row_coef[:, None, None, None] * w
        am = cw[:, None] * inv * e_c                               # d / d mean of colour c: inv (pp - pm) / cdf, absolute
        a_s = cw[:, None] * (plus.abs() + minus.abs() + 1) * e_c     # d / d log_scale: (plus pp - minus pm) / cdf, absolute
        out = torch.zeros_like(g)
        out[:, :nm] = cw * rel
        rest = out[:, nm:].view(out.shape[0], 3, 3, nm, *out.shape[2:])                 # [rows, colour, (mean, ls, coeff), k]
        rest.copy_(rel[:, None, None] * g[:, nm:].abs().view_as(rest))
        rest[:, :, 0] += am
        rest[:, :, 1] += a_s
        rest[:, 0, 2] += am[:, 1]                                    # coefficient c0 enters the green mean, c1 / c2 the blue
        rest[:, 1, 2] += am[:, 2]
        rest[:, 2, 2] += am[:, 2]
        return out


@pytest.mark.parametrize("S,rows,weights", [(32, 520, "zeros"), (64, 300, "zeros"), (32, 16, "null")])
def test_dlm_nll_bwd_vs_float64(env, S, rows, weights):
    """gcpx_dlm_nll_bwd as the balanced model's stored-parameters training path calls it (forward_plan.py:714, backward_plan.py:88:
    row weight = pad_mask, scale = dense_img_rec_weight / (B prod(traj.shape[1:])), colsum and nll_out set) against autograd in float64
    of oracle.dlm_nll x row weight x scale.  Targets on the loader's 256 levels with saturated blocks (the x = -1 / +1 branches) and
    their neighbours; log-scales below / at the -7 clamp; bins whose probability vanishes (log-pdf branch); sharp / flat logits;
    saturated colour coefficients; rows with weight 0 (written as zeros, colsum 0, nll 0) or no row weights at all.  300 / 520 rows:
    more workgroups than the chip has CUs.
    Tolerances: gradients 5e-5 of the row's largest + 2e-4 relative — the bound of test_conv3x3_head_nll_grad_values for the same
    formulas on the same hardware exp / rcp helpers (the bin probability is a difference of two sigmoids; one rounding of each is
    ~1e-5 of the difference and d / d mean, d / d log_scale divide by it) — plus, element by element, the cancellation in a bin's far
    tail (_tail_bound): both sigmoids round against 1, so any f32 evaluation of the formula keeps only ~8 eps / cdf_delta of relative
    precision in that bin's terms (up to 5 % just above the 1e-5 branch threshold), and through the responsibilities in the whole pixel.  nll_out: bit-equal to gcpx_dlm_nll on the same input (the
    kernel claims its reduction order) and within 1e-4 relative of float64 (npix terms of ~1e-6 relative each, edge rows included).
    colsum: the sum of the kernel's own rows within 1024 eps of the abs-terms (each lane sums npix / 4 <= 1024 values serially).
    Slots 100..111 are exactly 0."""
    rt, pk, lib, dev = env
    from oracle import gcp_model_oracle as O
    from video_gcp_amd import config
    hp = config("c1")
    g = torch.Generator(device=dev).manual_seed(S + rows)
    perm, inv = _inv_perm(pk)
    l = _dlm_params(rows, S, g, dev)
    x = _dlm_targets(rows, S, g, dev)
    params = _to_kernel(l, perm).contiguous()
    wgt = None
    if weights == "zeros":
        wgt = torch.rand(rows, device=dev, generator=g) * 0.5 + 0.75
        wgt[3::7] = 0.0
    scale = 1.0 / (4 * 20 * 3 * S * S)
    npix, P = S * S, len(perm)
    dpar = _nan(rows, npix, P)
    colsum = _nan(rows, P)
    nll = _nan(rows)
    rt.check(lib.gcpx_dlm_nll_bwd(params.data_ptr(), x.data_ptr(), rt.ptr(wgt), C.c_float(scale), dpar.data_ptr(), colsum.data_ptr(),
                                  nll.data_ptr(), rows, npix, P, 10, _st()), "dlm_nll_bwd")
    nll_fwd = _nan(rows)
    rt.check(lib.gcpx_dlm_nll(params.data_ptr(), x.data_ptr(), rt.ptr(wgt), nll_fwd.data_ptr(), rows, npix, P, 10, _st()), "dlm_nll")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dpar).all()) and bool(torch.isfinite(colsum).all()) and bool(torch.isfinite(nll).all())
    assert bool((dpar[..., 100:] == 0).all()), "slots 100..111 must be written as 0"
    assert torch.equal(nll, nll_fwd), "nll_out differs from gcpx_dlm_nll on the same input"
    w = wgt if wgt is not None else torch.ones(rows, device=dev)
    zero_rows = torch.nonzero(w == 0)[:, 0]
    if len(zero_rows):
        assert bool((dpar[zero_rows] == 0).all()) and bool((colsum[zero_rows] == 0).all()) and bool((nll[zero_rows] == 0).all())
    # colsum against the kernel's own rows
    cs_ref = dpar.double().sum(1)
    _within(colsum, cs_ref, 1024 * EPS * dpar.double().abs().sum(1) + 1e-30, "colsum")
    # every row against float64 autograd (chunks of rows: the float64 graph of 64 x 64 x 100 x 16 values is ~5 GB)
    worst, chunk = 0.0, 16 if S == 64 else 48
    for r0 in range(0, rows, chunk):
        r1 = min(rows, r0 + chunk)
        lc = l[r0:r1].double().requires_grad_(True)
        val = O.dlm_nll(lc, x[r0:r1].double(), hp)                                    # [rows, S, S]
        per_row = val.sum((1, 2))
        (gl,) = torch.autograd.grad((per_row * w[r0:r1].double() * scale).sum(), lc)
        ref = _to_kernel(gl, perm)
        cond = _to_kernel(_tail_bound(lc.detach(), x[r0:r1].double(), gl, w[r0:r1].double() * scale, hp), perm)
        got = dpar[r0:r1].double()
        rmax = ref.abs().flatten(1).max(1).values[:, None, None]
        worst = max(worst, _within(got, ref, 5e-5 * rmax + 2e-4 * ref.abs() + cond, f"d nll / d params rows {r0}..{r1}"))
        live = w[r0:r1] != 0
        want_nll = torch.where(live, per_row.detach(), torch.zeros_like(per_row.detach()))
        _within(nll[r0:r1], want_nll, 1e-4 * want_nll.abs(), f"nll_out rows {r0}..{r1}")
    print(f"dlm_nll_bwd S={S} rows={rows}: worst err / tol {worst:.3f}")


def _dlm_mean_params(rows, S, g, dev):
    l = _dlm_params(rows, S, g, dev, edges=False)
    nm, h = 10, S // 4
    rest = l[:, nm:].view(rows, 3, 3 * nm, S, S)
    l[0::3, :nm] *= 25.0                                             # sharp
    l[1::3, :nm] *= 0.01                                             # flat
    rest[:, :, 2 * nm:, :h] *= 12.0                                  # saturated tanh coefficients
    rest[:, :, :nm, h:2 * h] = 1.6                                   # mixture mean above +1 in every colour: the clamp blocks the gradient
    rest[:, :, :nm, 2 * h:3 * h, :h] = -1.7                          # below -1
    return l


@pytest.mark.parametrize("used", [112, 80])
def test_dlm_mean_bwd_vs_float64(env, used):
    """gcpx_dlm_mean_bwd as the adaptive model's backward calls it (backward_plan.py:81: rows = B N, pitch 112, used_slots 112, or
    8 n_mix = 80 for the lean head backward) against autograd in float64 of oracle.dlm_mean.  Pixels whose mixture mean lies outside
    [-1, 1] (the clamp blocks the gradient; colour values within 1e-4 of the clamp's edge, where f32 and float64 may disagree on the
    side, get a zero upstream gradient), sharp / flat logits, saturated colour coefficients.  used_slots = 80: slots >= 80 of
    dparams keep the NaN and colsum's slots >= 80 are 0; in both variants slot 7 of every mixture (log_scale_r) is 0.
    Tolerance: 2e-6 of the row's largest + 2e-5 relative.  The kernel uses the hardware exp / rcp (1-2 ulp) and tanh as
    1 - 2 / (exp(2x) + 1), whose absolute error is ~2 eps (relative error large only where tanh is ~0, where the products it enters
    are small too); each gradient value is a chain of <= 6 such roundings over a softmax of 10 terms: ~30 eps = 2e-6 of the largest
    value of a pixel, and the row's largest bounds the pixel's.  colsum: sums of npix / 4 values per lane, 256 eps of the abs-terms."""
    rt, pk, lib, dev = env
    from oracle import gcp_model_oracle as O
    from video_gcp_amd import config
    hp = config("c5")
    S, rows = 64, 270
    g = torch.Generator(device=dev).manual_seed(used)
    perm, inv = _inv_perm(pk)
    l = _dlm_mean_params(rows, S, g, dev)
    params = _to_kernel(l, perm).contiguous()
    if used == 80:
        params[..., 80:] = NAN                                       # not read in this variant
    dimg = torch.randn(rows, 3, S, S, device=dev, generator=g) * 1e-3
    with torch.no_grad():                                            # the unclamped mean (oracle.dlm_mean before its clamp), float64
        lg, means, _, cf = O.dlm_split(l.double(), hp)
        pi = torch.softmax(lg, 1)
        m_r = means[:, 0]
        m_g = means[:, 1] + cf[:, 0] * m_r
        m_b = means[:, 2] + cf[:, 1] * m_r + cf[:, 2] * m_g
        raw = torch.stack([(pi * m_r).sum(1), (pi * m_g).sum(1), (pi * m_b).sum(1)], 1)
        dimg[((raw.abs() - 1).abs() < 1e-4)] = 0.0                   # within rounding of the clamp's edge: no upstream gradient
        del lg, means, cf, pi, m_r, m_g, m_b
    P, npix = len(perm), S * S
    dpar = _nan(rows, npix, P)
    colsum = _nan(rows, P)
    rt.check(lib.gcpx_dlm_mean_bwd(params.data_ptr(), dimg.data_ptr(), dpar.data_ptr(), colsum.data_ptr(), rows, npix, P, 10, used,
                                   _st()), "dlm_mean_bwd")
    torch.cuda.synchronize()
    if used == 80:
        _untouched(dpar[..., 80:], "dparams slots >= 80")
        assert bool((colsum[:, 80:] == 0).all())
    else:
        assert bool((dpar[..., 80:] == 0).all())
    assert bool((dpar[..., 7:80:8] == 0).all()), "slot 7 of every mixture (log_scale_r) must be 0"
    got = dpar[..., :used].double()
    _within(colsum[:, :used], got.sum(1), 256 * EPS * got.abs().sum(1) + 1e-30, "colsum")
    worst = 0.0
    blocked = 0
    for r0 in range(0, rows, 30):
        r1 = min(rows, r0 + 30)
        lc = l[r0:r1].double().requires_grad_(True)
        img = O.dlm_mean(lc, hp)
        (gl,) = torch.autograd.grad((img * dimg[r0:r1].double()).sum(), lc)
        ref = _to_kernel(gl, perm)[..., :used]
        rmax = ref.abs().flatten(1).max(1).values[:, None, None]
        worst = max(worst, _within(got[r0:r1], ref, 2e-6 * rmax + 2e-5 * ref.abs(), f"d mean / d params rows {r0}..{r1}"))
        blocked += int(((img.detach().abs() >= 1.0)).sum())
    assert blocked > 0, "no pixel outside [-1, 1]: the clamp was not exercised"
    print(f"dlm_mean_bwd used={used}: worst err / tol {worst:.3f}; {blocked} clamped colour values")


def test_gather_rows_matched_distr(env):
    """gcpx_gather_rows as the stored-parameters path gathers the matched frames' parameters (forward_plan.py:707): out[b][t] =
    src[b][idx[b][t]] for rows of S S 112 floats, rows with idx < 0 (padded frames) zero-filled.  Exact copy."""
    rt, pk, lib, dev = env
    g = torch.Generator(device=dev).manual_seed(3)
    B, N, T, RF = 3, 15, 9, 16 * 16 * 112
    src = torch.randn(B, N, RF, device=dev, generator=g)
    idx = torch.randint(0, N, (B, T), device=dev, generator=g, dtype=torch.int32)
    idx[1, 4:] = -1
    idx[2, 0] = -1
    out = _nan(B, T, RF)
    rt.check(lib.gcpx_gather_rows(src.data_ptr(), idx.data_ptr(), out.data_ptr(), B, T, N, 0, RF, _st()), "gather_rows")
    torch.cuda.synchronize()
    want = torch.where((idx >= 0)[..., None], src.gather(1, idx.clamp_min(0).long()[..., None].expand(B, T, RF)), 0.0)
    assert torch.equal(out, want)


# ------------------------------------------------------------------------------------------------------------------------------
# d. attention backward (csrc/adaptive.hip)
# ------------------------------------------------------------------------------------------------------------------------------
def _attn_ref(q, k, v, end, temp, rpb):
    """single-head core of oracle.adaptive_oracle.multihead_attention (identity projections) in float64 on the rows' own keys"""
    M, T = q.shape[0], k.shape[1]
    kr, vr = k.repeat_interleave(rpb, 0), v.repeat_interleave(rpb, 0)
    er = end.repeat_interleave(rpb, 0)
    score = torch.einsum("rd,rtd->rt", q, kr) / math.sqrt(q.shape[1]) / temp
    outside = torch.arange(T, device=q.device)[None] > er[:, None]
    score = score.masked_fill(outside, float("-inf"))
    a = torch.softmax(score, -1)
    return torch.einsum("rt,rtd->rd", a, vr), a, score


@pytest.mark.parametrize("shape,rpb,temp", [("c5s", 1, 1.0), ("c5s", 3, 0.02), ("c5s32", 8, 1.0), ("c5", 16, 1.0), ("c5", 7, 0.02)])
def test_attention_bwd_vs_float64(env, shape, rpb, temp):
    """gcpx_attention (forward weights `att`) and gcpx_attention_bwd as backward_stages.py:263 calls them: dK / dV written into one
    level's column block of [B T][n_levels dk] / [B T][n_levels nz] buffers (ldk, ldv wider than dk, nz: the other blocks keep the NaN),
    dtemp_row summed over rows = d / d temperature.  Shapes: c5s (dk 32, nz 128 and 32, T 12), c5 (dk 32, nz 128, T 200).  end_ind
    ragged, including 0, T - 1 and past T - 1.  Temperature 1 and 0.02 (sharp softmax).  Against autograd in float64 of the single-head
    core of oracle.adaptive_oracle.multihead_attention (the test checks the core against that function).
    Tolerances (abs-terms in float64): a score is a dk-term dot, within 32 eps of its abs-terms |q||k| / sqrt(dk) / temp; a softmax
    weight moves with every score of its row, so att is within (64 max |score|-abs-terms + 8) eps relative, plus 2^-125 where the
    exponential underflows (sharp temperature: weights of 1e-70 are 0 in f32); the dk-term, T-term and rpb-term sums of
    the backward add their counts: dq, dK, dV, dS, d temp within (dk + nz + T + rpb + 8) eps x (1 + |score|-abs-terms) of their own
    abs-terms."""
    rt, pk, lib, dev = env
    from oracle import adaptive_oracle as A
    import video_gcp_amd as V
    dk, nz, T = {"c5s": (32, 128, 12), "c5s32": (32, 32, 12), "c5": (32, 128, 200)}[shape]
    B = 5
    M = B * rpb
    g = torch.Generator(device=dev).manual_seed(rpb * T)
    q = torch.randn(M, dk, device=dev, generator=g)
    k = torch.randn(B, T, dk, device=dev, generator=g)
    v = torch.randn(B, T, nz, device=dev, generator=g)
    end = torch.tensor([T - 1, 0, T // 2, T + 3, 1], device=dev)
    tmp = torch.tensor([temp], device=dev)
    dout = torch.randn(M, nz, device=dev, generator=g)
    out, att = _nan(M, nz), _nan(M, T)
    rt.check(lib.gcpx_attention(q.data_ptr(), k.data_ptr(), v.data_ptr(), None, end.data_ptr(), tmp.data_ptr(), out.data_ptr(),
                                att.data_ptr(), M, rpb, T, dk, nz, 1, _st()), "attention")
    nlev, li = 3, 1
    dS, dq, dtr = _nan(M, T), _nan(M, dk), _nan(M)
    dKb, dVb = _nan(B * T, nlev * dk), _nan(B * T, nlev * nz)
    rt.check(lib.gcpx_attention_bwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), att.data_ptr(), dout.data_ptr(), end.data_ptr(),
                                    tmp.data_ptr(), dS.data_ptr(), dq.data_ptr(), dtr.data_ptr(), dKb.data_ptr() + 4 * li * dk,
                                    nlev * dk, dVb.data_ptr() + 4 * li * nz, nlev * nz, M, rpb, T, dk, nz, _st()), "attention_bwd")
    torch.cuda.synchronize()
    for j in range(nlev):
        if j != li:
            _untouched(dKb[:, j * dk:(j + 1) * dk], f"dK block {j}")
            _untouched(dVb[:, j * nz:(j + 1) * nz], f"dV block {j}")
    dK, dV = dKb[:, li * dk:(li + 1) * dk].reshape(B, T, dk), dVb[:, li * nz:(li + 1) * nz].reshape(B, T, nz)
    # reference
    q64, k64, v64 = (t.double().requires_grad_(True) for t in (q, k, v))
    t64 = tmp.double().requires_grad_(True)
    o64, a64, s64 = _attn_ref(q64, k64, v64, end, t64, rpb)
    s64.retain_grad()
    (o64 * dout.double()).sum().backward()
    with torch.no_grad():                                            # the core is oracle.multihead_attention's (one head, identity projections)
        hp = V.config("c5s", n_attention_heads=1, nz_attn_key=dk, nz_enc=nz)
        sd = {}
        for nm_, d in (("q_proj", dk), ("k_proj", dk), ("v_proj", nz), ("out_proj", nz)):
            sd[f"a.{nm_}.weight"], sd[f"a.{nm_}.bias"] = torch.eye(d, dtype=torch.float64), torch.zeros(d, dtype=torch.float64)
        sd["a.temperature"] = tmp.double().cpu()
        rep = lambda t: t.repeat_interleave(rpb, 0)
        wo, wa = A.multihead_attention(sd, "a", hp, q.double().cpu(), rep(k.double().cpu()), rep(v.double().cpu()),
                                       torch.zeros(M, dtype=torch.long), rep(end.cpu()))
        assert torch.allclose(wo, o64.cpu(), rtol=1e-12, atol=1e-12) and torch.allclose(wa, a64.cpu(), rtol=1e-12, atol=1e-12)
        # abs-terms
        sabs = torch.einsum("rd,rtd->rt", q64.abs(), k64.abs().repeat_interleave(rpb, 0)) / math.sqrt(dk) / temp
        inside = a64 > 0
        cs = (1 + sabs) * inside
        n_sum = dk + nz + T + rpb + 8
        dA = torch.einsum("rd,rtd->rt", dout.double().abs(), v64.abs().repeat_interleave(rpb, 0))
        dS_abs = a64 * (dA + (a64 * dA).sum(1, keepdim=True)) * cs.amax(1, keepdim=True)
        dq_abs = torch.einsum("rt,rtd->rd", dS_abs, k64.abs().repeat_interleave(rpb, 0)) / math.sqrt(dk) / temp
        dK_abs = torch.einsum("rt,rd->rtd", dS_abs, q64.abs()).reshape(B, rpb, T, dk).sum(1) / math.sqrt(dk) / temp
        dV_abs = torch.einsum("rt,rd->rtd", a64 * cs, dout.double().abs()).reshape(B, rpb, T, nz).sum(1)
        dt_abs = (dS_abs * sabs.masked_fill(~inside, 0)).sum() / temp
    smax = sabs.masked_fill(~inside, 0).amax(1, keepdim=True)
    tiny = 2.0 ** -125                                               # expf underflows (flushes) below the f32 normal range
    w = [_within(att, a64.detach(), (64 * smax + 8) * EPS * a64.detach() + tiny, "att (forward weights)")]
    w.append(_within(dS, s64.grad, n_sum * EPS * dS_abs + tiny * (dA + (a64 * dA).sum(1, keepdim=True)), "dS"))
    w.append(_within(dq, q64.grad, n_sum * EPS * dq_abs + 1e-30, "dq"))
    w.append(_within(dK, k64.grad, n_sum * EPS * dK_abs + 1e-30, "dK"))
    w.append(_within(dV, v64.grad, n_sum * EPS * dV_abs + 1e-30, "dV"))
    dtemp = dtr.double().sum()
    w.append(_within(dtemp[None], t64.grad, (M + n_sum) * EPS * dt_abs[None], "d temperature (sum of dtemp_row)"))
    print(f"attention_bwd {shape} rpb={rpb} temp={temp}: worst err / tol {max(w):.3f}")


# ------------------------------------------------------------------------------------------------------------------------------
# e. averaging-criterion backward
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,near_opt", [("c5s", False), ("c5s", True), ("c5", False), ("c5", True)])
def test_averaging_nll_bwd_vs_float64(env, shape, near_opt):
    """gcpx_averaging_nll_bwd as backward_plan.py:65 calls it (coef = dense_img_rec_weight / (B prod(traj.shape[1:])), dlog_sigma
    ACCUMULATED into the gradient: prefilled here) against autograd in float64 of oracle.adaptive_oracle.averaging_loss (x B x coef),
    dsum the squared distances of the same images (what the forward's cdist produced).  c5s: N 15, T 12, 3 x 32 x 32; c5: N 255,
    T 200, 3 x 64 x 64; B 3 with a ragged pad mask (one sequence padded from frame 1).  near_opt: sigma^2 = the weighted mean squared
    distance per dimension, where d loss / d log sigma = coef sum w pad (D - dsum exp(-2 ls)) cancels to ~0.
    Tolerances: dimg (T + 4) eps of its abs-terms coef exp(-2 ls) (|img| sum wp + sum wp |traj|) (a T-term f32 MFMA sum and 4
    roundings); d log sigma (B N T / 4096 + 1024 + 16) eps of sum |terms| = coef sum w pad (D + dsum exp(-2 ls)): 1024 threads
    x 4 accumulators each sum B N T / 4096 terms, then a 1024-way tree; dsum is read in f32, one more eps — the bound is relative to
    the terms, not to the cancelled result."""
    rt, pk, lib, dev = env
    from oracle import adaptive_oracle as A
    from video_gcp_amd import config
    hp = config("c5s" if shape == "c5s" else "c5")
    B = 3
    N, T, S = (15, 12, 32) if shape == "c5s" else (255, 200, 64)
    D = 3 * S * S
    g = torch.Generator(device=dev).manual_seed(N + T + int(near_opt))
    traj = torch.rand(B, T, D, device=dev, generator=g) * 2 - 1
    end = torch.tensor([T - 1, 1, T // 2], device=dev)
    pad = (torch.arange(T, device=dev)[None] <= end[:, None]).float()
    traj = traj * pad[..., None]
    img = torch.rand(B, N, D, device=dev, generator=g) * 2 - 1
    w = torch.rand(B, N, T, device=dev, generator=g) ** 4
    w = w / w.sum(1, keepdim=True)
    dsum64 = A.batch_cdist(img.double(), traj.double())
    dsum = dsum64.float()
    if near_opt:
        wp = w.double() * pad[:, None]
        ls0 = 0.5 * math.log(float((wp * dsum.double()).sum() / (D * wp.sum())))
    else:
        ls0 = 0.3
    ls = torch.tensor([ls0], device=dev).float()
    coef = 1.0 / (B * T * D)
    dimg = _nan(B, N, D)
    pre = torch.tensor([0.625], device=dev)
    dls = pre.clone()
    rt.check(lib.gcpx_averaging_nll_bwd(w.data_ptr(), pad.data_ptr(), img.data_ptr(), traj.data_ptr(), dsum.data_ptr(), ls.data_ptr(),
                                        C.c_float(coef), B, N, T, D, dimg.data_ptr(), dls.data_ptr(), _st()), "averaging_nll_bwd")
    torch.cuda.synchronize()
    img64 = img.double().requires_grad_(True)
    sd = {"decoder.log_sigma": ls.double().requires_grad_(True)}
    val = A.averaging_loss(hp, sd, img64.view(B, N, 3, S, S), traj.double().view(B, T, 3, S, S), w.double(), pad.double()) * B * coef
    gi, gl = torch.autograd.grad(val, (img64, sd["decoder.log_sigma"]))
    with torch.no_grad():
        s2 = math.exp(-2 * float(ls))
        wp = w.double() * pad.double()[:, None]
        dimg_abs = coef * s2 * (img.double().abs() * wp.sum(2, keepdim=True) + torch.einsum("bnt,btd->bnd", wp, traj.double().abs()))
        dls_abs = coef * (wp * (D + dsum.double() * s2)).sum()
    w1 = _within(dimg, gi, (T + 4) * EPS * dimg_abs + 1e-30, "dimg")
    nt = B * N * T / 4096 + 1024 + 16
    w2 = _within(dls - pre.double(), gl.reshape(1), (nt * EPS * dls_abs + 2 * EPS * abs(float(pre))).reshape(1), "d log sigma (accumulated)")
    print(f"averaging_nll_bwd {shape} near_opt={near_opt}: d log sigma {float(gl):.3e} of abs-terms {float(dls_abs):.3e}; "
          f"worst err / tol {max(w1, w2):.3f}")


# ------------------------------------------------------------------------------------------------------------------------------
# f. KL and the reparametrised sample
# ------------------------------------------------------------------------------------------------------------------------------
def _kl_inputs(B, N, nz, bs, ns, free_nats, g, dev):
    """q / p rows [mu | log_sigma] at b bs + n ns + 2 nz (the planner's slot 1 onward) in NaN-filled buffers; per-dimension KL values
    on both sides of free_nats, none within 1e-3 of it (where f32 and float64 may take different sides of the clamp)"""
    q = _nan(B * bs + 4 * nz)
    p = _nan(B * bs + 4 * nz)
    mq = torch.randn(B, N, nz, device=dev, generator=g) * 1.2
    mp = torch.randn(B, N, nz, device=dev, generator=g) * 0.3
    lq = torch.randn(B, N, nz, device=dev, generator=g) * 0.5
    lp = torch.randn(B, N, nz, device=dev, generator=g) * 0.5
    for _ in range(8):
        kl = lp.double() - lq + (torch.exp(2 * lq.double()) + (mq.double() - mp) ** 2) / (2 * torch.exp(2 * lp.double())) - 0.5
        near = (kl - free_nats).abs() < 1e-3
        if not bool(near.any()):
            break
        mq = torch.where(near, mq + 0.05, mq)
    off = 2 * nz
    idx = (torch.arange(B, device=dev)[:, None, None] * bs + torch.arange(N, device=dev)[None, :, None] * ns + off +
           torch.arange(nz, device=dev)[None, None, :])
    q[idx], q[idx + nz], p[idx], p[idx + nz] = mq, lq, mp, lp
    return q, p, idx, (mq, lq, mp, lp)


@pytest.mark.parametrize("variant", ["plain", "weighted", "scheduled", "scheduled_weighted"])
@pytest.mark.parametrize("free_nats", [0.0, 1.0])
def test_kl_bwd_vs_float64(env, variant, free_nats):
    """gcpx_kl_bwd (backward_plan.py:102), gcpx_kl_bwd_scheduled (backward_plan.py:99: the burn-in weight read from device memory,
    no node weights; training_sequential.py:198: with them) and gcpx_kl_bwd_weighted (training_sequential.py:202: node weights
    pad_mask[:, 1:], zeros included) against autograd in float64 of the KL term of oracle.gcp_model_oracle.losses:
    coef (x device coefficient) x sum over (b, n, d) of weight[b][n] x clamp(KL, min=free_nats) (the flat model's form,
    gcp_sequential_oracle.py:162).  free_nats 0 and 1 (the reference's gcp_sequential setting: the per-dimension clamp).  Rows
    interleaved (node stride 2 rows, batch stride with a gap): the rows in between keep the NaN.
    Tolerance: 16 eps of each output's abs-terms (g |diff| exp(-2lp); g (exp(2lq - 2lp) + 1); g (1 + (exp(2lq) + diff^2) exp(-2lp)):
    two expf of 1 ulp, <= 6 roundings)."""
    rt, pk, lib, dev = env
    B, N, nz = 3, 7, 32
    ns, bs = 2 * (2 * nz), 2 * (2 * nz) * N + 6 * nz
    g = torch.Generator(device=dev).manual_seed(int(free_nats) * 10 + len(variant))
    q, p, idx, (mq, lq, mp, lp) = _kl_inputs(B, N, nz, bs, ns, free_nats, g, dev)
    coef = 0.37 / (B * 1000.0)
    T_ = N + 1
    nw = (torch.rand(B, T_, device=dev, generator=g) > 0.3).float() * (torch.rand(B, T_, device=dev, generator=g) + 0.5)
    nw[1, 3] = 0.0
    cdev = torch.tensor([0.55], device=dev)
    dq, dp = _nan(q.numel()), _nan(p.numel())
    o = 4 * 2 * nz                                                  # bytes to slot 1 (backward_plan.py: _addr(QZ, 2 nv))
    args = (q.data_ptr() + o, p.data_ptr() + o, dq.data_ptr() + o, dp.data_ptr() + o, B, N, nz, bs, ns, C.c_float(free_nats),
            C.c_float(coef))
    weighted = "weighted" in variant
    # node weights at offset 1 of a [B][T] row, as training_sequential passes pad_mask[:, 1:]
    wptr = nw.data_ptr() + 4 if weighted else None
    if variant == "plain":
        rt.check(lib.gcpx_kl_bwd(*args, _st()), "kl_bwd")
    elif variant == "weighted":
        rt.check(lib.gcpx_kl_bwd_weighted(*args, wptr, T_, _st()), "kl_bwd_weighted")
    else:
        rt.check(lib.gcpx_kl_bwd_scheduled(*args, wptr, T_ if weighted else 0, cdev.data_ptr(), _st()), "kl_bwd_scheduled")
    torch.cuda.synchronize()
    mask = torch.zeros(q.numel(), dtype=torch.bool, device=dev)
    mask[idx] = True
    mask[idx + nz] = True
    _untouched(dq[~mask], "dq gaps")
    _untouched(dp[~mask], "dp gaps")
    t = [x.double().requires_grad_(True) for x in (mq, lq, mp, lp)]
    kl = t[3] - t[1] + (torch.exp(2 * t[1]) + (t[0] - t[2]) ** 2) / (2 * torch.exp(2 * t[3])) - 0.5    # gcp_model_oracle.py:561-562
    kl = torch.clamp(kl, min=free_nats)
    wgt = nw[:, 1:N + 1].double()[..., None] if weighted else 1.0
    c = coef * (float(cdev) if variant.startswith("scheduled") else 1.0)
    grads = torch.autograd.grad((kl * wgt).sum() * c, t)
    with torch.no_grad():
        live = (kl > free_nats).double() * wgt * c
        diff = (mq - mp).double().abs()
        e2q, ie2p = torch.exp(2 * lq.double()), torch.exp(-2 * lp.double())
        ab = [live * diff * ie2p, live * (e2q * ie2p + 1), live * diff * ie2p, live * (1 + (e2q + diff ** 2) * ie2p)]
    got = [dq[idx], dq[idx + nz], dp[idx], dp[idx + nz]]
    names = ["d mu_q", "d log_sigma_q", "d mu_p", "d log_sigma_p"]
    w = max(_within(gv, rv, 16 * EPS * av + 1e-30, n) for gv, rv, av, n in zip(got, grads, ab, names))
    if free_nats > 0:
        assert bool((kl.detach() <= free_nats).any()) and bool((kl.detach() > free_nats).any()), "the clamp must be exercised"
    print(f"kl_bwd {variant} free_nats={free_nats}: worst err / tol {w:.3f}")


@pytest.mark.parametrize("with_dz1", [False, True])
def test_latent_bwd_vs_float64(env, with_dz1):
    """gcpx_latent_bwd as backward_plan.py:329 calls it for one tree level (rows (b, j) of the level at base + b pb + j prow in the
    interleaved position layout, eps rows strided, dz0 rows with a leading dimension wider than nz, dz1 NULL or set) against autograd
    in float64 of z = mu + exp(log_sigma) eps plus the gradients already accumulated at the q / p rows.
    Tolerance: dq_mu, dp exact up to one addition (2 eps of abs-terms); dq_log_sigma 6 eps of |dqz_pos| + |dz exp(ls) eps| (expf of 1 ulp
    and 4 roundings)."""
    rt, pk, lib, dev = env
    B, n, nz = 4, 4, 32
    M = B * n
    g = torch.Generator(device=dev).manual_seed(int(with_dz1))
    s = 3                                                           # level offset in slots (the planner's s = 2^l - 1)
    PS = 2 * n + s + 1
    pb, prow = PS * 2 * nz, 2 * 2 * nz                              # every other slot of the position layout
    QZ = torch.randn(B, PS, 2 * nz, device=dev, generator=g)
    dQZ = torch.randn(B, PS, 2 * nz, device=dev, generator=g)
    dPZ = torch.randn(B, PS, 2 * nz, device=dev, generator=g)
    Ne = 2 * n
    eps = torch.randn(B, Ne, nz, device=dev, generator=g)
    ld0, ld1 = 2 * nz + 16, 2 * nz + nz
    dz0 = torch.randn(M, ld0, device=dev, generator=g)
    dz1 = torch.randn(M, ld1, device=dev, generator=g) if with_dz1 else None
    dqo, dpo = _nan(M, 2 * nz), _nan(M, 2 * nz)
    base = s * 2 * nz
    rt.check(lib.gcpx_latent_bwd(dQZ.data_ptr() + 4 * base, dPZ.data_ptr() + 4 * base, QZ.data_ptr() + 4 * base, pb, prow,
                                 eps.data_ptr() + 4 * (n - 1) * nz, Ne * nz, nz, dz0.data_ptr() + 4 * 8, ld0,
                                 (dz1.data_ptr() + 4 * nz) if with_dz1 else None, ld1, dqo.data_ptr(), dpo.data_ptr(), M, n, nz,
                                 _st()), "latent_bwd")
    torch.cuda.synchronize()
    sl = s + 2 * torch.arange(n, device=dev)
    qrow = QZ[:, sl].reshape(M, 2 * nz).double().requires_grad_(True)
    prow_ = QZ.new_zeros(M, 2 * nz).double().requires_grad_(True)
    e = eps[:, n - 1:2 * n - 1].reshape(M, nz).double()
    dz = dz0[:, 8:8 + nz].double() + (dz1[:, nz:2 * nz].double() if with_dz1 else 0.0)
    z = qrow[:, :nz] + torch.exp(qrow[:, nz:]) * e
    dqp, dpp = dQZ[:, sl].reshape(M, 2 * nz).double(), dPZ[:, sl].reshape(M, 2 * nz).double()
    gq, gp = torch.autograd.grad((z * dz).sum() + (qrow * dqp).sum() + (prow_ * dpp).sum(), (qrow, prow_))
    ab = torch.cat([dqp[:, :nz].abs() + dz.abs(), dqp[:, nz:].abs() + (dz * torch.exp(qrow[:, nz:].detach()) * e).abs()], 1)
    _within(dqo[:, :nz], gq[:, :nz], 2 * EPS * ab[:, :nz] + 1e-30, "dq mu")
    _within(dqo[:, nz:], gq[:, nz:], 6 * EPS * ab[:, nz:] + 1e-30, "dq log_sigma")
    assert torch.equal(dpo.double(), gp), "dp is a copy of the accumulated prior-row gradient"


# ------------------------------------------------------------------------------------------------------------------------------
# g. loss heads
# ------------------------------------------------------------------------------------------------------------------------------
def _loss_args(rt, dev, g, B, T, N, sd_, with_state_mask, na=4):
    end = torch.randint(1, T, (B,), device=dev, generator=g)
    end[0] = T - 1
    pad = (torch.arange(T, device=dev)[None] <= end[:, None]).float()
    seq_len = (end + 1).int()
    t = dict(
        len_logits=torch.randn(B, T, device=dev, generator=g) * 3,
        end=end, pad=pad, seq_len=seq_len,
        exist=torch.randn(B, N, device=dev, generator=g) * 4,
        leave=(torch.rand(B, N, device=dev, generator=g) > 0.5).int(),
        rs=torch.randn(B, T, sd_, device=dev, generator=g), ts=torch.randn(B, T, sd_, device=dev, generator=g),
        smask=pad.clone(),
        ap=torch.randn(B, na, device=dev, generator=g), aseq=torch.randn(B, T - 1, na, device=dev, generator=g),
        inv_t0=torch.randint(0, T - 2, (B,), device=dev, generator=g),
        cp=torch.randn(B, device=dev, generator=g), ct=torch.randn(B, device=dev, generator=g) * 2,
    )
    t["smask"][:, 0] = 1.0
    t["smask"][1, 1] = 0.0
    la = rt.LossArgs()
    la.pad_mask, la.len_logits, la.end_ind, la.existence, la.leave = (t["pad"].data_ptr(), t["len_logits"].data_ptr(), end.data_ptr(),
                                                                       t["exist"].data_ptr(), t["leave"].data_ptr())
    la.regressed_state, la.state_target, la.seq_len = t["rs"].data_ptr(), t["ts"].data_ptr(), seq_len.data_ptr()
    la.B, la.T, la.N, la.state_dim = B, T, N, sd_
    la.w_rec, la.w_kl, la.w_len, la.w_exist, la.w_state, la.total_div = 1.0, 1.0, 0.7, 1.3, 0.9, float(T * 3 * 32 * 32)
    la.action_pred, la.action_seq, la.inv_t0 = t["ap"].data_ptr(), t["aseq"].data_ptr(), t["inv_t0"].data_ptr()
    la.cost_pred, la.cost_target, la.n_actions, la.w_action, la.w_cost = t["cp"].data_ptr(), t["ct"].data_ptr(), na, 1.7, 0.8
    la.state_mask = t["smask"].data_ptr() if with_state_mask else None
    return la, t


@pytest.mark.parametrize("T,with_state_mask", [(20, False), (20, True), (33, True)])
def test_loss_heads_bwd_vs_float64(env, T, with_state_mask):
    """gcpx_loss_heads_bwd as backward_plan.py:110 (length, existence, state) and training_sequential.py:209 (dexist NULL, state_mask
    set: the flat model's regression weights) call it, against autograd in float64 of the oracle.gcp_model_oracle.losses terms:
    F.cross_entropy(len_logits, end_ind), F.binary_cross_entropy_with_logits(existence, leave), mean of (regressed - target)^2 x mask
    over (B, max seq_len, state_dim), each x its weight / total_div.  Layouts: dlen [B][ceil16(T)], dexist [B N][16] (column 0),
    dstate [B T][16] (columns < state_dim, frames < max seq_len): every padding column / row is written as 0.
    Tolerance: 4 T eps of |dlen|'s abs-terms (softmax over T terms with expf); 8 eps of the abs-terms of the differences
    sigmoid(x) - target and regressed - target for the two element-wise heads."""
    rt, pk, lib, dev = env
    B, N, sd_ = 3, 31, 5
    g = torch.Generator(device=dev).manual_seed(T + int(with_state_mask))
    la, t = _loss_args(rt, dev, g, B, T, N, sd_, with_state_mask)
    ldl = (T + 15) // 16 * 16
    dlen, dexist, dstate = _nan(B, ldl), _nan(B * N, 16), _nan(B * T, 16)
    rt.check(lib.gcpx_loss_heads_bwd(C.byref(la), dlen.data_ptr(), dexist.data_ptr(), dstate.data_ptr(), _st()), "loss_heads_bwd")
    # the flat model's call: no existence head output
    dlen2, dstate2 = _nan(B, ldl), _nan(B * T, 16)
    rt.check(lib.gcpx_loss_heads_bwd(C.byref(la), dlen2.data_ptr(), None, dstate2.data_ptr(), _st()), "loss_heads_bwd (no dexist)")
    torch.cuda.synchronize()
    assert torch.equal(dlen2, dlen) and torch.equal(dstate2, dstate)
    div = float(la.total_div)
    ll = t["len_logits"].double().requires_grad_(True)
    ex = t["exist"].double().requires_grad_(True)
    rs = t["rs"].double().requires_grad_(True)
    rl = int(t["seq_len"].max())
    m = (t["smask"] if with_state_mask else t["pad"]).double()
    total = (float(la.w_len) * F.cross_entropy(ll, t["end"]) +
             float(la.w_exist) * F.binary_cross_entropy_with_logits(ex, t["leave"].double()) +
             float(la.w_state) * ((rs[:, :rl] - t["ts"].double()[:, :rl]) ** 2 * m[:, :rl, None]).mean()) / div
    gl, ge, gs = torch.autograd.grad(total, (ll, ex, rs))
    assert bool((dlen[:, T:] == 0).all()), "length padding columns"
    assert bool((dexist[:, 1:] == 0).all()), "existence padding columns"
    ds = dstate.view(B, T, 16)
    assert bool((ds[..., sd_:] == 0).all()) and bool((ds[:, rl:] == 0).all()), "state padding columns / frames"
    with torch.no_grad():                                            # abs-terms: p + target of p - target, |a| + |b| of a - b
        ke = float(la.w_exist) / (div * B * N)
        ex_abs = ke * (torch.sigmoid(ex) + t["leave"].double())
        ks = 2 * float(la.w_state) / (div * B * rl * sd_)
        st_abs = torch.zeros_like(gs)
        st_abs[:, :rl] = ks * (rs[:, :rl].abs() + t["ts"].double()[:, :rl].abs()) * m[:, :rl, None]
    _within(dlen[:, :T], gl, 4 * T * EPS * (gl.abs() + gl.abs().max(1, keepdim=True).values) + 1e-30, "dlen")
    _within(dexist[:, 0].view(B, N), ge, 8 * EPS * ex_abs, "dexist")
    _within(ds[..., :sd_], gs, 8 * EPS * st_abs + 1e-30, "dstate")


def test_loss_aux_heads_bwd_vs_float64(env):
    """gcpx_loss_aux_heads_bwd as backward_plan.py:135 / training_sequential.py:219 call it: the inverse model's L2 head (prediction
    against actions[b][inv_t0[b]]) and the cost model's, against autograd in float64 of the oracle's l2_loss terms (aux_models_oracle)
    x weight / total_div.  daction [B][16] (columns >= n_actions written 0), dcost [B][16] (column 0).  Tolerance 8 eps relative
    (one difference and three products)."""
    rt, pk, lib, dev = env
    from oracle import aux_models_oracle as AX
    B, T, na = 5, 12, 4
    g = torch.Generator(device=dev).manual_seed(5)
    la, t = _loss_args(rt, dev, g, B, T, 7, 3, False, na=na)
    da, dc = _nan(B, 16), _nan(B, 16)
    rt.check(lib.gcpx_loss_aux_heads_bwd(C.byref(la), da.data_ptr(), dc.data_ptr(), _st()), "loss_aux_heads_bwd")
    torch.cuda.synchronize()
    ap, cp = t["ap"].double().requires_grad_(True), t["cp"].double().requires_grad_(True)
    tgt = t["aseq"].double()[torch.arange(B, device=dev), t["inv_t0"]]
    div = float(la.total_div)
    total = (float(la.w_action) * AX.l2_loss(ap, tgt) + float(la.w_cost) * AX.l2_loss(cp, t["ct"].double())) / div
    ga, gc = torch.autograd.grad(total, (ap, cp))
    assert bool((da[:, na:] == 0).all()) and bool((dc[:, 1:] == 0).all()), "padding columns"
    _within(da[:, :na], ga, 8 * EPS * ga.abs() + 1e-30, "daction")
    _within(dc[:, 0], gc, 8 * EPS * gc.abs() + 1e-30, "dcost")


# ------------------------------------------------------------------------------------------------------------------------------
# h. GroupNorm + LeakyReLU backward of the Predictor MLPs
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C_,cpg", [(32, 1), (32, 4), (32, 16), (128, 2), (128, 8), (128, 16)])
@pytest.mark.parametrize("M", [1, 7, 8, 9, 1000])
def test_gn_lrelu_bwd_vs_float64(env, C_, cpg, M):
    """gcpx_gn_lrelu_bwd + gcpx_reduce_partials as backward_ops._mlp_bwd / _gn_param_grads call them (backward_ops.py:325, :354: one
    reduction over the 2 C columns of the partials when gamma and beta are neighbours) against autograd in float64 of F.group_norm +
    F.leaky_relu(0.2) (the group statistics written out: torch's group_norm refuses one value per group at M = 1).  M = 1, 7, 8, 9,
    1000 rows (8 rows per workgroup: a partial last block and a block of one row), a constant row
    (variance 0: rstd = 1 / sqrt(eps)), channels per group 1..16.  Elements whose pre-activation lies within 1e-4 of the kink get a zero
    upstream gradient (their derivative is rounding-defined and then irrelevant).
    Tolerance: du within (cpg + 16 + 4 |mean| rstd) eps of its abs-terms rstd (|dxh| + mean|dxh| + |xh| (mean|dxh xh| + mean|dxh|))
    (group sums of cpg terms, rsqrt of 1 ulp, <= 8 roundings; x - mean loses |mean| rstd eps when a group's spread is small against
    its mean, which x_hat, rstd and both group means inherit); d gamma / d beta within (M / 16 + 40) eps of sum |dy xh| / sum |dy| (per-wave sums of 2 rows,
    4 waves, then the 16-way strided reduction over M / 8 blocks)."""
    rt, pk, lib, dev = env
    from video_gcp_amd import config
    hp = config("c1")
    groups = C_ // cpg
    g = torch.Generator(device=dev).manual_seed(M * 7 + C_ + cpg)
    u = torch.randn(M, C_, device=dev, generator=g) * 2 + 0.3
    u[M // 2] = 0.75                                               # constant row
    gamma = torch.rand(C_, device=dev, generator=g) + 0.5
    beta = torch.randn(C_, device=dev, generator=g) * 0.5
    da = torch.randn(M, C_, device=dev, generator=g)
    u64 = u.double().requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    ug64 = u64.view(M, groups, cpg)
    xh64 = (ug64 - ug64.mean(-1, keepdim=True)) / torch.sqrt(ug64.var(-1, unbiased=False, keepdim=True) + hp.gn_eps)
    y = xh64.reshape(M, C_) * g64 + b64
    da[(y.detach().abs() < 1e-4)] = 0.0
    a = F.leaky_relu(y, 0.2)
    gu, gg, gb = torch.autograd.grad((a * da.double()).sum(), (u64, g64, b64))
    nb = lib.gcpx_gn_bwd_blocks(M)
    du, part = _nan(M, C_), _nan(nb, 2, C_)
    rt.check(lib.gcpx_gn_lrelu_bwd(u.data_ptr(), da.data_ptr(), gamma.data_ptr(), beta.data_ptr(), du.data_ptr(), part.data_ptr(), M, C_,
                                   groups, C.c_float(hp.gn_eps), C.c_float(0.2), _st()), "gn_lrelu_bwd")
    dgb = _nan(2 * C_ + 8)
    rt.check(lib.gcpx_reduce_partials(part.data_ptr(), nb, 2 * C_, 2 * C_, dgb.data_ptr(), 0, _st()), "reduce_partials")
    torch.cuda.synchronize()
    _untouched(dgb[2 * C_:], "past the reduced columns")
    with torch.no_grad():
        ug = u.double().view(M, groups, cpg)
        mu = ug.mean(-1, keepdim=True)
        var = ug.var(-1, unbiased=False, keepdim=True)
        rstd = 1.0 / torch.sqrt(var + hp.gn_eps)
        xh = (ug - mu) * rstd
        dy = (da.double() * torch.where(y > 0, 1.0, 0.2)).view(M, groups, cpg)
        dxh = dy * gamma.double().view(groups, cpg)
        ab = rstd * (dxh.abs() + dxh.abs().mean(-1, keepdim=True) +
                     xh.abs() * ((dxh * xh).abs().mean(-1, keepdim=True) + dxh.abs().mean(-1, keepdim=True)))
        cond = 4 * mu.abs() * rstd                                   # x - mean: a rounding of |mean| against the spread 1 / rstd
        gsum_abs, bsum_abs = (dy * xh).abs().sum(0).flatten(), dy.abs().sum(0).flatten()
        gsum_c = (dy.abs() * cond).sum(0).flatten()
    _within(du, gu, ((cpg + 16 + cond) * EPS * ab).view(M, C_) + 1e-30, "du")
    ns = M / 16 + 40
    # (+ 1e-12 of sum |dy|: float64 autograd leaves ~1e-16 where x_hat is exactly 0 — one channel per group, the constant row)
    _within(dgb[:C_], gg, ns * EPS * gsum_abs + EPS * gsum_c + 1e-12 * bsum_abs + 1e-30, "d gamma")
    _within(dgb[C_:2 * C_], gb, ns * EPS * bsum_abs + 1e-30, "d beta")


def _gamma(n):
    """n roundings: (1 + eps)^n - 1 <= n eps / (1 - n eps)"""
    return n * EPS / (1.0 - n * EPS)


def _same_bits(got, want, name):
    """bit-for-bit equality of two f32 / int32 buffers, NaN sentinels included (an untouched NaN keeps its bits)"""
    a, b = got.contiguous().view(torch.int32), want.contiguous().view(torch.int32)
    if not torch.equal(a, b):
        bad = torch.nonzero((a != b).flatten())[:, 0]
        i = int(bad[0])
        raise AssertionError(f"{name}: {len(bad)}/{a.numel()} elements differ in their bits; first at flat index {i}: got "
                             f"{float(got.flatten()[i])} want {float(want.flatten()[i])}")


# ------------------------------------------------------------------------------------------------------------------------------
# i. LSTM cell backward (csrc/common.h: lstm_bwd_cell, launched by gcpx_lstm_bwd)
# ------------------------------------------------------------------------------------------------------------------------------
# (M, H, rpb, layout, inputs left NULL, scale of the pre-activations)
_LSTM = [
    (1, 64, 1, "flat", (), 1.0),
    (37, 64, 3, "tree", (), 1.0),
    (37, 128, 3, "tree", ("dh_dense",), 12.0),
    (37, 128, 8, "tree", ("dh_pos",), 1.0),
    (1000, 128, 8, "tree", ("dc_pos",), 12.0),
    (1000, 256, 8, "tree", (), 12.0),
    (37, 256, 1, "tree", (), 1.0),
    (37, 64, 1, "flat", (), 12.0),
    (37, 128, 1, "flat", ("dh_pos", "dc_pos"), 1.0),
    (1000, 64, 1, "flat", (), 1.0),
]


@pytest.mark.parametrize("M,H,rpb,layout,nulls,scale", _LSTM)
def test_lstm_bwd_vs_float64(env, M, H, rpb, layout, nulls, scale):
    """gcpx_lstm_bwd against float64 autograd of c = f c_prev + i g, h = o tanh(c) for the loss sum h (dh_dense + dh_pos) + sum c dc_pos.
    The kernel is handed what the forward stores — the activated gates rounded to f32 in the [M][H][4] (i, f, g, o) layout and c rounded
    to f32 — so the reference differentiates the cell with respect to the stored activations by autograd (c pinned to the stored value)
    and multiplies by s (1 - s) / 1 - t^2 evaluated at those stored values in float64: the function the backward differentiates.
    Layouts: "tree" (backward_plan.py:203-213): rows (b, j) of a level in the position layout of Hid / dHid (pb, prow larger than the
    rows they address, layer 1 of 2: c at column 3H, d h at 2H, d c at 3H of a 4H-wide slot), c_prev / dc_prev at column 3H of the 4H-wide
    merged / dmerged rows; "flat" (training_sequential.py:130-142): rpb 1, pitch 2H with prow 0, dh_dense rows of stride 2H, dc_prev
    written over dc_pos in place.  Every input element the kernel must not read is NaN (a stray read poisons an output), the gaps of
    dc_prev's buffer must keep their NaN.  Each of dh_dense / dh_pos / dc_pos NULL in turn (and both recurrent terms, the flat model's
    last step).  M H not a multiple of 256 except at H = 256.  Saturation: pre-activations at scale 12, planted gates of exactly 0, 1,
    -1 and stored |c| up to 20 (tanh' underflows): those gradients are exactly 0 or tiny and finite.
    Tolerance, per element, 18 eps x abs-terms + 2^-125, counted from lstm_bwd_cell: dh = dh_above + dh_pos rounds once (1); tanhf is
    within 2 ulp = 4 eps, so t^2 is within 9 eps of itself and q = 1 - t^2 within 10 eps of its abs-terms 1 + t^2; dh o q adds two
    products: 13 eps of A_dh o (1 + t^2) with A_dh = |dh_above| + |dh_pos|; adding dc_pos: dc within 14 eps of A_dc = |dc_pos| + A_dh o
    (1 + t^2).  di = dc g i (1 - i): three products and the subtraction of a stored value from 1 (one relative rounding): 18 eps of
    A_dc |g| i (1 - i); df likewise with c_prev; dg = dc i (1 - g^2): 17 eps of A_dc i (1 + g^2); do = dh t o (1 - o): 9 eps of
    A_dh |t| o (1 - o); dc_prev = dc f: 15 eps of A_dc f.  2^-125: products below the normal range may flush.
    The GEMM-epilogue form (gcpx_gemm_args.lstm_bwd) runs the same device function on the same values:
    test_gemm_lstm_bwd_epilogue_equals_separate_launch (test_gpu_kernels.py) holds it bit for bit to this kernel, which carries this
    result over to it."""
    rt, pk, lib, dev = env
    g = torch.Generator(device=dev).manual_seed(M * 131 + H + 7 * rpb + int(scale))
    pre = torch.randn(4, M, H, device=dev, generator=g) * scale
    p64 = pre.double()
    gates = torch.stack([torch.sigmoid(p64[0]), torch.sigmoid(p64[1]), torch.tanh(p64[2]), torch.sigmoid(p64[3])], -1).float().contiguous()
    cp = torch.randn(M, H, device=dev, generator=g) * (3.0 if scale > 1 else 1.0)
    flat_i = torch.arange(M * H, device=dev).view(M, H)
    # planted gates: every 8th element, six patterns in turn
    pat = torch.where(flat_i % 8 == 0, (flat_i // 8) % 6, torch.full_like(flat_i, -1))
    gates[..., 0][pat == 0] = 1.0
    gates[..., 0][pat == 1] = 0.0
    gates[..., 1][pat == 2] = 1.0
    gates[..., 3][pat == 2] = 0.0
    gates[..., 2][pat == 3] = 1.0
    gates[..., 2][pat == 4] = -1.0
    gates[..., 3][pat == 4] = 1.0
    gates[..., 1][pat == 5] = 0.0
    g64 = gates.double()
    c_new = (g64[..., 1] * cp.double() + g64[..., 0] * g64[..., 2]).float()
    cvals = torch.tensor([20.0, -20.0, 9.5, -9.5, 0.0, -0.0, 15.0, -12.0], device=dev)
    csel = flat_i % 8 == 4
    c_new[csel] = cvals[(flat_i[csel] // 8) % 8]
    dhd = torch.randn(M, H, device=dev, generator=g)
    dhp = torch.randn(M, H, device=dev, generator=g)
    dcp = torch.randn(M, H, device=dev, generator=g)
    r = torch.arange(M, device=dev)
    if layout == "tree":
        s, SD = 1, 4 * H
        Bn, PS = (M + rpb - 1) // rpb, 2 * rpb + 3
        c_col, dh_col, dc_col, cp_col, cp_ld, dhd_ld = 3 * H, 2 * H, 3 * H, 3 * H, SD, H
    else:
        assert rpb == 1
        s, SD, Bn, PS = 0, 2 * H, M, 1
        c_col, dh_col, dc_col, cp_col, cp_ld, dhd_ld = H, H, 0, H, 2 * H, 2 * H
    bi, sl = r // rpb, s + 2 * s * (r % rpb)
    pb, prow = PS * SD, 2 * s * SD
    Hid, dHid = _nan(Bn, PS, SD), _nan(Bn, PS, SD)
    dcbuf = dHid if layout == "tree" else _nan(Bn, PS, SD)             # flat: the dc buffer is its own [B][2H] block, dc_prev written in place
    Hid[bi, sl, c_col:c_col + H] = c_new
    if "dh_pos" not in nulls:
        dHid[bi, sl, dh_col:dh_col + H] = dhp
    if "dc_pos" not in nulls:
        dcbuf[bi, sl, dc_col:dc_col + H] = dcp
    merged = _nan(M, cp_ld)
    merged[:, cp_col:cp_col + H] = cp
    above = _nan(M, dhd_ld)
    above[:, :H] = dhd
    dgates = _nan(M, 4 * H)
    if layout == "tree":
        dmerged = _nan(M, SD)
        dcp_ptr, dcp_stride = dmerged.data_ptr() + 4 * cp_col, SD
    else:
        dmerged = dcbuf
        dcp_ptr, dcp_stride = dcbuf.data_ptr(), 2 * H
    a = rt.LstmBwdArgs()
    a.gates = gates.data_ptr()
    a.c_prev, a.c_prev_stride = merged.data_ptr() + 4 * cp_col, cp_ld
    a.c_new, a.pb, a.prow = Hid.data_ptr() + 4 * (s * SD + c_col), pb, prow
    a.dh_dense, a.dh_stride = (None if "dh_dense" in nulls else above.data_ptr()), dhd_ld
    a.dh_pos = None if "dh_pos" in nulls else dHid.data_ptr() + 4 * (s * SD + dh_col)
    a.dc_pos = None if "dc_pos" in nulls else dcbuf.data_ptr() + 4 * (s * SD + dc_col)
    a.dgates, a.dc_prev, a.dcp_stride = dgates.data_ptr(), dcp_ptr, dcp_stride
    a.M, a.H, a.rpb = M, H, rpb
    rt.check(lib.gcpx_lstm_bwd(C.byref(a), _st()), "lstm_bwd")
    torch.cuda.synchronize()
    # reference
    zero = torch.zeros(M, H, device=dev, dtype=torch.float64)
    dh_a = zero if "dh_dense" in nulls else dhd.double()
    dh_p = zero if "dh_pos" in nulls else dhp.double()
    dc_p = zero if "dc_pos" in nulls else dcp.double()
    ga = gates.double().requires_grad_(True)
    cp64 = cp.double().requires_grad_(True)
    c_lin = ga[..., 1] * cp64 + ga[..., 0] * ga[..., 2]
    c = c_lin + (c_new.double() - c_lin).detach()                     # the stored c, with the cell's dependence on its inputs
    h = ga[..., 3] * torch.tanh(c)
    gga, gcp = torch.autograd.grad((h * (dh_a + dh_p)).sum() + (c * dc_p).sum(), (ga, cp64))
    with torch.no_grad():
        si, sf, tg, so = g64[..., 0], g64[..., 1], g64[..., 2], g64[..., 3]
        act_d = torch.stack([si * (1 - si), sf * (1 - sf), 1 - tg * tg, so * (1 - so)], 1)           # [M][4][H]
        want = gga.permute(0, 2, 1) * act_d
        t = torch.tanh(c_new.double())
        A_dh = dh_a.abs() + dh_p.abs()
        A_dc = dc_p.abs() + A_dh * so * (1 + t * t)
        ab = torch.stack([A_dc * tg.abs() * si * (1 - si), A_dc * cp.double().abs() * sf * (1 - sf), A_dc * si * (1 + tg * tg),
                          A_dh * t.abs() * so * (1 - so)], 1)
        ab_cp = A_dc * sf
    tiny = 2.0 ** -125
    w1 = _within(dgates.view(M, 4, H), want, 18 * EPS * ab + tiny, "dgates (i | f | g | o)")
    if layout == "tree":
        got_cp = dmerged[:, cp_col:cp_col + H]
        mask = torch.zeros_like(dmerged, dtype=torch.bool)
        mask[:, cp_col:cp_col + H] = True
    else:
        got_cp = dcbuf[:, 0, :H]
        mask = torch.zeros_like(dcbuf, dtype=torch.bool)
        mask[:, 0, :H] = True
    w2 = _within(got_cp, gcp, 18 * EPS * ab_cp + tiny, "dc_prev")
    _untouched(dmerged[~mask], "gaps of the dc_prev buffer")
    # the planted saturated elements: exactly-0 derivative factors give exactly 0
    dg4 = dgates.view(M, 4, H)
    assert bool((dg4[:, 0][(pat == 0) | (pat == 1)] == 0).all()) and bool((dg4[:, 2][(pat == 3) | (pat == 4)] == 0).all())
    assert bool((dg4[:, 1][(pat == 2) | (pat == 5)] == 0).all()) and bool((dg4[:, 3][(pat == 2) | (pat == 4)] == 0).all())
    print(f"lstm_bwd M={M} H={H} rpb={rpb} {layout} nulls={nulls} scale={scale}: worst err / tol {max(w1, w2):.3f}")


# ------------------------------------------------------------------------------------------------------------------------------
# j. tree and sequence bookkeeping
# ------------------------------------------------------------------------------------------------------------------------------
# (n, width, sources: (ld, off_left, off_right, off_ctx0, off_ctxg, dst_col)), row width of the destination
_ACCUM = [
    (1, 32, [(2 * 32, 0, 32, -1, -1, 0)], 32),                                                   # backward_plan.py:117 (length head)
    (1, 32, [(4 * 32 + 8, 0, 32, 64, 96, 0)], 40),                                               # n = 1: slot 0 is left parent and e_0
    (2, 100, [(4 * 100 + 4, 0, 100, 200, 300, 4), (2 * 100, 0, 100, -1, -1, 4)], 112),            # two sources into the same columns
    (16, 128, [(2 * 128, 0, 128, -1, -1, j * 128) for j in range(4)], 4 * 128 + 16),              # backward_plan.py:300: disjoint columns
    (16, 32, [(4 * 32 + 8, 0, 32, 72, 104, 0), (64, 0, 32, -1, -1, 0), (64, 32, 0, -1, -1, 0), (96, 0, 32, -1, -1, 0), (64, 0, 32, -1, -1, 0),
              (64, -1, -1, 0, 32, 0)], 32),                                                      # backward_plan.py:366-372, nsrc 6
    (64, 128, [(4 * 128, 0, 128, 256, 384, 0), (128, 0, 0, -1, -1, 0), (128, -1, 0, -1, -1, 0)], 128),   # :275 (sum tree: both offsets 0)
    (64, 100, [(200, 100, 0, -1, -1, 0)], 100),
]


@pytest.mark.parametrize("n,width,srcs,roww", _ACCUM)
def test_tree_accum_vs_float64(env, n, width, srcs, roww):
    """gcpx_tree_accum as backward_ops.py:417-424 fills it, against float64 autograd of the forward it inverts: parents P[b][0..n] (row
    dst + b dst_sb + k slot_stride, columns dst_col .. + width), the level's input row (b, k) of source s = [P[k] | P[k + 1] | P[0] |
    P[n]] at off_left / off_right / off_ctx0 / off_ctxg of its ld-wide dense row (-1: absent), loss = sum over sources of src x input;
    expected dst_after = dst_before + dP.  n = 1 (slot 0 is the left child's parent and e_0, slot 1 the right one's and e_g), 2, 16, 64;
    1 to 6 sources; sources sharing a dst_col and sources on disjoint columns of a wider row; width 100 (the masked second 64-lane
    workgroup); ld wider than the used columns (the unused ones NaN).  The slots between the level's parents, the slots behind them and
    the destination rows' other columns hold NaN and must keep it.
    Tolerance (n + nsrc + 1) eps x abs-terms: a source adds at most 2 + n terms in f32 before it is added to the slot, nsrc sources."""
    rt, pk, lib, dev = env
    B, step = 3, 2
    g = torch.Generator(device=dev).manual_seed(n * 1000 + width + len(srcs))
    PS = n * step + 2
    dst = _nan(B, PS, roww)
    covered = torch.zeros(roww, dtype=torch.bool, device=dev)
    for s in srcs:
        covered[s[5]:s[5] + width] = True
    before = torch.randn(B, n + 1, roww, device=dev, generator=g)
    par = torch.arange(n + 1, device=dev) * step
    dst[:, par] = torch.where(covered, before, torch.full_like(before, NAN))
    a = rt.TreeAccumArgs()
    bufs = []
    P = torch.zeros(B, n + 1, roww, device=dev, dtype=torch.float64, requires_grad=True)
    loss, loss_abs = 0.0, 0.0
    for i, (ld, ol, orr, c0, cg, dcol) in enumerate(srcs):
        t = _nan(B * n, ld)
        for off in (ol, orr, c0, cg):
            if off >= 0:
                t[:, off:off + width] = torch.randn(B * n, width, device=dev, generator=g)
        bufs.append(t)
        sa = a.src[i]
        sa.ptr, sa.ld, sa.off_left, sa.off_right, sa.off_ctx0, sa.off_ctxg, sa.dst_col = t.data_ptr(), ld, ol, orr, c0, cg, dcol
        t64 = t.double().view(B, n, ld)
        Pc = P[..., dcol:dcol + width]
        parts = ((ol, Pc[:, :n]), (orr, Pc[:, 1:]), (c0, Pc[:, :1].expand(B, n, width)), (cg, Pc[:, n:].expand(B, n, width)))
        for off, inp in parts:
            if off >= 0:
                loss = loss + (t64[..., off:off + width] * inp).sum()
                loss_abs = loss_abs + (t64[..., off:off + width].abs() * inp).sum()
    a.dst, a.dst_sb, a.slot_stride, a.nsrc, a.B, a.n, a.width = dst.data_ptr(), PS * roww, step * roww, len(srcs), B, n, width
    rt.check(lib.gcpx_tree_accum(C.byref(a), _st()), "tree_accum")
    torch.cuda.synchronize()
    (dP,) = torch.autograd.grad(loss, P, retain_graph=True)
    (dPa,) = torch.autograd.grad(loss_abs, P)
    got = dst[:, par]
    w = _within(got[..., covered], (before.double() + dP)[..., covered], (n + len(srcs) + 1) * EPS * (before.double().abs() + dPa)[..., covered],
                "parent slots")
    _untouched(got[..., ~covered], "other columns of the parent rows")
    other = torch.ones(PS, dtype=torch.bool, device=dev)
    other[par] = False
    _untouched(dst[:, other], "slots between and behind the level's parents")
    print(f"tree_accum n={n} width={width} nsrc={len(srcs)}: worst err / tol {w:.3f}")


@pytest.mark.parametrize("L,T,nz,pitch", [(5, 20, 32, 32), (5, 20, 200, 216), (7, 80, 32, 48), (7, 80, 200, 200)])
def test_timestep_scatter_vs_float64(env, L, T, nz, pitch):
    """gcpx_timestep_scatter as backward_plan.py:402 calls it (det = the position-layout gradient one slot in: batch stride PS x pitch,
    node stride pitch; pitch = nz as there, and wider with NaN between the rows) with node_t from gcpx_balanced_binding for end_ind =
    1, 2, T / 2, T - 1 in one batch: a short sequence maps many nodes to one timestep and most of its timesteps receive nothing — those are
    written as 0, not left NaN.  nz = 200 > 128 threads: the column loop.  Reference: float64 index_add_ over the nodes whose timestep
    lies in [0, T).  Tolerance: count eps x abs-terms, count = the nodes a timestep receives (a serial sum; one node is a copy)."""
    rt, pk, lib, dev = env
    B, N = 4, 2 ** L - 1
    g = torch.Generator(device=dev).manual_seed(L * T + nz)
    end = torch.tensor([1, 2, T // 2, T - 1], dtype=torch.long, device=dev)
    node_t, leave = torch.zeros(B, N, dtype=torch.int32, device=dev), torch.zeros(B, N, dtype=torch.int32, device=dev)
    f2n, et = torch.zeros(B, T, dtype=torch.int32, device=dev), torch.zeros(B * N, dtype=torch.int32, device=dev)
    sl, n2r = torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, N, dtype=torch.int32, device=dev)
    rt.check(lib.gcpx_balanced_binding(end.data_ptr(), B, L, T, node_t.data_ptr(), leave.data_ptr(), f2n.data_ptr(), et.data_ptr(),
                                       sl.data_ptr(), n2r.data_ptr(), _st()), "binding")
    PS = N + 2
    det = _nan(B, PS, pitch)
    vals = torch.randn(B, N, nz, device=dev, generator=g)
    det[:, 1:N + 1, :nz] = vals
    out = _nan(B, T, nz)
    rt.check(lib.gcpx_timestep_scatter(det.data_ptr() + 4 * pitch, PS * pitch, pitch, node_t.data_ptr(), out.data_ptr(), B, N, T, nz, _st()),
             "timestep_scatter")
    torch.cuda.synchronize()
    want = torch.zeros(B, T, nz, dtype=torch.float64, device=dev)
    wabs, cnt = torch.zeros_like(want), torch.zeros(B, T, dtype=torch.float64, device=dev)
    for b in range(B):
        ok = (node_t[b] >= 0) & (node_t[b] < T)
        ti = node_t[b][ok].long()
        want[b].index_add_(0, ti, vals[b][ok].double())
        wabs[b].index_add_(0, ti, vals[b][ok].double().abs())
        cnt[b].index_add_(0, ti, torch.ones(len(ti), dtype=torch.float64, device=dev))
    assert float(cnt[0].max()) >= 2 and bool((cnt[0] == 0).any()), "the short sequence must share timesteps and leave some empty"
    w = _within(out, want, cnt[..., None] * EPS * wabs, "d inference input per timestep")
    assert bool((out[cnt == 0] == 0).all())
    print(f"timestep_scatter L={L} T={T} nz={nz}: worst err / tol {w:.3f}; up to {int(cnt.max())} nodes per timestep")


@pytest.mark.parametrize("B,rpb,width,dst_sr,with_src2", [(3, 7, 32, 32, False), (3, 7, 32, 64, True), (4, 15, 100, 100, True),
                                                          (2, 11, 128, 128, False)])
def test_add_rows_vs_float64(env, B, rpb, width, dst_sr, with_src2):
    """gcpx_add_rows as backward_plan.py:156-161 / training_sequential.py:330 call it: dst rows (b, j) one slot into a [B][PS][width]
    position buffer (dst_sr = width as there, and 2 width with NaN rows between), dense sources, src2 NULL or given; B rpb width not a
    multiple of 256.  One source: dst + src is ONE correctly rounded f32 addition, so the result equals float32(float64(dst) +
    float64(src)) bit for bit (the float64 sum of two f32 is exact).  Two sources: (src1 + src2) rounds first: 2 eps of |dst| + |src1| +
    |src2|.  Rows the kernel does not address keep their NaN bits."""
    rt, pk, lib, dev = env
    g = torch.Generator(device=dev).manual_seed(B + rpb + width)
    step = dst_sr // width
    PS = rpb * step + 2
    dst = _nan(B, PS, width)
    rows = 1 + torch.arange(rpb, device=dev) * step
    before = torch.randn(B, rpb, width, device=dev, generator=g)
    dst[:, rows] = before
    s1 = torch.randn(B * rpb, width, device=dev, generator=g)
    s2 = torch.randn(B * rpb, width, device=dev, generator=g) if with_src2 else None
    want = dst.clone()
    rt.check(lib.gcpx_add_rows(dst.data_ptr() + 4 * width, PS * width, dst_sr, s1.data_ptr(), rt.ptr(s2), B, rpb, width, _st()), "add_rows")
    torch.cuda.synchronize()
    ref = before.double() + s1.double().view(B, rpb, width) + (s2.double().view(B, rpb, width) if with_src2 else 0.0)
    if not with_src2:
        want[:, rows] = ref.float()
        _same_bits(dst, want, "dst += src1")
    else:
        ab = before.double().abs() + s1.double().abs().view(B, rpb, width) + s2.double().abs().view(B, rpb, width)
        w = _within(dst[:, rows], ref, 2 * EPS * ab, "dst += src1 + src2")
        print(f"add_rows B={B} rpb={rpb} width={width} two sources: worst err / tol {w:.3f}")
        other = torch.ones(PS, dtype=torch.bool, device=dev)
        other[rows] = False
        _untouched(dst[:, other], "rows between / around the addressed ones")


# (name, mode, B, rpb, width, dst offset, dst_sb, dst_sr, src offset, src_sb, src_sr)
_ROWS = [
    ("forward_plan.py:418 one zero-state row broadcast to a slot of every batch element", 0, 5, 1, 100, 200, 9 * 100, 0, 0, 0, 0),
    ("forward_plan.py:359 left parents -> dense merged rows", 0, 3, 4, 64, 0, 4 * 64, 64, 0, 11 * 64, 2 * 64),
    ("forward_plan.py:359 right parents added", 1, 3, 4, 64, 0, 4 * 64, 64, 2 * 64, 11 * 64, 2 * 64),
    ("backward_ops.py:373 un-padding copy (B 1, width = dst pitch < src pitch)", 0, 1, 128, 5, 0, 0, 5, 0, 0, 16),
    ("training_sequential.py:308 per-step input gradient slices", 1, 3, 9, 32, 0, 10 * 32, 32, 0, 9 * 80, 80),
    ("training_sequential.py:228 one row per batch element", 1, 7, 1, 32, 0, 10 * 32, 0, 0, 64, 0),
    ("training_sequential.py:419 copy behind the first step", 0, 3, 9, 32, 32, 10 * 32, 32, 0, 9 * 48, 48),
    ("training_sequential.py:429 context gradient summed over the steps", 2, 3, 9, 32, 0, 10 * 32, 0, 40, 9 * 104, 104),
    ("training_sequential.py:430 dense goal gradient, 33 steps", 2, 5, 33, 100, 0, 100, 0, 0, 33 * 100, 100),
]


@pytest.mark.parametrize("name,mode,B,rpb,width,doff,dst_sb,dst_sr,soff,src_sb,src_sr", _ROWS, ids=[r[0].split(" ")[0] + f"-m{r[1]}-{i}"
                                                                                                   for i, r in enumerate(_ROWS)])
def test_rows_strided_vs_float64(env, name, mode, B, rpb, width, doff, dst_sb, dst_sr, soff, src_sb, src_sr):
    """gcpx_rows_strided with the strides of its call sites (named per case), the degenerate ones included: src_sb = src_sr = dst_sr = 0
    with rpb 1 (one source row broadcast into a row of every batch element), dst_sb = src_sb = 0 with B 1 (the un-padding copy: width =
    destination pitch < source pitch), mode 2's sum over j in order.  Against float64 index arithmetic on flat buffers whose unaddressed
    elements are NaN (sources: a stray read poisons; destinations: must keep the NaN bits).  Mode 0 is a copy and mode 1 ONE correctly
    rounded addition: both bit for bit (float32(float64(dst) + float64(src))); mode 2: rpb eps x abs-terms (rpb - 1 additions of the
    ordered sum, one into dst).  Totals (B rpb width, B width for mode 2) not a multiple of 256 in most cases."""
    rt, pk, lib, dev = env
    g = torch.Generator(device=dev).manual_seed(B * rpb + width + mode)
    b_, j_, c_ = torch.meshgrid(torch.arange(B, device=dev), torch.arange(rpb, device=dev), torch.arange(width, device=dev), indexing="ij")
    si = soff + b_ * src_sb + j_ * src_sr + c_
    di = doff + b_ * dst_sb + (0 if mode == 2 else j_ * dst_sr) + c_
    src = _nan(int(si.max()) + 9)
    vals = torch.randn(B, rpb, width, device=dev, generator=g)
    src[si.flatten()] = vals.flatten()
    vals = src[si]                                                    # (a broadcast source: every (b, j) sees the last value written)
    dst = _nan(int(di.max()) + 9)
    if mode != 0:
        dst[di.flatten()] = torch.randn(di.numel(), device=dev, generator=g)
    before = dst.clone()
    rt.check(lib.gcpx_rows_strided(dst.data_ptr() + 4 * doff, dst_sb, dst_sr, src.data_ptr() + 4 * soff, src_sb, src_sr, B, rpb, width, mode,
                                   _st()), "rows_strided")
    torch.cuda.synchronize()
    want = before.clone()
    if mode == 0:
        want[di.flatten()] = vals.flatten()
        _same_bits(dst, want, name)
    elif mode == 1:
        assert di.unique().numel() == di.numel()
        want[di.flatten()] = (before[di].double() + vals.double()).float().flatten()
        _same_bits(dst, want, name)
    else:
        d0 = di[:, 0]
        ref = before[d0].double() + vals.double().sum(1)
        ab = before[d0].double().abs() + vals.double().abs().sum(1)
        w = _within(dst[d0], ref, rpb * EPS * ab, name)
        mask = torch.ones_like(dst, dtype=torch.bool)
        mask[d0.flatten()] = False
        _untouched(dst[mask], "unaddressed destination elements")
        print(f"rows_strided mode 2 rpb={rpb}: worst err / tol {w:.3f}")


@pytest.mark.parametrize("n", [1000, 256 * 5 + 1])
def test_lrelu_bwd_bit_exact(env, n):
    """gcpx_lrelu_bwd (backward_ops.py:334, backward_stages.py:230): dx = dy x (a > 0 ? 1 : slope) is ONE correctly rounded f32 product, so
    it equals float32(float64(dy) x (a > 0 ? 1 : float64(float32(slope)))) bit for bit (the float64 product of two f32 is exact).  `a`
    holds +0.0 and -0.0 (both take the slope), positive and negative denormals (a positive denormal is > 0), negatives; n is not a multiple
    of 256."""
    rt, pk, lib, dev = env
    g = torch.Generator(device=dev).manual_seed(n)
    a_host = torch.randn(n, generator=torch.Generator().manual_seed(n))      # planted on the host: no device kernel between the values and the test
    a_host[0::10] = 0.0
    a_host[1::10] = -0.0
    a_host[2::10] = 1e-40
    a_host[3::10] = -1e-40
    a_host[4::10] = 2.0 ** -149
    assert bool((a_host[2::10] > 0).all()) and bool((a_host[3::10] < 0).all()) and float(a_host[4]) > 0.0
    a = a_host.to(dev)
    dy = torch.randn(n, device=dev, generator=g)
    slope = C.c_float(0.2)
    dx = _nan(n + 8)
    rt.check(lib.gcpx_lrelu_bwd(a.data_ptr(), dy.data_ptr(), dx.data_ptr(), n, slope, _st()), "lrelu_bwd")
    torch.cuda.synchronize()
    want = _nan(n + 8)
    mult = torch.where(a_host > 0, torch.tensor(1.0, dtype=torch.float64), torch.tensor(float(slope.value), dtype=torch.float64)).to(dev)
    want[:n] = (dy.double() * mult).float()
    _same_bits(dx, want, "lrelu_bwd")


@pytest.mark.parametrize("B,rpb,width,s", [(3, 4, 32, 2), (5, 1, 32, 4), (2, 16, 100, 1)])
def test_tanh_bwd_rows_vs_float64(env, B, rpb, width, s):
    """gcpx_tanh_bwd_rows as backward_plan.py:189 calls it: dy and y rows (b, j) of a tree level in the position layout (base one level
    offset s in, batch stride PS width, row stride 2 s width; every other element NaN), dx dense [B rpb][width]; y holds exactly +1 and
    -1 (dx exactly 0 there).  Tolerance 3 eps of |dy| (1 + y^2): y^2, the subtraction against its abs-terms 1 + y^2, the product."""
    rt, pk, lib, dev = env
    g = torch.Generator(device=dev).manual_seed(B * rpb + width)
    PS = 2 * s * rpb + s + 1
    slots = s + 2 * s * torch.arange(rpb, device=dev)
    Y, dY = _nan(B, PS, width), _nan(B, PS, width)
    y = torch.tanh(torch.randn(B, rpb, width, device=dev, generator=g) * 3)
    y[:, :, 0::7] = 1.0
    y[:, :, 3::7] = -1.0
    dy = torch.randn(B, rpb, width, device=dev, generator=g)
    Y[:, slots], dY[:, slots] = y, dy
    dx = _nan(B * rpb * width + 8)
    rt.check(lib.gcpx_tanh_bwd_rows(dY.data_ptr() + 4 * s * width, Y.data_ptr() + 4 * s * width, dx.data_ptr(), PS * width, 2 * s * width, B, rpb,
                                    width, _st()), "tanh_bwd_rows")
    torch.cuda.synchronize()
    _untouched(dx[B * rpb * width:], "past the dense output")
    y64, dy64 = y.double(), dy.double()
    got = dx[:B * rpb * width].view(B, rpb, width)
    w = _within(got, dy64 * (1 - y64 * y64), 3 * EPS * dy64.abs() * (1 + y64 * y64), "dx")
    assert bool((got[:, :, 0::7] == 0).all()) and bool((got[:, :, 3::7] == 0).all())
    print(f"tanh_bwd_rows B={B} rpb={rpb} width={width}: worst err / tol {w:.3f}")


@pytest.mark.parametrize("row_floats", [4, 32 * 32 * 112])
@pytest.mark.parametrize("pattern", ["ends_mapped", "all_mapped", "none_mapped"])
def test_zero_unmapped_rows_exact(env, row_floats, pattern):
    """gcpx_zero_unmapped_rows (forward_plan.py:244, sequential.py:489): rows with row2frame < 0 become exactly 0, mapped rows are not
    touched (they hold NaN before and after, bit for bit).  row_floats = 4 (one float4) and S S pitch of the 32 x 32 head (28672 float4 >
    64 x 256 threads: the grid-stride loop); first and last row mapped / every row / none."""
    rt, pk, lib, dev = env
    rows = 6
    r2f = {"ends_mapped": [3, -1, 0, -1, -1, 7], "all_mapped": [0, 1, 2, 3, 4, 5], "none_mapped": [-1] * 6}[pattern]
    r2f = torch.tensor(r2f, dtype=torch.int32, device=dev)
    buf = torch.randn(rows + 1, row_floats, device=dev)
    buf[:rows][r2f >= 0] = NAN
    buf[rows] = NAN                                                   # the row behind the last one
    want = buf.clone()
    want[:rows][r2f < 0] = 0.0
    rt.check(lib.gcpx_zero_unmapped_rows(buf.data_ptr(), row_floats, r2f.data_ptr(), rows, _st()), "zero_unmapped_rows")
    torch.cuda.synchronize()
    _same_bits(buf, want, "zero_unmapped_rows")


def test_index_offset_and_inverse_exact(env):
    """gcpx_index_offset (backward_stages.py:56: out[b][t] = idx[b][t] + b stride, B T not a multiple of 256) and gcpx_index_inverse
    (forward_plan.py:238, backward_stages.py:98) on node2row from gcpx_balanced_binding (negative entries for nodes that match no frame;
    every non-negative entry < n_inv = B T, as the planner produces them): inv[r] = the node that maps to row r, -1 for rows nobody
    maps to (padded frames), over a prefilled buffer.  Exact."""
    rt, pk, lib, dev = env
    L, T, B = 5, 20, 4
    N = 2 ** L - 1
    end = torch.tensor([1, 2, T // 2, T - 1], dtype=torch.long, device=dev)
    node_t, leave = torch.zeros(B, N, dtype=torch.int32, device=dev), torch.zeros(B, N, dtype=torch.int32, device=dev)
    f2n, et = torch.zeros(B, T, dtype=torch.int32, device=dev), torch.zeros(B * N, dtype=torch.int32, device=dev)
    sl, n2r = torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, N, dtype=torch.int32, device=dev)
    rt.check(lib.gcpx_balanced_binding(end.data_ptr(), B, L, T, node_t.data_ptr(), leave.data_ptr(), f2n.data_ptr(), et.data_ptr(),
                                       sl.data_ptr(), n2r.data_ptr(), _st()), "binding")
    out = torch.full((B * T + 4,), -77, dtype=torch.int32, device=dev)
    rt.check(lib.gcpx_index_offset(f2n.data_ptr(), out.data_ptr(), B, T, N, _st()), "index_offset")
    inv = torch.full((B * T + 4,), 12345, dtype=torch.int32, device=dev)
    rt.check(lib.gcpx_index_inverse(n2r.data_ptr(), B * N, inv.data_ptr(), B * T, _st()), "index_inverse")
    torch.cuda.synchronize()
    assert torch.equal(out[:B * T].view(B, T), f2n + torch.arange(B, device=dev, dtype=torch.int32)[:, None] * N)
    assert bool((out[B * T:] == -77).all())
    fwd = n2r.flatten().long()
    assert bool((fwd < 0).any()) and int(fwd.max()) < B * T
    want = torch.full((B * T,), -1, dtype=torch.int32, device=dev)
    valid = torch.nonzero(fwd >= 0)[:, 0]
    assert fwd[valid].unique().numel() == valid.numel()
    want[fwd[valid]] = valid.int()
    assert torch.equal(inv[:B * T], want) and bool((want == -1).any())
    assert bool((inv[B * T:] == 12345).all())


# ------------------------------------------------------------------------------------------------------------------------------
# k. encoder data gradient and first-layer patches
# ------------------------------------------------------------------------------------------------------------------------------
def _unfold_rows(x):
    """F.unfold(x, 4, padding=1, stride=2) of NCHW x as rows [F Ho Wo][tap][ci] (tap = ky 4 + kx)"""
    Fr, Ci = x.shape[:2]
    u = F.unfold(x, 4, padding=1, stride=2)                           # [F][ci 16 + tap][Ho Wo]
    return u.view(Fr, Ci, 16, -1).permute(0, 3, 2, 1)


@pytest.mark.parametrize("H,W,Cin,Fr", [(4, 4, 4, 1), (4, 4, 64, 5), (8, 8, 16, 5), (8, 8, 64, 1), (64, 64, 4, 5), (64, 64, 64, 1),
                                        (16, 8, 16, 5), (8, 16, 4, 1)])
def test_col2im4x4s2_vs_float64(env, H, W, Cin, Fr):
    """gcpx_col2im4x4s2 (backward_stages.py:319) against float64 autograd of F.unfold(x, 4, padding=1, stride=2) re-ordered to the
    kernel's columns k = (tap, ci): dx = the gradient of sum(unfold(x) x dcol) w.r.t. x, NHWC.  4 x 4: every pixel is a border pixel (one
    to four taps); H != W both ways.  At most 4 addends: 4 eps x abs-terms."""
    rt, pk, lib, dev = env
    g = torch.Generator(device=dev).manual_seed(H * W + Cin + Fr)
    Ho, Wo = H // 2, W // 2
    dcol = torch.randn(Fr * Ho * Wo, 16 * Cin, device=dev, generator=g)
    dx = _nan(Fr * H * W * Cin + 8)
    rt.check(lib.gcpx_col2im4x4s2(dcol.data_ptr(), dx.data_ptr(), Fr, H, W, Cin, _st()), "col2im4x4s2")
    torch.cuda.synchronize()
    _untouched(dx[Fr * H * W * Cin:], "past dx")
    x = torch.zeros(Fr, Cin, H, W, dtype=torch.float64, device=dev, requires_grad=True)
    u = _unfold_rows(x)
    d64 = dcol.double().view(Fr, Ho * Wo, 16, Cin)
    (gx,) = torch.autograd.grad((u * d64).sum(), x, retain_graph=True)
    (ga,) = torch.autograd.grad((u * d64.abs()).sum(), x)
    w = _within(dx[:Fr * H * W * Cin].view(Fr, H, W, Cin), gx.permute(0, 2, 3, 1), 4 * EPS * ga.permute(0, 2, 3, 1), "dx")
    print(f"col2im4x4s2 {H}x{W} Cin={Cin} F={Fr}: worst err / tol {w:.3f}")


@pytest.mark.parametrize("H,W", [(8, 8), (64, 64), (16, 8)])
def test_im2col_image_exact(env, H, W):
    """gcpx_im2col_image (backward_stages.py:345): col [F Ho Wo][48], k = (ci, ky, kx), equals F.unfold(x, 4, padding=1, stride=2) of the
    NCHW image exactly; the image has no zero, so the padding taps are the only (exact) zeros."""
    rt, pk, lib, dev = env
    Fr = 3
    g = torch.Generator(device=dev).manual_seed(H + W)
    x = torch.rand(Fr, 3, H, W, device=dev, generator=g) + 0.5
    n = Fr * (H // 2) * (W // 2) * 48
    col = _nan(n + 8)
    rt.check(lib.gcpx_im2col_image(x.data_ptr(), col.data_ptr(), Fr, H, W, _st()), "im2col_image")
    torch.cuda.synchronize()
    want = F.unfold(x, 4, padding=1, stride=2).permute(0, 2, 1).reshape(-1)
    assert torch.equal(col[:n], want)
    assert int((col[:n] == 0).sum()) == int((want == 0).sum()) > 0
    _untouched(col[n:], "past col")


# ------------------------------------------------------------------------------------------------------------------------------
# l. column sums and partial reductions
# ------------------------------------------------------------------------------------------------------------------------------
def _colsum_terms(R, N, nsplit):
    """additions on the longest path of gcpx_colsum (+ gcpx_reduce_partials): a thread sums ceil(rows of its chunk / rpi) values (the
    4-way unrolled tree is shallower than serial; + 2 for its shape), the rpi row classes are combined serially, then the 16-way strided
    reduction over the chunks; never more than R - 1 (adding an exact 0 does not round)"""
    c4 = (N + 3) // 4
    tl = 0
    while (1 << tl) < c4 and tl < 8:
        tl += 1
    rpi = 256 >> tl
    rows_per = -(-R // nsplit)
    depth = -(-rows_per // rpi) + 2 + rpi + (0 if nsplit == 1 else -(-nsplit // 16) + 16)
    return min(R, depth)


@pytest.mark.parametrize("N,layout", [(N, "dense") for N in (1, 3, 16, 100, 112, 512, 2048)] + [(N, "batched") for N in (3, 16, 100, 512)])
def test_colsum_vs_float64(env, N, layout):
    """gcpx_colsum (+ gcpx_reduce_partials over its partials) as backward_ops.py:208-224 issues them, against float64 column sums.
    N = 1, 3 (a partial float4, ldy 16), 100 (32 threads per row, 7 of them idle), 2048 (two column workgroups); R = 1, 5, 255, 1000, 4099
    (fewer rows than row classes; a remainder after the 4-way unrolled loop); nsplit = 1 (direct, accumulate 0 and 1, with and without
    dst2), 7, 64 (nsplit > R: the empty chunks write 0 partials, every partial finite); "batched": rows (b, j) of a tree level in the
    position layout (dy_rpb 8, dy_sb, ldy = two slots: the `out` bias of backward_plan.py:195), R not a multiple of dy_rpb included.
    Every column >= N of dy and every unaddressed row is NaN; dst's columns beyond N keep their NaN.
    Tolerance: (terms + 1) eps x abs-terms with terms = the additions on the kernel's longest path, from the launch geometry
    (_colsum_terms; <= R - 1), + 1 for the accumulation.  Chosen over the plain R eps: at R = 4099, N = 2048 the path is 4099 + 3 long
    either way, but at N = 16 it is 4099 / 64 + 66 — the plain bound would be 30x looser there."""
    rt, pk, lib, dev = env
    g = torch.Generator(device=dev).manual_seed(N)
    pitch = 16 if N < 16 else (N + 3) // 4 * 4 + 8
    worst = 0.0
    for R in (1, 5, 255, 1000, 4099):
        vals = torch.randn(R, N, device=dev, generator=g) + 0.25
        if layout == "dense":
            dy = _nan(R, pitch)
            dy[:, :N] = vals
            ptr, ldy, rpb, sb = dy.data_ptr(), pitch, 0, 0
        else:
            rpb = 8
            Bn, PS = (R + rpb - 1) // rpb, 2 * rpb + 2
            dy = _nan(Bn, PS, pitch)
            r = torch.arange(R, device=dev)
            dy[r // rpb, 1 + 2 * (r % rpb), :N] = vals
            ptr, ldy, sb = dy.data_ptr() + 4 * pitch, 2 * pitch, PS * pitch
        ref, ab = vals.double().sum(0), vals.double().abs().sum(0)
        for nsplit in (1, 7, 64):
            for acc in (0, 1):
                pre = torch.randn(2, N, device=dev, generator=g)
                dst = _nan(2, N + 8)
                if acc:
                    dst[:, :N] = pre
                use2 = bool(acc) or nsplit > 1
                if nsplit == 1:
                    rt.check(lib.gcpx_colsum(ptr, ldy, R, N, rpb, sb, 1, None, dst[0].data_ptr(), dst[1].data_ptr() if use2 else None, acc,
                                             _st()), "colsum")
                else:
                    part = _nan(nsplit, N)
                    rt.check(lib.gcpx_colsum(ptr, ldy, R, N, rpb, sb, nsplit, part.data_ptr(), None, None, 0, _st()), "colsum")
                    rt.check(lib.gcpx_reduce_partials(part.data_ptr(), nsplit, N, N, dst[0].data_ptr(), acc, _st()), "reduce_partials")
                    rt.check(lib.gcpx_reduce_partials(part.data_ptr(), nsplit, N, N, dst[1].data_ptr(), acc, _st()), "reduce_partials")
                    torch.cuda.synchronize()
                    assert bool(torch.isfinite(part).all()), "every partial is written"
                    if nsplit > R:
                        assert bool((part[R:] == 0).all()), "empty chunks write 0"
                torch.cuda.synchronize()
                k = _colsum_terms(R, N, nsplit) + 1
                base = pre.double() if acc else torch.zeros(2, N, dtype=torch.float64, device=dev)
                for d in range(2 if use2 else 1):
                    worst = max(worst, _within(dst[d, :N], base[d] + ref, _gamma(k) * (base[d].abs() + ab),
                                               f"colsum R={R} nsplit={nsplit} acc={acc} dst{d}"))
                _untouched(dst[:, N:], "columns beyond N")
                if not use2:
                    _untouched(dst[1], "dst2 not given")
    print(f"colsum N={N} {layout}: worst err / tol {worst:.3f}")


def _wreduce_case(pk, case, dev):
    """(N, K, map_mode, Cin, ntap, Cout, n_map or None, ldw, k_off, dst shape, scatter(S [N][K] float64 -> (index tuple, values)))"""
    if case == "linear":
        N, K, ldw, k_off = 7, 9, 20, 3
        return N, K, 0, 0, 0, 0, None, ldw, k_off, (N, ldw), lambda S: ((slice(None), slice(k_off, k_off + K)), S)
    if case == "conv":
        Cout, Cin, ntap = 6, 5, 9                                     # Cin != ntap: an exchanged (tap, ci) lands elsewhere
        return Cout, ntap * Cin, 1, Cin, ntap, 0, None, 0, 0, (Cout, Cin, ntap), lambda S: ((slice(None),), S.view(Cout, ntap, Cin).permute(0, 2, 1))
    if case in ("conv_nmap", "bias_nmap"):
        perm = torch.tensor(pk.dlm_channel_perm(10), dtype=torch.int32, device=dev)      # 112 kernel slots -> 100 channels, -1 = empty slot
        Cin, ntap = (4, 9) if case == "conv_nmap" else (1, 1)
        sl = torch.nonzero(perm >= 0)[:, 0]
        ch = perm[sl].long()
        return (len(perm), ntap * Cin, 1, Cin, ntap, 0, perm, 0, 0, (104, Cin, ntap),
                lambda S: ((ch,), S.view(len(perm), ntap, Cin).permute(0, 2, 1)[sl]))
    if case == "bias":
        N = 37
        return N, 1, 1, 1, 1, 0, None, 0, 0, (N, 1, 1), lambda S: ((slice(None),), S.view(N, 1, 1))
    Cout, Cin, ntap = 3, 5, 16                                        # convt: n = (tap, co), k = ci -> w[ci][co][tap]
    return ntap * Cout, Cin, 2, Cin, ntap, Cout, None, 0, 0, (Cin, Cout, ntap), lambda S: ((slice(None),), S.view(ntap, Cout, Cin).permute(2, 1, 0))


@pytest.mark.parametrize("nsplit", [1, 15, 16, 17, 1024])
@pytest.mark.parametrize("case", ["linear", "conv", "conv_nmap", "bias_nmap", "bias", "convt"])
def test_wgrad_reduce_vs_float64(env, case, nsplit):
    """gcpx_wgrad_reduce (backward_ops.py:170, :201-206, :227): partial [nsplit][N][K] summed over the splits and scattered into the
    canonical parameter layout, against a float64 sum scattered by the documented maps written with torch indexing: LINEAR dst[n][k_off +
    k] with ldw > K (the other columns keep the NaN); CONV k = (tap, ci) -> w[n_map[n]][ci][tap] (Cin 5 != 9 taps) without a map, with
    the head's 112 slots -> 100 channels map (12 slots are -1: skipped; the rows of dst behind channel 99 keep the NaN) and the K = 1 bias
    forms; CONVT n = (tap, co), k = ci -> w[ci][co][tap].  N K = 63, 270, 37 (not multiples of 16: the masked last workgroup), 112, 240, 4032.
    accumulate 0 and 1.
    Tolerance (nsplit / 16 + 16) eps x abs-terms: each of the 16 thread groups adds nsplit / 16 values, 16 partial sums, the
    accumulation; never more than nsplit additions."""
    rt, pk, lib, dev = env
    N, K, mode, Cin, ntap, Cout, n_map, ldw, k_off, dshape, scatter = _wreduce_case(pk, case, dev)
    g = torch.Generator(device=dev).manual_seed(nsplit + N * K)
    part = torch.randn(nsplit, N, K, device=dev, generator=g)
    S, Sa = part.double().sum(0), part.double().abs().sum(0)
    idx, val = scatter(S)
    _, vab = scatter(Sa)
    worst = 0.0
    for acc in (0, 1):
        dst = _nan(*dshape)
        pre = torch.randn(*dshape, device=dev, generator=g)
        written = torch.zeros(dshape, dtype=torch.bool, device=dev)
        written[idx] = True
        if acc:
            dst[written] = pre[written]
        rt.check(lib.gcpx_wgrad_reduce(part.data_ptr(), nsplit, N, K, dst.data_ptr(), mode, Cin, ntap, Cout, rt.ptr(n_map), ldw, k_off, acc,
                                       _st()), "wgrad_reduce")
        torch.cuda.synchronize()
        want = torch.zeros(dshape, dtype=torch.float64, device=dev)
        wab = torch.zeros_like(want)
        want[idx], wab[idx] = val, vab
        if acc:
            want, wab = want + pre.double(), wab + pre.double().abs()
        k = min(nsplit, nsplit / 16 + 16)
        worst = max(worst, _within(dst[written], want[written], k * EPS * wab[written], f"{case} nsplit={nsplit} acc={acc}"))
        _untouched(dst[~written], "elements outside the map")
    print(f"wgrad_reduce {case} nsplit={nsplit}: worst err / tol {worst:.3f}")


@pytest.mark.parametrize("n", [1, 16, 17, 1000])
@pytest.mark.parametrize("ln", [1, 16, 33])
def test_reduce_partials_vs_float64(env, n, ln):
    """gcpx_reduce_partials with stride > len and a pointer offset into the partial rows (backward_ops.py:357: the d beta half of the
    GroupNorm partials), accumulate 0 and 1; everything outside the addressed columns is NaN, dst behind len keeps its NaN.
    Tolerance (n / 16 + 16) eps x abs-terms, as gcpx_wgrad_reduce (the same reduction), never more than n additions."""
    rt, pk, lib, dev = env
    g = torch.Generator(device=dev).manual_seed(n * 100 + ln)
    stride, off = 2 * ln + 5, ln + 2
    part = _nan(n, stride)
    vals = torch.randn(n, ln, device=dev, generator=g) + 0.25
    part[:, off:off + ln] = vals
    worst = 0.0
    for acc in (0, 1):
        pre = torch.randn(ln, device=dev, generator=g)
        dst = _nan(ln + 8)
        if acc:
            dst[:ln] = pre
        rt.check(lib.gcpx_reduce_partials(part.data_ptr() + 4 * off, n, stride, ln, dst.data_ptr(), acc, _st()), "reduce_partials")
        torch.cuda.synchronize()
        base = pre.double() if acc else torch.zeros(ln, dtype=torch.float64, device=dev)
        k = min(n, n / 16 + 16)
        worst = max(worst, _within(dst[:ln], base + vals.double().sum(0), k * EPS * (base.abs() + vals.double().abs().sum(0)), f"acc={acc}"))
        _untouched(dst[ln:], "behind len")
    print(f"reduce_partials n={n} len={ln}: worst err / tol {worst:.3f}")
