"""FLOAT64 restatements, analytic gradients and rounding bounds of the attentive posterior's widened attention
(attentive_inference.py:80-84 with n_attention_heads, n_attention_layers > 1): masked single-query multi-head attention and the
row layer-norm without affine.  tests/test_gpu_attention_heads.py checks gcpx_attention_bwd_heads, gcpx_row_layernorm and
gcpx_row_layernorm_bwd against them; tests/test_attn_refs_cpu.py pins everything here, without a GPU, to float64 autograd of
oracle.adaptive_oracle.multihead_attention / attention and F.layer_norm.

The functions are plain torch in the dtype of their arguments, typed out from the formulas and calling neither the oracle nor
F.layer_norm / torch.softmax's autograd.

  mha(q, k, v, end, temp, heads, rpb)            q [M, dk], k [B, T, dk], v [B, T, nz], row r reads sequence r // rpb,
      dh = dk / heads, vh = nz / heads:          score[r, h, t] = q_h . k_h[t] / sqrt(dh) / temp, t <= end[b]; a = softmax_t;
                                                 out[r, h] = sum_t a[r, h, t] v_h[t]
  mha_grads(..., dout)                           dA = dO_h . V_h[t];  dS = a (dA - sum_t a dA);  dq_h = sum_t dS k_h[t] / (sqrt(dh) temp);
                                                 dK_h[b, t] = sum_j dS[(b, j), t] q_h[(b, j)] / (sqrt(dh) temp);
                                                 dV_h[b, t] = sum_j a[(b, j), t] dO_h[(b, j)];
                                                 dtemp_row[r] = - sum_h sum_t dS score / temp
  layernorm(x, add)                              s = x (+ add); y = (s - mean s) / sqrt(var s + 1e-5), biased variance; also rstd
  layernorm_bwd(dy, y, rstd)                     dx = rstd (dy - mean dy - y mean(dy y)): the gradient of x and of add alike

Bounds (derived, nothing measured).  u = 2^-24.  "abs-terms" of a quantity = the same expression with every term replaced by its
absolute value, in float64; a sum of n f32 terms is within n u abs-terms of the exact sum in any order, a chain of k roundings
within k u relative.

  attention backward, per head, as tests/test_gpu_backward_kernels.py derives it for one head, with the head's own widths: a score
  is a dh-term dot within dh u of its abs-terms sabs = |q_h| . |k_h| / sqrt(dh) / temp; a softmax weight moves with every score of
  its row, so the relative error of a and of everything that carries a is a multiple of (1 + max_t sabs); the dh-, vh-, T- and
  rpb-term sums of the backward add their counts.  With n = dh + vh + T + rpb + 8 and c = 1 + sabs inside the window:
      dS     n u a (|dA| + sum_t a |dA|) max_t c           (+ 2^-125 (|dA| + sum a |dA|): a weight below the f32 normal range is 0)
      dq     n u sum_t dS_abs |k_h| / (sqrt(dh) temp)
      dK     n u sum_j dS_abs |q_h| / (sqrt(dh) temp)
      dV     n u sum_j a c |dO_h|                          (+ 2^-125 sum_j |dO_h|)
      dtemp  (heads + n) u sum_h sum_t dS_abs sabs / temp  per row: the heads are one more sum

  layer-norm.  The sums of a row of W <= 1024 floats run as at most 4 float4 groups per lane (3 additions each), 6 shuffle steps
  and one division: a chain of at most ks = 20 roundings.  A = mean |s|, d = s - mean:
      s       es = u |s| with an addend, 0 without
      mean    em = ks u A + mean es
      d       ed = es + em + u |d|
      var     ev = mean(2 |d| ed) + (ks + 1) u var
      rstd    relative er = (ev + u (var + eps)) / (2 (var + eps)) + 2 u        (square root and division: one rounding each)
      y       rstd ed + |y| (er + u)
  A constant row has d = 0 exactly and var = 0: the bound is rstd em = 316 ks u |c|, what a mean that misses c by one rounding gives.
      dx      (ks + 4) u rstd (|dy| + mean |dy| + |y| mean |dy y|)
  The backward is checked on the y and rstd it is handed (f32 values), so their own forward error does not enter."""
import math

import torch

U = 2.0 ** -24
TINY = 2.0 ** -125
LN_EPS = 1e-5
KS = 20


def _split(x, heads):
    return x.reshape(*x.shape[:-1], heads, x.shape[-1] // heads)


def mha(q, k, v, end, temp, heads, rpb):
    """-> out [M, nz], a [M, heads, T], score [M, heads, T] (score is -inf outside the window)"""
    M, T = q.shape[0], k.shape[1]
    dh = q.shape[1] // heads
    qh = _split(q, heads)                                            # [M, h, dh]
    kh = _split(k, heads).repeat_interleave(rpb, 0)                  # [M, T, h, dh]
    vh = _split(v, heads).repeat_interleave(rpb, 0)                  # [M, T, h, vh]
    score = (qh[:, None] * kh).sum(-1).transpose(1, 2) / math.sqrt(dh) / temp            # [M, h, T]
    outside = torch.arange(T, device=q.device)[None, None, :] > end.repeat_interleave(rpb, 0)[:, None, None]
    score = score.masked_fill(outside, float("-inf"))
    ex = torch.exp(score - score.amax(-1, keepdim=True))
    a = ex / ex.sum(-1, keepdim=True)
    out = (a.transpose(1, 2)[..., None] * vh).sum(1).reshape(M, -1)
    return out, a, score


def mha_grads(q, k, v, end, temp, heads, rpb, dout):
    """analytic gradients of sum(out * dout): dict(a, dS [M, heads, T], dq [M, dk], dK [B, T, dk], dV [B, T, nz], dtemp_row [M])"""
    M, T, B = q.shape[0], k.shape[1], k.shape[0]
    dh = q.shape[1] // heads
    out, a, score = mha(q, k, v, end, temp, heads, rpb)
    qh, doh = _split(q, heads), _split(dout, heads)
    kh = _split(k, heads).repeat_interleave(rpb, 0)
    vh = _split(v, heads).repeat_interleave(rpb, 0)
    dA = (doh[:, None] * vh).sum(-1).transpose(1, 2)                 # [M, h, T]
    dS = a * (dA - (a * dA).sum(-1, keepdim=True))
    sc = 1.0 / (math.sqrt(dh) * temp)
    dq = (dS.transpose(1, 2)[..., None] * kh).sum(1).reshape(M, -1) * sc
    dK = (dS.transpose(1, 2)[..., None] * qh[:, None]).reshape(B, rpb, T, -1).sum(1) * sc
    dV = (a.transpose(1, 2)[..., None] * doh[:, None]).reshape(B, rpb, T, -1).sum(1)
    dtemp_row = -(dS * score.masked_fill(a == 0, 0.0)).sum((1, 2)) / temp
    return dict(out=out, a=a, dS=dS, dq=dq, dK=dK, dV=dV, dtemp_row=dtemp_row)


def mha_bounds(q, k, v, end, temp, heads, rpb, dout):
    """per-element bounds of an f32 evaluation of mha_grads (module docstring); float64 inputs"""
    assert q.dtype == torch.float64
    M, T, B = q.shape[0], k.shape[1], k.shape[0]
    dh, vw = q.shape[1] // heads, v.shape[2] // heads
    _, a, _ = mha(q, k, v, end, temp, heads, rpb)
    qh, doh = _split(q, heads).abs(), _split(dout, heads).abs()
    kh = _split(k, heads).abs().repeat_interleave(rpb, 0)
    vh = _split(v, heads).abs().repeat_interleave(rpb, 0)
    sc = 1.0 / (math.sqrt(dh) * abs(float(temp)))
    inside = a > 0
    sabs = ((qh[:, None] * kh).sum(-1).transpose(1, 2) * sc).masked_fill(~inside, 0.0)
    c = (1 + sabs) * inside
    n = dh + vw + T + rpb + 8
    dA = (doh[:, None] * vh).sum(-1).transpose(1, 2)
    spread = dA + (a * dA).sum(-1, keepdim=True)
    dS_abs = a * spread * c.amax(-1, keepdim=True)
    dq_abs = (dS_abs.transpose(1, 2)[..., None] * kh).sum(1).reshape(M, -1) * sc
    dK_abs = (dS_abs.transpose(1, 2)[..., None] * qh[:, None]).reshape(B, rpb, T, -1).sum(1) * sc
    dV_abs = ((a * c).transpose(1, 2)[..., None] * doh[:, None]).reshape(B, rpb, T, -1).sum(1)
    dO_sum = doh.reshape(B, rpb, 1, -1).sum(1).expand(B, T, -1)
    dt_abs = (dS_abs * sabs).sum((1, 2)) / abs(float(temp))
    return dict(dS=n * U * dS_abs + TINY * spread, dq=n * U * dq_abs + 1e-30, dK=n * U * dK_abs + 1e-30,
                dV=n * U * dV_abs + TINY * dO_sum + 1e-30, dtemp_row=(heads + n) * U * dt_abs + 1e-30)


def layernorm(x, add=None, eps=LN_EPS):
    """-> y, rstd [rows]"""
    s = x if add is None else x + add
    W = s.shape[1]
    d = s - s.sum(1, keepdim=True) / W
    rstd = 1.0 / torch.sqrt((d * d).sum(1, keepdim=True) / W + eps)
    return d * rstd, rstd[:, 0]


def layernorm_bwd(dy, y, rstd):
    W = dy.shape[1]
    m1, m2 = dy.sum(1, keepdim=True) / W, (dy * y).sum(1, keepdim=True) / W
    return rstd[:, None] * (dy - m1 - y * m2)


def layernorm_bound(x, add=None, eps=LN_EPS):
    assert x.dtype == torch.float64 and x.shape[1] <= 1024
    s = x if add is None else x + add
    mean = lambda t: t.mean(1, keepdim=True)
    es = U * s.abs() if add is not None else torch.zeros_like(s)
    em = KS * U * mean(s.abs()) + mean(es)
    d = s - mean(s)
    ed = es + em + U * d.abs()
    var = mean(d * d)
    ev = mean(2 * d.abs() * ed) + (KS + 1) * U * var
    er = (ev + U * (var + eps)) / (2 * (var + eps)) + 2 * U
    rstd = 1.0 / torch.sqrt(var + eps)
    return rstd * ed + (d * rstd).abs() * (er + U), (rstd * er)[:, 0]


def layernorm_bwd_bound(dy, y, rstd):
    assert dy.dtype == torch.float64
    mean = lambda t: t.mean(1, keepdim=True)
    return (KS + 4) * U * rstd[:, None] * (dy.abs() + mean(dy.abs()) + y.abs() * mean((dy * y).abs()))


# ---- the shared cases of the kernel test (the issue's list) ----
B_SEQ, DK, NZ = 3, 32, 128
T_CASES = (37, 300)                    # below and above one 256-thread trip over the frames
HEAD_CASES = (1, 2, 4, 8)              # 8: the minimal head widths 4 and 16
RPB_CASES = (1, 5)
TEMP = 0.6


def end_ind(T):
    """whole window, a one-frame window (dS and dq all zero), an interior cut"""
    return torch.tensor([T - 1, 0, 20])


def mha_case(T, rpb, seed=0):
    g = torch.Generator().manual_seed(1000 * T + 10 * rpb + seed)
    M = B_SEQ * rpb
    return dict(q=torch.randn(M, DK, generator=g), k=torch.randn(B_SEQ, T, DK, generator=g), v=torch.randn(B_SEQ, T, NZ, generator=g),
                dout=torch.randn(M, NZ, generator=g), end=end_ind(T), temp=TEMP, rpb=rpb)


def layernorm_case(W, with_add, seed=0):
    """7 rows (a last partial group of 4): spread and offset vary by row; row 3 is constant (var = 0)"""
    g = torch.Generator().manual_seed(77 * W + with_add + seed)
    R = 7
    x = torch.randn(R, W, generator=g) * (torch.rand(R, 1, generator=g) * 3 + 0.1) + torch.randn(R, 1, generator=g)
    add = torch.randn(R, W, generator=g) if with_add else None
    x[3] = 1.7
    if with_add:
        add[3] = -0.45
    return dict(x=x, add=add, dy=torch.randn(R, W, generator=g))
