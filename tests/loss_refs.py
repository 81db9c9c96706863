"""FLOAT64 references, rounding bounds and the shared input sets of the loss, KL and BatchNorm-statistics kernel tests
(tests/test_gpu_loss_kernels.py runs the kernels on them, tests/test_loss_refs_cpu.py pins everything here without a GPU).

The references are plain torch in float64 (F.cross_entropy, F.binary_cross_entropy_with_logits, explicit sums) of the formulas
include/gcpx.h states for gcpx_kl_gauss / gcpx_loss_combine / gcpx_bn_finalize and oracle.gcp_model_oracle.losses computes; they are no
transcription of csrc/loss.hip.  Every reference returns its abs-terms beside the value: the same expression with every term replaced
by its absolute value.

The bounds are built from abs-terms and counted roundings, nothing measured.  eps = 2^-24 (f32 unit roundoff = half an ulp).  Form:
        eps x (k_elem x abs-terms of the elements + depth x sum |elements|) / divisor
  k_elem  the f32 roundings one element goes through as the kernel performs them (a fused multiply-add only removes one); expf, logf
          and log1pf are TAKEN as <= 2 ulp = 4 eps relative each (the device library documents 1 - 2 ulp);
  depth   the longest chain of additions a value passes through: the serial trips of one thread, log2 of the workgroup for the LDS
          tree, and the final combination (the division by the count).
The counts stand beside the code that uses them."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

EPS = 2.0 ** -24
U64 = 2.0 ** -53
NAN = float("nan")
SENT = 1.0e6            # finite sentinel in positions a kernel must not read: one read shows as an error of ~1e6, not as a NaN
TRANSC = 4.0            # roundings (in eps) taken for one expf / logf / log1pf: 2 ulp


def f32(x):
    """a Python float as the C ABI passes it (float arguments are rounded to f32 on the way in)"""
    return float(np.float32(x))


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _ceil_div(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------------------------------------
# 1. gcpx_kl_gauss
# ------------------------------------------------------------------------------------------------------------------------------
def _kl_elements(q, p, free_nats):
    """q, p [B][N][2 nz] = [mu | log_sigma] -> (clamped KL per dimension, abs-terms per dimension, unclamped KL), float64"""
    nz = q.shape[-1] // 2
    mq, lq, mp, lp = q[..., :nz].double(), q[..., nz:].double(), p[..., :nz].double(), p[..., nz:].double()
    ratio = (torch.exp(2 * lq) + (mq - mp) ** 2) / (2 * torch.exp(2 * lp))
    raw = lp - lq + ratio - 0.5
    mag = lp.abs() + lq.abs() + ratio + 0.5
    return torch.clamp(raw, min=free_nats), torch.clamp(mag, min=abs(free_nats)), raw


def kl_gauss(q, p, free_nats, node_weight=None):
    """per sequence, sum_n w[b, n] sum_d max(lp - lq + (e^{2 lq} + (mq - mp)^2) / (2 e^{2 lp}) - 1/2, free_nats)  (inference.py:38-43 with
    the node weights of sequential.py:543) -> (kl [B], abs-terms [B]); q, p [B][N][2 nz], node_weight [B][N] or None"""
    kl, mag, _ = _kl_elements(q, p, free_nats)
    w = torch.ones(q.shape[:2], dtype=torch.float64) if node_weight is None else node_weight.double()
    return (kl.sum(-1) * w).sum(1), (mag.sum(-1) * w.abs()).sum(1)


KL_K_ELEM = 2 * TRANSC + 5      # see kl_tol


def kl_depth(N, nz):
    """the additions a value of kl_sequence passes through: 3 over the four dimensions of a thread's float4, 1 product with the node
    weight, ceil(N nz / 4 / 1024) serial trips, 10 levels of the 1024-thread tree"""
    return 3 + 1 + _ceil_div(N * (nz // 4), 1024) + 10


def kl_tol(q, p, free_nats, node_weight=None):
    """Bound on |kl_out[b] - kl_gauss| of kl_sequence (csrc/loss.hip), [B].
    One element, abs-terms m = |lp| + |lq| + ratio + 1/2:
      ratio = (expf(2 lq) + diff^2) / (2 expf(2 lp)): the numerator's two non-negative terms carry 4 eps (expf) and 3 eps (the rounded
      difference squared), their sum one more: 5 eps; the denominator 4 eps (expf; the doubling is exact); the quotient 1:
      10 eps x ratio.  lp - lq, + ratio, - 1/2: one rounding each of a value no larger than m: 3 eps x m.
      Together <= 13 eps x m = (2 x 4 + 5) eps x m.  fmaxf is exact and 1-Lipschitz.
    depth: kl_depth."""
    kl, mag, _ = _kl_elements(q, p, free_nats)
    N, nz = q.shape[1], q.shape[2] // 2
    w = torch.ones(q.shape[:2], dtype=torch.float64) if node_weight is None else node_weight.double().abs()
    depth = kl_depth(N, nz)
    return EPS * (KL_K_ELEM * (mag.sum(-1) * w).sum(1) + depth * (kl.abs().sum(-1) * w).sum(1))


def _kl_rows(g, B, N, nz, same_seq=None):
    """[mu | log_sigma] rows of q and p, log-sigmas uniform over [-4, 2]; node (b, n) is, by (b + n) % 4: 0 q == p (KL exactly 0, or
    exactly the floor); 1 q near p (KL of a few hundredths); 2, 3 independent (KL from a tenth to 1e4).  Every node of sequence
    `same_seq` has q == p."""
    def draw():
        return torch.cat([torch.randn(B, N, nz, generator=g), torch.rand(B, N, nz, generator=g) * 6 - 4], 2)
    p, q = draw(), draw()
    q[..., nz - 1], p[..., nz - 1], q[..., 2 * nz - 1], p[..., 2 * nz - 2] = 0.0, 0.0, -4.0, 2.0     # the ends of the range
    near = p.clone()
    near[..., :nz] += 0.2 * torch.exp(p[..., nz:]) * torch.randn(B, N, nz, generator=g)
    near[..., nz:] += 0.05 * torch.randn(B, N, nz, generator=g)
    kind = (torch.arange(B)[:, None] + torch.arange(N)[None]) % 4
    q = torch.where((kind == 0)[..., None], p, torch.where((kind == 1)[..., None], near, q))
    if same_seq is not None and same_seq < B:
        q[same_seq] = p[same_seq]
    return q.contiguous(), p.contiguous()


# name -> layout (which sets the node weights), nz, N, B, free_nats.  Work items N nz / 4 of a 1024-thread workgroup: 248, 1024
# (exactly one trip), 960, 2112 (three trips), 19, 1040 and 1100 (two trips at nz = 32 and nz = 4), 2112 with five sequences, 4.
#   tree   forward_plan.py:523: rows inside [B][PS][2 nz] with PS = N + 2, base one slot in, node_stride 2 nz, no weights
#   seq    sequential.py:543:   [B][T - 1][2 nz] dense, node_weight = pad_mask + 1 with weight_bstride = T
#   wide   node_stride = 2 nz + 8 (gap COLUMNS), PS = N + 1, weights [B][N + 3] two floats in, values 0 / 0.5 / 1 / 2.5
KL_CASES = {
    "tree-nz32-N31-B5-fn0.1": ("tree", 32, 31, 5, 0.1),
    "tree-nz32-N128-B1-fn0": ("tree", 32, 128, 1, 0.0),
    "tree-nz256-N15-B5-fn1": ("tree", 256, 15, 5, 1.0),
    "wide-nz256-N33-B1-fn0.1": ("wide", 256, 33, 1, 0.1),
    "seq-nz4-N19-B5-fn0": ("seq", 4, 19, 5, 0.0),
    "seq-nz32-N130-B5-fn1": ("seq", 32, 130, 5, 1.0),
    "wide-nz4-N1100-B1-fn0.1": ("wide", 4, 1100, 1, 0.1),
    "tree-nz256-N33-B5-fn0": ("tree", 256, 33, 5, 0.0),
    "seq-nz4-N4-B1-fn1": ("seq", 4, 4, 1, 1.0),
}


@functools.lru_cache(maxsize=None)
def kl_case(name):
    """-> dict: q, p [B][N][2 nz] (the rows), w [B][N] or None, the buffers the kernel gets (q_buf, p_buf, w_buf: SENT in every gap) with
    their offsets (in floats) and strides, fn (free_nats as f32)"""
    layout, nz, N, B, fn = KL_CASES[name]
    g = _gen(1000 + sorted(KL_CASES).index(name))
    q, p = _kl_rows(g, B, N, nz, same_seq=1)
    c = dict(name=name, layout=layout, B=B, N=N, nz=nz, fn=f32(fn), q=q, p=p, w=None, w_buf=None, w_off=0, w_bs=0)
    if layout == "tree":
        PS = N + 2
        c.update(ns=2 * nz, bs=PS * 2 * nz, off=2 * nz)
        shape, rows = (B, PS, 2 * nz), slice(1, N + 1)
    elif layout == "seq":
        T = N + 1
        c.update(ns=2 * nz, bs=N * 2 * nz, off=0)
        shape, rows = (B, N, 2 * nz), slice(0, N)
        end = torch.randint(1, T, (B,), generator=g)
        end[0] = T - 1                                                  # one full sequence
        pad = (torch.arange(T)[None] <= end[:, None]).float()
        w_buf = pad.clone()
        w_buf[:, 0] = SENT                                              # frame 0 has no latent: its weight is never read
        c.update(w=pad[:, 1:].contiguous(), w_buf=w_buf, w_off=1, w_bs=T)
    else:
        PS, ns = N + 1, 2 * nz + 8
        c.update(ns=ns, bs=PS * ns, off=ns)
        shape, rows = (B, PS, ns), slice(1, N + 1)
        w = torch.tensor([0.0, 0.5, 1.0, 2.5])[torch.randint(0, 4, (B, N), generator=g)]
        w_buf = torch.full((B, N + 3), SENT)
        w_buf[:, 2:N + 2] = w
        c.update(w=w, w_buf=w_buf, w_off=2, w_bs=N + 3)
    for key, t in (("q_buf", q), ("p_buf", p)):
        buf = torch.full(shape, SENT)
        buf[:, rows, :2 * nz] = t
        c[key] = buf
    # the last float the kernel may touch lies inside the buffer
    assert c["off"] + (B - 1) * c["bs"] + (N - 1) * c["ns"] + 2 * nz <= c["q_buf"].numel()
    assert c["w_buf"] is None or c["w_off"] + (B - 1) * c["w_bs"] + N <= c["w_buf"].numel()
    return c


def kl_clamp_shares(c):
    """(share of the dimensions at or below the floor, share above it)"""
    _, _, raw = _kl_elements(c["q"], c["p"], c["fn"])
    low = float((raw <= c["fn"]).double().mean())
    return low, 1.0 - low


# ------------------------------------------------------------------------------------------------------------------------------
# 2. gcpx_loss_combine / gcpx_loss_pre + gcpx_loss_final
# ------------------------------------------------------------------------------------------------------------------------------
SLOTS = ("dense_img_rec", "kl", "len_pred", "existence_predictor", "state_regression", "total", "nll", "action_reconst", "cost_estimation")
WEIGHTS = ("w_rec", "w_kl", "w_len", "w_exist", "w_state", "w_action", "w_cost")
W_SLOT = dict(w_rec=0, w_kl=1, w_len=2, w_exist=3, w_state=4, w_action=7, w_cost=8)


def kl_weight(c):
    """the KL weight in force: *w_kl_dev when that pointer is set"""
    return c["w_kl_dev"] if c["w_kl_dev"] is not None else c["w_kl"]


def _loss_pieces(c):
    """Every term of gcpx_loss_args `c` (a dict of CPU tensors, None = NULL pointer) -> {slot: (value, abs-terms of the elements in eps
    units [k_elem x abs-terms, summed], sum |elements|, divisor, number of elements)}, float64"""
    B, T = c["B"], c["T"]
    pieces = {}
    # reconstruction: element nll x pad, one rounding
    e = c["nll_bt"].double() * c["pad_mask"].double()
    pieces[0] = (float(e.sum()) / B, 1 * float(e.abs().sum()), float(e.abs().sum()), B, B * T)
    if c["kl_b"] is not None:                                            # an element is a loaded value: no rounding
        e = c["kl_b"].double()
        pieces[1] = (float(e.sum()) / B, 0.0, float(e.abs().sum()), B, B)
    if c["len_logits"] is not None:
        lg, end = c["len_logits"].double(), c["end_ind"]
        val = F.cross_entropy(lg, end, reduction="sum")
        # one sequence: m = max (exact); s = sum_t expf(l_t - m), x_t = m - l_t >= 0: the rounded difference moves the argument by
        # eps x_t, expf adds 4 eps: term t carries (x_t + 4) eps relative, the sum over a lane's ceil(T / 64) serial trips and the 6
        # butterfly levels (ceil(T / 64) + 6) eps: s is within (sum_t p_t x_t + 4 + ceil(T / 64) + 6) eps relative, p = softmax, which
        # is that many eps ABSOLUTE on log s.  logf: 4 eps |log s|.  m + log s and - l[end]: one rounding each of at most
        # |m| + log s + |l_end|.  abs-terms of the element: |m| + log s + |l_end|.
        m = lg.max(1).values
        x = m[:, None] - lg
        logs = torch.logsumexp(-x, 1)
        px = (torch.softmax(-x, 1) * x).sum(1)
        l_end = lg[torch.arange(B), end]
        mag = m.abs() + logs + l_end.abs()
        rnd = px + TRANSC + _ceil_div(T, 64) + 6 + TRANSC * logs + 2 * mag
        elems = m + logs - l_end
        pieces[2] = (float(val) / B, float(rnd.sum()), float(elems.abs().sum()), B, B)
    if c["existence"] is not None:
        x, y = c["existence"].double(), c["leave"].double()
        val = F.binary_cross_entropy_with_logits(x, y, reduction="sum")
        # element max(x, 0) - x y + log1pf(expf(-|x|)), abs-terms m = max(x, 0) + |x| y + log1p(e), e = exp(-|x|) <= 1: expf 4 eps of e,
        # which log1p passes on as at most 4 eps e <= 5.8 eps log1p(e) (log1p(e) >= e ln 2 on [0, 1]); log1pf 4 eps log1p(e); x y is
        # exact (y is 0 or 1); the two additions one rounding each of at most m: <= (5.8 + 4 + 2) eps m <= 12 eps m
        mag = x.clamp_min(0) + x.abs() * y + torch.log1p(torch.exp(-x.abs()))
        n = x.numel()
        pieces[3] = (float(val) / n, 12 * float(mag.sum()), float(mag.sum()), n, n)
    if c["regressed_state"] is not None and c["state_target"] is not None:
        ml, sd = int(c["seq_len"].max()), c["state_dim"]
        mask = (c["state_mask"] if c["state_mask"] is not None else c["pad_mask"]).double().view(B, T)
        # element mask x (pred - target)^2: the difference 1 eps, the two products 1 each on a value that carries the difference twice:
        # 4 eps relative
        e = (c["regressed_state"].double()[:, :ml] - c["state_target"].double()[:, :ml]) ** 2 * mask[:, :ml, None]
        n = B * ml * sd
        pieces[4] = (float(e.sum()) / n, 4 * float(e.abs().sum()), float(e.abs().sum()), n, n)
    if c["action_pred"] is not None:
        tgt = c["action_seq"].double()[torch.arange(B), c["inv_t0"]]
        e = (c["action_pred"].double() - tgt) ** 2                      # difference 1 eps, squared: 3 eps relative
        n = e.numel()
        pieces[7] = (float(e.sum()) / n, 3 * float(e.sum()), float(e.sum()), n, n)
    if c["cost_pred"] is not None:
        e = (c["cost_pred"].double() - c["cost_target"].double()) ** 2
        pieces[8] = (float(e.sum()) / B, 3 * float(e.sum()), float(e.sum()), B, B)
    return pieces


def loss_terms(c):
    """The nine outputs of gcpx_loss_combine (include/gcpx.h:376-379, oracle.gcp_model_oracle.losses) for the gcpx_loss_args `c`
    (dict of CPU tensors; None = NULL) -> (out [9], abs-terms [9]) in float64:
      dense_img_rec = sum_bt pad_mask nll_bt / B;  kl = sum_b kl_b / B;  len_pred = cross entropy of len_logits against end_ind;
      existence_predictor = BCE with logits against leave;  state_regression = sum mask (pred - target)^2 / (B max(seq_len) state_dim),
      mask = state_mask when given, else pad_mask;  action_reconst, cost_estimation = mean squared errors;
      total = sum of w x term over the terms with w > 0 (the KL weight is *w_kl_dev when set), / total_div;  nll = dense_img_rec + kl.
    An absent optional term is 0 and out of the total."""
    pieces = _loss_pieces(c)
    out, mag = torch.zeros(9, dtype=torch.float64), torch.zeros(9, dtype=torch.float64)
    for s, (v, _, asum, div, _) in pieces.items():
        out[s], mag[s] = v, asum / div
    w = {k: c[k] for k in WEIGHTS}
    w["w_kl"] = kl_weight(c)
    for k in WEIGHTS:
        if w[k] > 0:
            out[5] += w[k] * out[W_SLOT[k]]
            mag[5] += w[k] * mag[W_SLOT[k]]
    out[5] /= c["total_div"]
    mag[5] /= c["total_div"]
    out[6], mag[6] = out[0] + out[1], mag[0] + mag[1]
    return out, mag


def loss_tol(c, threads):
    """Bound on |out[0..8] - loss_terms| for the launch whose five latent-side terms run in workgroups of `threads` threads (256:
    gcpx_loss_combine; 1024: gcpx_loss_pre).  The reconstruction and KL sums run in 256 threads in both forms.
    A term: eps (k_elem abs-terms + depth sum |elements|) / divisor, depth = the serial trips of a thread + log2(threads) + 1 (the
    division).  The length cross entropy gives one wavefront a sequence: its trips are ceil(B / (threads / 64)).
    total: every w x term one rounding, the (at most 7) additions one each, the division one: sum of w x bound + 9 eps sum w |term|,
    over total_div.  nll = rec + kl: the two bounds + one rounding."""
    pieces = _loss_pieces(c)
    out, mag = loss_terms(c)
    tol = torch.zeros(9, dtype=torch.float64)
    for s, (_, rnd, asum, div, n) in pieces.items():
        thr = 256 if s in (0, 1) else threads
        trips = _ceil_div(n, thr // 64 if s == 2 else thr)
        depth = trips + int(math.log2(thr)) + 1
        tol[s] = EPS * (rnd + depth * asum) / div
    w = {k: c[k] for k in WEIGHTS}
    w["w_kl"] = kl_weight(c)
    for k in WEIGHTS:
        if w[k] > 0:
            tol[5] += w[k] * tol[W_SLOT[k]]
    tol[5] = (tol[5] + 9 * EPS * float(mag[5]) * c["total_div"]) / c["total_div"]
    tol[6] = tol[0] + tol[1] + EPS * float(mag[6])
    return tol


# shapes: B, T, N, state_dim, n_actions, end_ind, inv_t0, state_mask given
#   T 5 / 64 / 65 / 130: part of a wavefront, exactly one trip of the lane loop, one trip and one lane, three trips
#   B 1 / 4 / 5 / 17: one wavefront's sequence, exactly the four wavefronts of gcpx_loss_combine, one trip more, and more than the
#     sixteen of gcpx_loss_pre
#   B N 7 and 252 (below 256), 527, 1275 (above 1024); B T 2210 and 325 (above 256)
#   max(seq_len): 1 < T with pad_mask as the state weights, = T with a state_mask, 41 < T with a state_mask, = T with pad_mask, 13 < T
_SHAPES = {
    "T5-B1": (1, 5, 7, 1, 1, [0], [0], False),
    "T64-B4": (4, 64, 63, 2, 2, [0, 63, 30, 63], [62, 0, 5, 62], True),
    "T65-B5": (5, 65, 255, 5, 7, [40, 3, 0, 17, 39], [63, 0, 1, 63, 30], True),
    "T130-B17": (17, 130, 31, 2, 7, [129, 0] + [7 * i % 130 for i in range(1, 16)], [128, 0] + [11 * i % 129 for i in range(1, 16)], False),
    "T20-B5": (5, 20, 31, 2, 2, [12, 2, 0, 7, 9], [18, 0, 3, 18, 9], True),
}
_VARIANTS = ([f"{w}={v}" for w in WEIGHTS for v in ("0", "-0.5")] + ["wkldev=0.25", "wkldev=0", "wkldev=-1"] +
             [f"null:{k}" for k in ("kl_b", "len_logits", "existence", "regressed_state", "state_target", "action_pred", "cost_pred")])
LOSS_CASES = [s for s in _SHAPES if s != "T20-B5"] + ["T20-B5"] + [f"T20-B5/{v}" for v in _VARIANTS]
KL_NZ = 4               # latent width of the KL rows a loss case hands gcpx_loss_pre


@functools.lru_cache(maxsize=None)
def loss_case(name):
    """-> the gcpx_loss_args of a case as a dict of CPU tensors (None = NULL pointer) and numbers, plus q / p [B][N][2 KL_NZ] rows for
    the KL workgroups of gcpx_loss_pre (tree layout, free_nats 0.1).  The variants of T20-B5 change one thing each."""
    shape, _, variant = name.partition("/")
    B, T, N, sd, na, ends, t0s, smask = _SHAPES[shape]
    g = _gen(2000 + sorted(_SHAPES).index(shape))
    end = torch.tensor(ends, dtype=torch.int64)
    assert end.shape == (B,) and 0 <= int(end.min()) and int(end.max()) <= T - 1
    t0 = torch.tensor(t0s, dtype=torch.int64)
    assert t0.shape == (B,) and 0 <= int(t0.min()) and int(t0.max()) <= T - 2
    full = (torch.arange(T)[None] <= end[:, None]).float()               # inputs.pad_mask
    pad = full.clone()
    if smask:
        pad[:, 0] = 0.0                                                  # sequential.py:63-66: the reconstruction weight has frame 0 zeroed
    ml = int(end.max()) + 1
    # reconstruction: rows of weight 0 hold values of 1e4 size (finite, so 0 x value is 0; they must not enter at any other weight)
    nll = torch.rand(B, T, generator=g) * 100
    nll = torch.where(pad == 0, 1e4 * (1 + torch.rand(B, T, generator=g)), nll)
    # length logits over +-50: without the max-subtraction expf overflows
    lg = (torch.randn(B, T, generator=g) * 20).clamp(-50, 50)
    if B > 1:
        lg[B - 1] = lg[B - 1].clamp(max=-30.0)                           # a sequence whose largest logit is far below 0
    lg[0, T // 2], lg[0, T - 1] = 50.0, -50.0
    # existence logits to +-30; leave all 0 for sequence 0, all 1 for sequence 1
    ex = (torch.randn(B, N, generator=g) * 10).clamp(-30, 30)
    ex[0, 0], ex[0, N - 1], ex[B - 1, 1] = 30.0, -30.0, -30.0
    leave = torch.randint(0, 2, (B, N), generator=g, dtype=torch.int32)
    leave[0] = 0
    if B > 1:
        leave[1] = 1
    reg, tgt = torch.randn(B, T, sd, generator=g), torch.randn(B, T, sd, generator=g)
    reg[:, ml:], tgt[:, ml:] = SENT, SENT                                # beyond max(seq_len): never read
    act = torch.randn(B, na, generator=g)
    acts = torch.full((B, T - 1, na), SENT)                              # only the step inv_t0[b] of a sequence is read
    acts[torch.arange(B), t0] = torch.randn(B, na, generator=g)
    q, p = _kl_rows(g, B, N, KL_NZ)
    c = dict(name=name, B=B, T=T, N=N, state_dim=sd, n_actions=na, nll_bt=nll, pad_mask=pad, kl_b=torch.rand(B, generator=g) * 50 + 1,
             len_logits=lg, end_ind=end, existence=ex, leave=leave, regressed_state=reg, state_target=tgt,
             seq_len=(end + 1).to(torch.int32), state_mask=full if smask else None, action_pred=act, action_seq=acts, inv_t0=t0,
             cost_pred=torch.randn(B, generator=g), cost_target=torch.randn(B, generator=g),
             w_rec=1.0, w_kl=0.5, w_len=1.0, w_exist=1.0, w_state=1.0, w_action=2.0, w_cost=1.0, w_kl_dev=None,
             total_div=float(T * 3 * 8 * 8),                             # T x input_nc x img_sz^2 (forward_plan.py:549) of 8 x 8 frames
             q=q, p=p, kl_fn=f32(0.1))
    if variant.startswith("null:"):
        assert variant[5:] in c
        c[variant[5:]] = None
    elif variant.startswith("wkldev="):
        c["w_kl_dev"] = float(variant[7:])
    elif variant:
        k, v = variant.split("=")
        assert k in WEIGHTS
        c[k] = float(v)
    return c


# ------------------------------------------------------------------------------------------------------------------------------
# 3. gcpx_bn_finalize
# ------------------------------------------------------------------------------------------------------------------------------
BN_CASES = [(1, 1, 1), (3, 48, 48), (2047, 16, 16), (2048, 16, 16), (2049, 112, 100), (130, 128, 8), (600, 64, 4)]
BN_EPS = f32(1e-5)
BN_GROUP = 4            # samples behind one entry of the partial table


@functools.lru_cache(maxsize=None)
def bn_case(n_partial, pitch, C):
    """The f32 partial table [n_partial][2][pitch] a producer leaves (sum and sum of squares of BN_GROUP samples per entry; entry
    (p, k C + c) belongs to channel c, k < pitch // C; columns from (pitch // C) C on are padding and hold SENT) with gamma, beta and
    running buffers.  Channel c, by c % 4: 0 |mean| = 1e3 std; 1 constant 3 (the variance is exactly 0: the clamp); 2 zeros; 3 mean and
    std of order one.  count = 1 for the one-entry table (the running variance then takes the biased form), else every sample."""
    g = _gen(3000 + n_partial + pitch + C)
    rep = pitch // C
    kind = torch.arange(C) % 4 if C > 1 else torch.tensor([3])
    mean = torch.where(kind == 0, torch.tensor(1e3), torch.where(kind == 3, torch.randn(C, generator=g), torch.tensor(0.0)))
    std = torch.where((kind == 0) | (kind == 3), torch.tensor(1.0), torch.tensor(0.0))
    x = mean + std * torch.randn(n_partial, rep, BN_GROUP, C, generator=g)
    x = torch.where(kind == 1, torch.tensor(3.0), x)
    if (n_partial, pitch, C) == (1, 1, 1):
        x = x[:, :, :1]                                                   # one sample: count = 1
    part = torch.full((n_partial, 2, pitch), SENT)
    part[:, 0, :rep * C] = x.sum(2).reshape(n_partial, rep * C)
    part[:, 1, :rep * C] = (x * x).sum(2).reshape(n_partial, rep * C)
    return dict(n_partial=n_partial, pitch=pitch, C=C, partial=part, count=float(n_partial * rep * x.shape[2]),
                gamma=torch.rand(C, generator=g) + 0.5, beta=torch.randn(C, generator=g),
                running_mean=torch.randn(C, generator=g), running_var=torch.rand(C, generator=g) + 0.5)


def _exact_column_sums(a):
    """a [n][C] of f32 values -> their exact column sums, rounded once to float64"""
    a = a.double().numpy()
    return torch.tensor([math.fsum(a[:, j]) for j in range(a.shape[1])], dtype=torch.float64)


def bn_finalize(partial, n_partial, pitch, C, count, gamma, beta, eps, momentum=0.0, running_mean=None, running_var=None):
    """float64 from the f32 partial table: s1, s2 = sums over rows p and replicas k of partial[p][0 | 1][k C + c] (exact), mean = s1 / count,
    var = max(s2 / count - mean^2, 0), scale = gamma / sqrt(var + eps), shift = beta - mean scale, rstd = 1 / sqrt(var + eps), the running
    values (1 - momentum) old + momentum new with the unbiased variance (the biased one when count <= 1).
    -> (values, bounds): dicts over scale, shift, mean, rstd (and running_mean, running_var when given).
    The kernel adds in float64 (unit roundoff u): ceil(n_partial rep / 256) serial trips and 8 tree levels, d additions: s1 and s2 are
    within d u of their abs-terms.  em = bound on the mean, ev = on the variance (its subtraction amplifies: (s2 / count + mean^2) u
    is far above var u where |mean| >> std); the clamp is 1-Lipschitz.  rv = relative bound on 1 / sqrt(var + eps) in float64 =
    ev / (2 (var + eps)) + 4 u.  Then the casts of the last block, one eps each:
      rstd_out = (float) rstd: 1 eps relative + rv              mean_out = (float) mean: 1 eps |mean| + em
      scale = gamma x (float) rstd: 2 eps relative + rv
      shift = beta - (float) mean x scale: the product carries the cast, scale's 2 eps + rv and its own rounding (4 eps + rv of
              |mean scale|, + em |scale|), the subtraction one rounding of at most |beta| + |mean scale|
      running = (1 - momentum) x old + momentum x (float) new: the f32 difference, the two products, the cast and the sum: at most
              3 roundings of |(1 - momentum) old| + |momentum new|, + momentum x (em | ev count / (count - 1))"""
    rep = pitch // C
    tab = partial.view(n_partial, 2, pitch)[:, :, :rep * C].reshape(n_partial, 2, rep, C)
    a, b = tab[:, 0].reshape(-1, C), tab[:, 1].reshape(-1, C)
    s1, s2 = _exact_column_sums(a), _exact_column_sums(b)
    a1, a2 = _exact_column_sums(a.abs()), _exact_column_sums(b.abs())
    d = _ceil_div(n_partial * rep, 256) + 8
    mean = s1 / count
    var_raw = s2 / count - mean ** 2
    var = var_raw.clamp_min(0)
    rstd = 1 / torch.sqrt(var + eps)
    g, bt = gamma.double(), beta.double()
    scale = g * rstd
    em = (d + 1) * U64 * a1 / count
    ev = (d + 1) * U64 * a2 / count + 2 * mean.abs() * em + 2 * U64 * (a2 / count + mean ** 2)
    rv = ev / (2 * (var + eps)) + 4 * U64
    ms = (mean * scale).abs()
    val = dict(scale=scale, shift=bt - mean * scale, mean=mean, rstd=rstd)
    tol = dict(scale=scale.abs() * (2 * EPS + rv), rstd=rstd * (EPS + rv), mean=EPS * mean.abs() + em,
               shift=EPS * (4 * ms + bt.abs() + ms) + ms * rv + em * scale.abs())
    if running_mean is not None:
        m = float(momentum)
        unb = count / (count - 1) if count > 1 else 1.0
        rm, rvar = running_mean.double(), running_var.double()
        val["running_mean"] = (1 - m) * rm + m * mean
        val["running_var"] = (1 - m) * rvar + m * var * unb
        tol["running_mean"] = 3 * EPS * (((1 - m) * rm).abs() + (m * mean).abs()) + m * em
        tol["running_var"] = 3 * EPS * (((1 - m) * rvar).abs() + m * var * unb) + m * ev * unb
    return val, tol
