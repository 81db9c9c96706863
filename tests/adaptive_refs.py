"""Plain FLOAT64 references of the adaptive-binding kernels (csrc/adaptive.hip), each written from the formula include/gcpx.h states —
no tiling, no split sums, no quadratic expansion.  tests/test_adaptive_refs_cpu.py pins them (to the goldens of the executed reference
and to oracle/adaptive_oracle.py); tests/test_gpu_adaptive_kernels.py compares the kernels with them.

Every reference returns its value AND its "abs-terms" as tests/test_gpu_glue_kernels.py defines them: the same expression with every
term replaced by its absolute value, in float64 — the scale a count of f32 roundings multiplies into a bound."""
import math

import numpy as np
import torch

from oracle import adaptive_oracle as A
from oracle import tree_index_oracle as TI

HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


# ------------------------------------------------------------------------------------------------------------------------------
# attention
# ------------------------------------------------------------------------------------------------------------------------------
def attention(q, k, v, start, end, temperature, rpb, heads):
    """Masked single-query multi-head attention.  q [M][dk], k [B][T][dk], v [B][T][nz] (any float dtype, taken to float64), start [B]
    or None (= 0), end [B] (frames t > end are outside, so an end beyond T - 1 is the whole tail), row r belongs to sequence r // rpb.
    Returns a dict of float64 arrays:
      out [M][nz], att [M][T] (mean over heads), a [M][heads][T] per-head weights,
      score [M][heads][T] (scaled, unmasked), score_abs (its abs-terms), inside [M][T] bool, out_abs [M][nz] = sum_t a |v|.
    A row whose window is empty is a softmax over nothing: NaN in a, att and out (what torch.softmax gives on a row of -inf)."""
    q, k = np.asarray(q, dtype=np.float64), np.asarray(k, dtype=np.float64)
    M, dk = q.shape
    B, T, _ = k.shape
    dh = dk // heads
    b_of = np.arange(M) // rpb
    s = np.zeros(B, dtype=np.int64) if start is None else np.asarray(start, dtype=np.int64)
    e = np.asarray(end, dtype=np.int64)
    t = np.arange(T)
    inside = (t[None] >= s[b_of][:, None]) & (t[None] <= e[b_of][:, None])
    inv = 1.0 / math.sqrt(dh) / float(temperature)
    qh = q.reshape(M, heads, dh)
    kh = k.reshape(B, T, heads, dh)[b_of]                                   # [M][T][h][dh]
    score = np.einsum("mhd,mthd->mht", qh, kh) * inv
    score_abs = np.einsum("mhd,mthd->mht", np.abs(qh), np.abs(kh)) * inv
    masked = np.where(inside[:, None, :], score, -np.inf)
    mx = masked.max(-1, keepdims=True)
    with np.errstate(invalid="ignore"):
        ex = np.where(inside[:, None, :], np.exp(masked - np.where(np.isinf(mx), 0.0, mx)), 0.0)
        a = ex / ex.sum(-1, keepdims=True)                                  # 0 / 0 = NaN on an empty window
    out = attention_values(a, v, inside, rpb, False)
    out_abs = attention_values(np.nan_to_num(a), v, inside, rpb, True)
    return dict(out=out, att=a.mean(1), a=a, score=score, score_abs=score_abs, inside=inside, out_abs=out_abs)


def attention_values(wgt, v, inside, rpb, absolute):
    """sum over the frames INSIDE the window of wgt[m][h][t] * v[b][t][h][:] (absolute: of |v|) -> [M][nz]; nothing outside the
    window is read.  wgt [M][heads][T]."""
    v = np.asarray(v, dtype=np.float64)
    M, heads, T = wgt.shape
    B, _, nz = v.shape
    vv = (np.abs(v) if absolute else v).reshape(B, T, heads, nz // heads)
    out = np.empty((M, nz))
    for m in range(M):
        sel = inside[m]
        out[m] = np.einsum("ht,thd->hd", wgt[m][:, sel], vv[m // rpb][sel]).reshape(nz)
        if not sel.any() and not absolute:
            out[m] = np.nan
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# squared distance
# ------------------------------------------------------------------------------------------------------------------------------
def sqdist(x, y):
    """out[b][n][t] = sum_k (x[b][n][k] - y[b][t][k])^2, the true value (never negative); abs-terms of the quadratic expansion the
    kernel evaluates: |x|^2 + |y|^2 + 2 sum_k |x_k| |y_k|.  x [B][N][K], y [B][T][K] -> (out, abs) float64 [B][N][T]."""
    x, y = torch.as_tensor(x).double(), torch.as_tensor(y).double()
    B, N, K = x.shape
    out = torch.empty(B, N, y.shape[1], dtype=torch.float64)
    for b in range(B):
        for n0 in range(0, N, 64):                                          # blocks of rows: the difference tensor stays small
            d = x[b, n0:n0 + 64, None, :] - y[b, None, :, :]
            out[b, n0:n0 + 64] = (d * d).sum(-1)
    xn, yn = (x * x).sum(-1), (y * y).sum(-1)
    ab = xn[:, :, None] + yn[:, None, :] + 2.0 * torch.bmm(x.abs(), y.abs().transpose(1, 2))
    return out, ab


# ------------------------------------------------------------------------------------------------------------------------------
# soft-DTW
# ------------------------------------------------------------------------------------------------------------------------------
def f32_cost(dsum, D, temp):
    """cost = (dsum / D) / temp as the model forms it: two correctly rounded f32 divisions.  The accumulators are float64 sums of
    THESE numbers (include/gcpx.h), so the float64 reference starts from them."""
    return (np.asarray(dsum, dtype=np.float32) / np.float32(D)) / np.float32(temp)


def _sweep(C, begin):
    """D[0][begin] = C[0][begin]; D[i][j] = C[i][j] + logaddexp(D[i-1][j], D[i-1][j-1]); row by row.  C [B][r][c] float64.
    Returns D and Dabs (the recurrence on |C| with max + log 2 in place of logaddexp: a bound on |D| along every path)."""
    B, r, c = C.shape
    D = np.full((B, r, c), -np.inf)
    Dabs = np.zeros((B, r, c))
    ar = np.arange(B)
    D[ar, 0, begin] = C[ar, 0, begin]
    Dabs[ar, 0, begin] = np.abs(C[ar, 0, begin])
    ninf, zero = np.full((B, 1), -np.inf), np.zeros((B, 1))
    for i in range(1, r):
        up, left = D[:, i - 1], np.concatenate([ninf, D[:, i - 1, :-1]], 1)
        lse = np.logaddexp(up, left)
        D[:, i] = np.where(np.isinf(lse), -np.inf, C[:, i] + lse)
        ua, la = Dabs[:, i - 1], np.concatenate([zero, Dabs[:, i - 1, :-1]], 1)
        Dabs[:, i] = np.where(np.isinf(lse), 0.0, np.abs(C[:, i]) + np.maximum(ua, la) + math.log(2.0))
    return D, Dabs


def soft_dtw(cost, end):
    """cost [B][r][c] (float32 or float64 numbers, used as float64), end [B] in [0, c-1].  Returns a dict:
      fwd, bwd [B][r][c]   the two accumulators in the orientation of `cost` (gcpx_soft_dtw's acc[:B] and acc[B:]), -inf where no
                           alignment reaches; fwd_abs, bwd_abs their path bounds;
      w_raw [B][r][c]      exp(fwd + bwd - C - z), z = fwd[r-1][end]: P(node i is aligned with frame j);
      w [B][r][c]          w_raw / max(sum over nodes, 1e-7);  colsum [B][c]."""
    C = -np.asarray(cost, dtype=np.float64)
    B, r, c = C.shape
    end = np.asarray(end, dtype=np.int64)
    fwd, fa = _sweep(C, np.zeros(B, dtype=np.int64))
    bwd, ba = _sweep(C[:, ::-1, ::-1], c - end - 1)
    bwd, ba = bwd[:, ::-1, ::-1], ba[:, ::-1, ::-1]
    z = fwd[np.arange(B), r - 1, end][:, None, None]
    with np.errstate(invalid="ignore"):
        e = fwd + bwd - C
    e = np.where(np.isinf(fwd) | np.isinf(bwd), -np.inf, e)
    w_raw = np.exp(e - z)
    colsum = w_raw.sum(1)
    w = w_raw / np.maximum(colsum, 1e-7)[:, None, :]
    return dict(fwd=fwd, bwd=bwd, fwd_abs=fa, bwd_abs=ba, w_raw=w_raw, w=w, colsum=colsum, z=z[:, 0, 0])


def soft_dtw_torch(C, end, normalised=True):
    """The same recurrence in float64 torch ops, differentiable: C [B][r][c] = MINUS the cost (a float64 tensor that may carry a
    gradient), end [B].  Returns w [B][r][c] float64: divided by max(sum over nodes, 1e-7), or (normalised=False) the raw
    probabilities.  Cells no alignment passes through are exact zeros and carry no derivative."""
    B, r, c = C.shape
    end = torch.as_tensor(end, dtype=torch.long)
    ninf = torch.full((B, 1), -np.inf, dtype=torch.float64)

    def sweep(Cm, begin):
        first = torch.full((B, c), -np.inf, dtype=torch.float64).scatter(1, begin[:, None], Cm[:, 0].gather(1, begin[:, None]))
        rows = [first]
        for i in range(1, r):
            up = rows[-1]
            left = torch.cat([ninf, up[:, :-1]], 1)
            m = torch.maximum(up, left)
            dead = torch.isinf(m)
            zero = torch.zeros_like(m)
            u0, l0, m0 = torch.where(dead, zero, up), torch.where(dead, zero, left), torch.where(dead, zero, m)
            lse = torch.log(torch.exp(u0 - m0) + torch.exp(l0 - m0)) + m0
            rows.append(torch.where(dead, m, Cm[:, i] + lse))
        return torch.stack(rows, 1)

    fwd = sweep(C, torch.zeros_like(end))
    bwd = sweep(C.flip(1, 2), c - end - 1).flip(1, 2)
    z = fwd[torch.arange(B), r - 1, end][:, None, None]
    reach = torch.isfinite(fwd) & torch.isfinite(bwd)
    zero = torch.zeros_like(C)
    e = torch.where(reach, fwd, zero) + torch.where(reach, bwd, zero) - C
    w_raw = torch.where(reach, torch.exp(torch.where(reach, e - z, zero)), zero)
    return w_raw / w_raw.sum(1, keepdim=True).clamp_min(1e-7) if normalised else w_raw


def _tangent_sweep(Dm, Cdot, begin):
    """Ddot[0][begin] = Cdot; Ddot[i][j] = Cdot[i][j] + s Ddot[i-1][j] + (1 - s) Ddot[i-1][j-1], s = the share of D[i-1][j] in
    logaddexp(D[i-1][j], D[i-1][j-1]); 0 on unreachable cells."""
    B, r, c = Dm.shape
    Td = np.zeros((B, r, c))
    ar = np.arange(B)
    Td[ar, 0, begin] = Cdot[ar, 0, begin]
    ninf, zero = np.full((B, 1), -np.inf), np.zeros((B, 1))
    for i in range(1, r):
        up, left = Dm[:, i - 1], np.concatenate([ninf, Dm[:, i - 1, :-1]], 1)
        tu, tl = Td[:, i - 1], np.concatenate([zero, Td[:, i - 1, :-1]], 1)
        with np.errstate(invalid="ignore", over="ignore"):
            s = np.where(np.isinf(up), 0.0, np.where(np.isinf(left), 1.0, 1.0 / (1.0 + np.exp(left - up))))
        Td[:, i] = np.where(np.isinf(Dm[:, i]), 0.0, Cdot[:, i] + s * tu + (1.0 - s) * tl)
    return Td


def soft_dtw_tangent(r, Cdot, end):
    """r = soft_dtw(cost, end); Cdot [B][r][c] = d C / d tau of the scores C = -cost.  Returns (w_raw, d w_raw / d tau)."""
    B, N, T = Cdot.shape
    end = np.asarray(end, dtype=np.int64)
    tf = _tangent_sweep(r["fwd"], Cdot, np.zeros(B, dtype=np.int64))
    tb = _tangent_sweep(r["bwd"][:, ::-1, ::-1], Cdot[:, ::-1, ::-1], T - end - 1)[:, ::-1, ::-1]
    zdot = tf[np.arange(B), N - 1, end][:, None, None]
    return r["w_raw"], r["w_raw"] * (tf + tb - Cdot - zdot)


def averaging_value(w, dsum, pad, log_sigma, D, coef):
    """coef * sum_{b,n,t} w * pad[b][t] * (0.5 dsum exp(-2 ls) + D (ls + 0.5 log 2 pi)), float64 torch"""
    gl = 0.5 * dsum * math.exp(-2.0 * log_sigma) + D * (log_sigma + HALF_LOG_2PI)
    return coef * (w * gl * pad[:, None, :]).sum()


def soft_dtw_dtemp(dsum, D, temp, end, pad, log_sigma, coef):
    """d / d temp of averaging_value(normalize(soft_dtw(cost)), ...) at cost = f32_cost(dsum, D, temp), by float64 autograd.
    The lattice scores are C(tau) = -cost * temp / tau at tau = temp: their VALUE is the f32 cost the kernel sweeps, their derivative
    d C / d tau = cost / temp.  Returns (gradient, abs1, abs2), the two abs-terms of the two ways the gradient is a sum:
      abs1 = sum over cells |d value / d C| * |d C / d tau|                       (a sum over the tangent's inputs)
      abs2 = |coef| sum_{b,t} pad * (sum_n |gl wdot| + (sum_n |gl| w) (sum_n |wdot|) / S) / S   (the combine kernel's own sums:
             w the raw probabilities, wdot = d w / d tau, S = sum_n w, gl the per-cell loss)."""
    cost = torch.from_numpy(f32_cost(dsum, D, temp)).double()
    t32 = float(np.float32(temp))
    dsum64, pad64 = torch.as_tensor(dsum).double(), torch.as_tensor(pad).double()
    C = (-cost).requires_grad_(True)
    val = averaging_value(soft_dtw_torch(C, end), dsum64, pad64, log_sigma, D, coef)
    (gC,) = torch.autograd.grad(val, C)
    Cdot = cost / t32
    grad, abs1 = float((gC * Cdot).sum()), float((gC.abs() * Cdot.abs()).sum())
    # the tangent of the raw probabilities for abs2: forward mode along the lattice in numpy (pinned against the autograd gradient
    # above by tests/test_adaptive_refs_cpu.py: sum of gl * d (w / S) must reproduce it)
    r = soft_dtw(cost.numpy(), end)
    w, wdot = (torch.from_numpy(x) for x in soft_dtw_tangent(r, Cdot.numpy(), end))
    gl = (0.5 * dsum64 * math.exp(-2.0 * log_sigma) + D * (log_sigma + HALF_LOG_2PI)).abs()
    S = w.sum(1)
    Ssafe = torch.where(S > 0, S, torch.ones_like(S))
    col = ((gl * wdot.abs()).sum(1) + (gl * w).sum(1) * wdot.abs().sum(1) / Ssafe) / Ssafe
    abs2 = abs(coef) * float((pad64 * torch.where(S > 0, col, torch.zeros_like(col))).sum())
    return grad, abs1, abs2


# ------------------------------------------------------------------------------------------------------------------------------
# bookkeeping on the matching distribution
# ------------------------------------------------------------------------------------------------------------------------------
def match_stats(w, end, L):
    """w [B][N = 2^L - 1][T] depth-first, end [B].  Returns a dict:
      frame2node [B][T] int32: depth-first position of the FIRST maximum over nodes taken in breadth-first order (an all-zero column
                               has its first maximum at breadth-first 0, the root);
      matched_idx [B][T] int32: the same for t <= end[b], -1 beyond;
      best_t [B][N] int32: first maximum over frames;
      entropy, entropy_abs [B][N]: -sum p log p with 0 log 0 = 0;  p_n, p_abs [B][N]: clamp(sum p, 0, 1) and sum |p|."""
    w = np.asarray(w, dtype=np.float64)
    B, N, T = w.shape
    perm = TI.bf2df_perm(L)
    f2n = perm[w[:, perm, :].argmax(1)].astype(np.int32)                     # np.argmax: first maximum
    midx = np.where(np.arange(T)[None] <= np.asarray(end)[:, None], f2n, -1).astype(np.int32)
    best_t = w.argmax(2).astype(np.int32)
    with np.errstate(divide="ignore", invalid="ignore"):
        plogp = np.where(w > 0, w * np.log(np.where(w > 0, w, 1.0)), 0.0)
    return dict(frame2node=f2n, matched_idx=midx, best_t=best_t, entropy=-plogp.sum(2), entropy_abs=np.abs(plogp).sum(2),
                p_n=np.clip(w.sum(2), 0.0, 1.0), p_abs=np.abs(w).sum(2))


def distance_prune(dist, thr, best_t=None):
    """dist [B][N-1], thr; node 0 is always kept, node p > 0 is kept unless sigmoid(dist[p-1]) > thr (float64 sigmoid).
    Returns leave [B][N], kept_idx [B][N] (kept positions in order, then -1), count [B], target [B][N-1] (best_t[p] == best_t[p-1])
    or None, all int32, and margin = min |sigmoid - thr| (the caller asserts the decision is not a rounding question)."""
    dist = np.asarray(dist, dtype=np.float64)
    B, N = dist.shape[0], dist.shape[1] + 1
    sig = 1.0 / (1.0 + np.exp(-dist))
    leave = np.concatenate([np.ones((B, 1), dtype=bool), ~(sig > thr)], 1)
    kept = np.full((B, N), -1, dtype=np.int32)
    for b in range(B):
        pos = np.nonzero(leave[b])[0]
        kept[b, :len(pos)] = pos
    target = None
    if best_t is not None:
        bt = np.asarray(best_t)
        target = (bt[:, 1:] == bt[:, :-1]).astype(np.int32)
    return dict(leave=leave.astype(np.int32), kept_idx=kept, count=leave.sum(1).astype(np.int32), target=target,
                margin=float(np.abs(sig - thr).min()) if sig.size else 1.0, sig=sig)


def averaging_nll(dsum, w, log_sigma, D):
    """nll_bt[b][t] = sum_n w * (0.5 dsum exp(-2 ls) + D (ls + 0.5 log 2 pi)); abs-terms: sum_n |w| (0.5 |dsum| exp(-2 ls) +
    D (|ls| + 0.5 log 2 pi)).  -> (value, abs) float64 [B][T]"""
    dsum, w = np.asarray(dsum, dtype=np.float64), np.asarray(w, dtype=np.float64)
    iv2 = math.exp(-2.0 * log_sigma)
    val = (w * (0.5 * dsum * iv2 + D * (log_sigma + HALF_LOG_2PI))).sum(1)
    ab = (np.abs(w) * (0.5 * np.abs(dsum) * iv2 + D * (abs(log_sigma) + HALF_LOG_2PI))).sum(1)
    return val, ab


def soft_average(w, x):
    """out[b][t][:] = sum_n w[b][n][t] x[b][n][:] -> (value, abs) float64 [B][T][D]"""
    w, x = np.asarray(w, dtype=np.float64), np.asarray(x, dtype=np.float64)
    return np.einsum("bnt,bnd->btd", w, x), np.einsum("bnt,bnd->btd", np.abs(w), np.abs(x))


# ------------------------------------------------------------------------------------------------------------------------------
# hard DTW
# ------------------------------------------------------------------------------------------------------------------------------
def dtw_align(cost, n_len=None, t_len=None):
    """oracle.adaptive_oracle.dtw_matches (pinned to the executed reference) on cost[b][:n_len[b]][:t_len[b]].  cost [B][N][T].
    Returns per sequence a dict: n, t, acc [n][t] float64, path (rows, cols) start -> end, inds [T] int32 (-1 beyond t), dist."""
    cost = np.asarray(cost)
    B, N, T = cost.shape
    res = []
    for b in range(B):
        n = N if n_len is None else int(n_len[b])
        t = T if t_len is None else int(t_len[b])
        d, acc, path, inds = A.dtw_matches(cost[b, :n, :t])
        full = np.full(T, -1, dtype=np.int32)
        full[:t] = inds
        res.append(dict(n=n, t=t, acc=acc, path=(np.asarray(path[0]), np.asarray(path[1])), inds=full, dist=float(d)))
    return res
