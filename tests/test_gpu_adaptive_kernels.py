"""-m gpu: the forward kernels of the adaptive path (csrc/adaptive.hip: attention, the squared-distance GEMM, the soft-DTW sweeps and
their temperature tangent, the matching bookkeeping, pruning, the averaging loss, the soft average, the hard DTW of the evaluation)
against the plain FLOAT64 references of tests/adaptive_refs.py (pinned on the CPU by tests/test_adaptive_refs_cpu.py), at the sizes
where their loops wrap: a second trip of every strided loop, every launch shape the host picks, lengths 1, tiles plus one.

Conventions (those of tests/test_gpu_glue_kernels.py):
  * the kernel is called through video_gcp_amd.runtime;
  * every float output starts as NaN, every integer output as a sentinel: what the kernel must write is checked finite and against the
    reference, what it must leave alone still holds the fill;  1e6 stands wherever a kernel must not read;
  * every tolerance is derived.  eps = 2^-24 (f32 unit roundoff), u = 2^-53 (f64), "abs-terms" = the expression with every term replaced
    by its absolute value, in float64: a sum of n f32 terms is within n eps x abs-terms of the exact sum.  An f32 MFMA is counted as one
    rounding per multiply-add (a fused or wider internal sum only lowers it).
    Device math functions: the ROCm install here carries no accuracy table for the HIP device library, so expf, logf and the float64
    exp are ASSUMED to be within 2 ulp (ulp = 2 eps, resp. 2 u).  softplus_neg (the kernel's own float64 log1p(exp(x))) is taken at the
    same 2 ulp.
    "worst" beside a bound = the largest error / bound measured on an MI355X over the cases of that test."""
import math

import numpy as np
import pytest
import torch

import adaptive_refs as R

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
U64 = 2.0 ** -53
ULP32, ULP64 = 2 * EPS, 2 * U64
MATH_ULPS = 2            # assumed accuracy of expf / logf / exp (see the module docstring)
TINY = 2.0 ** -126       # smallest normal f32: a result below it may be flushed to zero
NAN = float("nan")
SENT = 1.0e6
ISENT = -77
UNSUPPORTED = -2         # GCPX_ERR_UNSUPPORTED


@pytest.fixture(scope="module")
def env():
    from video_gcp_amd import runtime as rt
    lib = rt.load_library()
    assert torch.cuda.is_available()
    return rt, lib, torch.device("cuda")


def _st():
    return torch.cuda.current_stream().cuda_stream


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device="cuda")


def _isent(*shape):
    return torch.full(shape, ISENT, dtype=torch.int32, device="cuda")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _within(got, ref, tol, name):
    """|got - ref| <= tol element-wise; got must be finite (a NaN is an element the kernel did not write).  Returns worst err / tol."""
    got = torch.as_tensor(got).detach().double().cpu()
    ref = torch.as_tensor(np.asarray(ref) if not torch.is_tensor(ref) else ref).double().cpu()
    tol = torch.as_tensor(np.asarray(tol) if not torch.is_tensor(tol) else tol).double().cpu().expand_as(ref)
    assert got.shape == ref.shape, f"{name}: {tuple(got.shape)} against {tuple(ref.shape)}"
    assert bool(torch.isfinite(got).all()), f"{name}: {int((~torch.isfinite(got)).sum())} elements not written (or not finite)"
    err = (got - ref).abs()
    ratio = err / tol.clamp_min(1e-300)
    bad = err > tol
    if bool(bad.any()):
        i = int(torch.nonzero(bad.flatten())[0])
        raise AssertionError(f"{name}: {int(bad.sum())}/{bad.numel()} elements outside the bound; first at flat index {i}: got "
                             f"{float(got.flatten()[i])!r} want {float(ref.flatten()[i])!r} tol {float(tol.flatten()[i]):.3e}; "
                             f"worst err/tol {float(ratio.max()):.3g}")
    w = float(ratio.max()) if ratio.numel() else 0.0
    print(f"[ratio] {name}: worst err/tol {w:.3g}")
    return w


def _same(got, ref, name):
    got, ref = torch.as_tensor(got).cpu(), torch.as_tensor(np.asarray(ref) if not torch.is_tensor(ref) else ref).cpu()
    assert got.shape == ref.shape, f"{name}: {tuple(got.shape)} against {tuple(ref.shape)}"
    bad = ~(got == ref.to(got.dtype))
    if bool(bad.any()):
        i = int(torch.nonzero(bad.flatten())[0])
        raise AssertionError(f"{name}: {int(bad.sum())}/{bad.numel()} elements differ; first at flat index {i}: got "
                             f"{got.flatten()[i].item()} want {ref.flatten()[i].item()}")


def _untouched(t, name, fill=NAN):
    ok = torch.isnan(t) if isinstance(fill, float) and math.isnan(fill) else (t == fill)
    assert bool(ok.all()), f"{name}: {int((~ok).sum())} elements written that the kernel must leave alone"


# ------------------------------------------------------------------------------------------------------------------------------
# a. gcpx_attention
# ------------------------------------------------------------------------------------------------------------------------------
def _attention_bounds(r, v, rpb, heads, dh):
    """Bounds on att [M][T] and out [M][nz] from the reference's per-head quantities.
    score: dh fmas, sqrtf, two divisions and one product for the scale: (dh + 3) eps x score-abs-terms = ds.  The softmax is
    exp(s_t - max) / sum: an error of at most Delta = max ds in every score moves a weight by a factor e^(+-2 Delta); the subtraction
    s_t - max rounds once (eps |s_t - max|, in the numerator and, weighted by a, in the denominator); expf MATH_ULPS ulp in both; the
    sum of the n keys of the window n eps; the division eps:
        rel_t = 2 Delta + eps |s_t - max| + sum_u a_u eps |s_u - max| + (n + 1) eps + 2 MATH_ULPS ulp,   tol_a = a rel + TINY
    (TINY: an expf below the smallest normal may flush to zero; the sum is at least 1).
    att = sum_h a_h / heads: a division and an add per head: tol_att = sum_h (tol_a + 2 eps a) / heads + heads eps att.
    out = sum_t a_t v_t: the weight errors times |v|, plus an fma chain over the keys of one group and the fixed-order sum of the
    non-zero group sums, at most n + 1 roundings on any term: tol_out = sum_t tol_a |v_t| + (n + 1) eps x abs-terms."""
    inside = r["inside"][:, None, :]
    a = np.nan_to_num(r["a"])
    ds = np.where(inside, (dh + 3) * EPS * r["score_abs"], 0.0)
    delta = ds.max(-1, keepdims=True)
    sm = np.where(inside, r["score"], -np.inf)
    mx = sm.max(-1, keepdims=True)
    with np.errstate(invalid="ignore"):
        rt = EPS * np.where(inside, np.abs(sm - mx), 0.0)
    n = inside.sum(-1, keepdims=True)
    rel = 2 * delta + rt + (a * rt).sum(-1, keepdims=True) + (n + 1) * EPS + 2 * MATH_ULPS * ULP32
    tol_a = np.where(inside, a * rel + TINY, 0.0)
    tol_att = ((tol_a + 2 * EPS * a) / heads).sum(1) + heads * EPS * np.nan_to_num(r["att"])
    tol_out = R.attention_values(tol_a, v, r["inside"], rpb, True) + (n[:, 0] + 1) * EPS * r["out_abs"]
    return tol_att, tol_out


def _run_attention(env, q, k, v, start, end, temp, rpb, heads, with_att):
    rt, lib, dev = env
    M, dk = q.shape
    B, T, nz = v.shape
    out, att = _nan(M * nz + 5), (_nan(M * T + 5) if with_att else None)
    qd, kd, vd, ed = q.to(dev), k.to(dev), v.to(dev), torch.as_tensor(end, dtype=torch.int64).to(dev)
    sd = None if start is None else torch.as_tensor(start, dtype=torch.int64).to(dev)
    td = torch.tensor([temp], device=dev)
    rt.check(lib.gcpx_attention(qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), rt.ptr(sd), ed.data_ptr(), td.data_ptr(), out.data_ptr(),
                                rt.ptr(att), M, rpb, T, dk, nz, heads, _st()), "attention")
    torch.cuda.synchronize()
    _untouched(out[M * nz:], "out past M rows")
    if with_att:
        _untouched(att[M * T:], "att past M rows")
    return out[:M * nz].view(M, nz).cpu(), (att[:M * T].view(M, T).cpu() if with_att else None)


_ATT_CFG = [(4, 4, 1), (16, 64, 4), (32, 128, 1), (8, 1024, 1), (8, 2048, 2)]


@pytest.mark.parametrize("cfg", _ATT_CFG, ids=lambda c: "dk%d-nz%d-h%d" % c)
@pytest.mark.parametrize("T", [1, 37, 256, 257, 301])
def test_attention_matches_float64(env, T, cfg):
    """gcpx_attention against R.attention.  T = 257 and 301 take a second trip of the three `t += 256` loops, and with T % 4 != 0 put the
    partial sums at the rounded-up offset (T+3)&~3; (dk, nz, heads) give c4n = nz / heads / 4 = 1, 4, 32, 256, 256 (G = 256 ... 1 key
    groups) and head widths down to 4; rpb 1 and 5; start_ind NULL and given; att NULL and given; temperature 1 and 0.02 (expf underflows
    for most keys).  Four sequences: the full window, start == end (the weight is exactly 1 and out exactly that value row), a late
    start, an end beyond T (clamped).  Keys and values outside a window hold 1e6.
    Bound: _attention_bounds.  worst att 0.21, out 0.13 (MI355X)."""
    dk, nz, heads = cfg
    dh = dk // heads
    B = 4
    starts_all = np.array([0, T // 2, T // 3, 0])
    ends = np.array([T - 1, T // 2, T - 1, T + 5])
    worst_a = worst_o = 0.0
    for rpb in (1, 5):
        M = B * rpb
        g = _gen(1000 * T + dk + nz + rpb)
        q, k0, v0 = torch.randn(M, dk, generator=g), torch.randn(B, T, dk, generator=g), torch.randn(B, T, nz, generator=g)
        for use_start in (False, True):
            starts = starts_all if use_start else np.zeros(B, dtype=np.int64)
            k, v = k0.clone(), v0.clone()
            for b in range(B):
                outside = (torch.arange(T) < int(starts[b])) | (torch.arange(T) > int(ends[b]))
                k[b, outside], v[b, outside] = SENT, SENT
            for temp in (1.0, 0.02):
                r = R.attention(q, k, v, starts, ends, np.float32(temp), rpb, heads)
                tol_att, tol_out = _attention_bounds(r, v, rpb, heads, dh)
                for with_att in (True, False):
                    out, att = _run_attention(env, q, k, v, starts if use_start else None, ends, temp, rpb, heads, with_att)
                    name = f"T {T} cfg {cfg} rpb {rpb} start {use_start} temp {temp} att {with_att}"
                    worst_o = max(worst_o, _within(out, r["out"], tol_out, "attention out " + name))
                    if with_att:
                        worst_a = max(worst_a, _within(att, r["att"], tol_att, "attention att " + name))
                        assert bool((att[torch.from_numpy(~r["inside"])] == 0).all()), "weights outside the window are exact zeros"
                    if use_start:                                   # sequence 1: start == end
                        rows = slice(rpb, 2 * rpb)
                        _same(out[rows], v[1, T // 2].expand(rpb, nz), "out of a one-frame window is that value row, bit for bit")
                        if with_att:
                            assert bool((att[rows, T // 2] == 1).all())
    print(f"[ratio] attention T {T} cfg {cfg}: att {worst_a:.3g} out {worst_o:.3g}")


def test_attention_empty_window_row_is_nan(env):
    """include/gcpx.h: a row whose window is empty (start_ind > end_ind) is a softmax over nothing — out and att of that row are NaN,
    what the masking of the reference gives (oracle multihead_attention; tests/test_adaptive_refs_cpu.py) — and the rows of the other
    sequences of the same launch are within the bound of test_attention_matches_float64.  The kernel before this test wrote zeros to
    out (the value loop of an empty window never runs) beside a NaN att.  worst att 0.03, out 0.02 (MI355X)."""
    dk, nz, heads, T, rpb = 16, 64, 4, 37, 2
    g = _gen(77)
    q, k, v = torch.randn(3 * rpb, dk, generator=g), torch.randn(3, T, dk, generator=g), torch.randn(3, T, nz, generator=g)
    starts, ends = np.array([0, 5, 3]), np.array([36, 3, 40])
    r = R.attention(q, k, v, starts, ends, np.float32(0.8), rpb, heads)
    tol_att, tol_out = _attention_bounds(r, v, rpb, heads, dk // heads)
    out, att = _run_attention(env, q, k, v, starts, ends, 0.8, rpb, heads, True)
    assert bool(torch.isnan(out[2:4]).all()), "out of the empty-window rows"
    assert bool(torch.isnan(att[2:4]).all()), "att of the empty-window rows"
    ok = [0, 1, 4, 5]
    _within(out[ok], r["out"][ok], tol_out[ok], "attention out beside an empty window")
    _within(att[ok], r["att"][ok], tol_att[ok], "attention att beside an empty window")
    out2, _ = _run_attention(env, q, k, v, starts, ends, 0.8, rpb, heads, False)
    assert bool(torch.isnan(out2[2:4]).all()) and bool(torch.isfinite(out2[ok]).all())


# ------------------------------------------------------------------------------------------------------------------------------
# b. gcpx_cdist
# ------------------------------------------------------------------------------------------------------------------------------
_CDIST_SPLITS = {32: 1, 64: 2, 96: 1, 128: 4, 256: 8}


def _cdist_case(env, x, y, name):
    """Bound: the kernel evaluates |x|^2 + |y|^2 - 2 x.y in f32.  A norm: at most 4 ceil(K / 1024) fmas per thread and an 8-level
    tree; a dot product: K / splits MFMA multiply-adds and the serial sum of the split partials; then two adds (the doubling is exact)
    and a clamp at 0, which moves a result towards the true value (>= 0):
        tol = eps ((4 ceil(K/1024) + 10) (|x|^2 + |y|^2) + (K / splits + splits + 2) 2 sum |x_k y_k|)."""
    rt, lib, dev = env
    B, N, K = x.shape
    T = y.shape[1]
    ns = lib.gcpx_cdist_splits(K)
    part, xn, yn, out = _nan(ns * B * N * T), _nan(B * N), _nan(B * T), _nan(B * N * T + 7)
    xd, yd = x.to(dev), y.to(dev)
    rt.check(lib.gcpx_cdist(xd.data_ptr(), yd.data_ptr(), B, N, T, K, part.data_ptr(), xn.data_ptr(), yn.data_ptr(), out.data_ptr(),
                            _st()), "cdist")
    torch.cuda.synchronize()
    ref, _ = R.sqdist(x, y)
    x64, y64 = x.double(), y.double()
    norms = (x64 * x64).sum(-1)[:, :, None] + (y64 * y64).sum(-1)[:, None, :]
    cross = 2.0 * torch.bmm(x64.abs(), y64.abs().transpose(1, 2))
    tol = EPS * ((4 * math.ceil(K / 1024) + 10) * norms + (K // ns + ns + 2) * cross)
    got = out[:B * N * T].view(B, N, T)
    w = _within(got, ref, tol, "cdist " + name)
    assert float(got.min()) >= 0.0
    _untouched(out[B * N * T:], "out past B N T")
    assert bool(torch.isfinite(part).all()), "every split partial is written"
    return w, got.cpu(), tol


@pytest.mark.parametrize("K", sorted(_CDIST_SPLITS))
def test_cdist_matches_float64(env, K):
    """gcpx_cdist against the true sum of squared differences.  K = 32 ... 256 give 1, 2, 1, 4, 8 split-K partials (asserted), K = 32 a
    chunk of a single 32-step; N and T from 1, 63, 64, 65, 130 (one row, a tile less one, a tile, a tile plus one, three tiles).  One
    exact duplicate row: >= 0 and within the bound of 0.  Bound: _cdist_case.  worst 0.10 (MI355X)."""
    rt, lib, dev = env
    assert lib.gcpx_cdist_splits(K) == _CDIST_SPLITS[K]
    worst = 0.0
    for N, T in [(1, 1), (63, 65), (64, 64), (65, 130), (130, 63), (1, 130), (65, 1)]:
        g = _gen(K + 7 * N + T)
        x, y = torch.rand(2, N, K, generator=g) * 2 - 1, torch.rand(2, T, K, generator=g) * 2 - 1
        y[1, T - 1] = x[1, N // 2]
        w, got, tol = _cdist_case(env, x, y, f"K {K} N {N} T {T}")
        assert 0.0 <= float(got[1, N // 2, T - 1]) <= float(tol[1, N // 2, T - 1])
        worst = max(worst, w)
    print(f"[ratio] cdist K {K}: {worst:.3g}")


def test_cdist_finish_grid_stride(env):
    """B N T = 9 x 255 x 230 = 527 850 outputs at K = 32: more than the 2048 x 256 = 524 288 threads the finishing kernel's grid is
    capped at, so its last 3 562 outputs come from the second trip of the grid-stride loop.  worst 0.11 (MI355X)."""
    g = _gen(9)
    x, y = torch.rand(9, 255, 32, generator=g) * 2 - 1, torch.rand(9, 230, 32, generator=g) * 2 - 1
    assert 9 * 255 * 230 > 2048 * 256
    _cdist_case(env, x, y, "grid stride")


def test_cdist_cancellation(env):
    """x, y = 100 + 1e-2 noise: the distance (~1e-2) is seven decades below the norms (~1e6) it is the difference of.  A relative
    tolerance means nothing here; the abs-terms bound (~1) is what f32 can promise, and the kernel must still be inside it and >= 0.
    worst 0.13 (MI355X)."""
    g = _gen(10)
    for K in (32, 256):
        x, y = 100 + 1e-2 * torch.randn(2, 65, K, generator=g), 100 + 1e-2 * torch.randn(2, 63, K, generator=g)
        _cdist_case(env, x, y, f"cancellation K {K}")


# ------------------------------------------------------------------------------------------------------------------------------
# c. gcpx_soft_dtw / gcpx_soft_dtw_dtemp
# ------------------------------------------------------------------------------------------------------------------------------
def _soft_dtw_bounds(r, C, end):
    """acc: a row step is max + softplus_neg(min - max) + C: the subtraction rounds once and softplus has slope <= 1 with |x| e^x <= 1/e
    (0.37 u), softplus itself MATH_ULPS ulp of at most log 2 (2.8 u), two adds (u |D| each).  logaddexp is a convex combination of its
    arguments, so the errors of the rows above pass through with a factor <= 1 and add up:
        tol_acc[i][j] = steps (4 + 2 Dabs[i][j]) u,   steps = i + 1 (forward) or N - i (backward), Dabs the path bound of the reference.
    w: e = F + Bw - C - z inherits tol_F + tol_Bw + tol_z and three f64 adds; the f64 exp MATH_ULPS ulp; the cast to f32 eps:
        rel = tol_F + tol_Bw + tol_z + 3 u (Fabs + Bwabs + |C| + |z|) + MATH_ULPS ulp64 + eps.
    The column sum of at most N positive f32 terms is within N eps, the division eps:
        tol_w = w (rel + max over the column of rel + (N + 1) eps) + TINY."""
    B, N, T = C.shape
    steps_f = (np.arange(N) + 1.0)[None, :, None]
    steps_b = (N - np.arange(N) + 0.0)[None, :, None]
    tol_f = steps_f * (4 + 2 * r["fwd_abs"]) * U64
    tol_b = steps_b * (4 + 2 * r["bwd_abs"]) * U64
    reach = np.isfinite(r["fwd"]) & np.isfinite(r["bwd"])
    zabs = np.abs(r["z"])[:, None, None]
    tol_z = tol_f[np.arange(B), N - 1, np.asarray(end)][:, None, None]
    rel = np.where(reach, tol_f + tol_b + tol_z + 3 * U64 * (r["fwd_abs"] + r["bwd_abs"] + np.abs(C) + zabs)
                   + MATH_ULPS * ULP64 + EPS, 0.0)
    tol_w = r["w"] * (rel + rel.max(1, keepdims=True) + (N + 1) * EPS) + TINY
    return tol_f, tol_b, tol_w


def _run_soft_dtw(env, dsum, D, temp, end):
    rt, lib, dev = env
    B, N, T = dsum.shape
    acc, w = _nan(2 * B * N * T + 3, dtype=torch.float64), _nan(B * N * T + 3)
    dd, td, ed = dsum.to(dev), torch.tensor([temp], device=dev), torch.as_tensor(end, dtype=torch.int64).to(dev)
    status = lib.gcpx_soft_dtw(dd.data_ptr(), D, td.data_ptr(), ed.data_ptr(), B, N, T, acc.data_ptr(), w.data_ptr(), _st())
    torch.cuda.synchronize()
    return status, acc, w, (dd, td, ed)


def _check_soft_dtw(env, dsum, D, temp, end, name):
    rt = env[0]
    B, N, T = dsum.shape
    status, acc, w, keep = _run_soft_dtw(env, dsum, D, temp, end)
    rt.check(status, "soft_dtw")
    cost = R.f32_cost(dsum.numpy(), D, temp)
    r = R.soft_dtw(cost, end)
    tol_f, tol_b, tol_w = _soft_dtw_bounds(r, -cost.astype(np.float64), end)
    _untouched(acc[2 * B * N * T:], "acc past 2 B N T")
    _untouched(w[B * N * T:], "w past B N T")
    got = acc[:2 * B * N * T].view(2, B, N, T).cpu().numpy()
    assert not np.isnan(got).any(), f"{name}: {int(np.isnan(got).sum())} cells of acc not written"
    worst = {}
    for half, key, tol in ((0, "fwd", tol_f), (1, "bwd", tol_b)):
        ref = r[key]
        assert np.array_equal(np.isinf(got[half]), np.isinf(ref)), f"{name}: the -inf pattern of {key} differs"
        fin = np.isfinite(ref)
        worst[key] = _within(got[half][fin], ref[fin], tol[fin], f"soft_dtw {key} {name}")
    wg = w[:B * N * T].view(B, N, T).cpu()
    worst["w"] = _within(wg, r["w"], tol_w, f"soft_dtw w {name}")
    for b in range(B):
        e = int(end[b])
        assert bool((wg[b, :, e + 1:] == 0).all()), "columns beyond end_ind are exact zeros"
    return worst, r, wg, acc, keep


@pytest.mark.parametrize("shape", [(64, 64), (70, 65), (300, 257), (511, 300), (600, 513), (1024, 1024)], ids=lambda s: "%dx%d" % s)
def test_soft_dtw_matches_float64(env, shape):
    """gcpx_soft_dtw: both accumulators (float64, -inf pattern equal) and the normalised w against R.soft_dtw on the f32 cost
    (dsum / D) / temp.  T = 64, 65 launch the combine with 4 node groups, 257 and 300 with 2, 513 and 1024 with 1; N == T leaves one
    alignment (the diagonal) when end = T - 1; end_ind 0 (the alignment goes down column 0: w[:, 0] = 1 / N after the normalisation,
    every other column exact zeros), T - 1 and between.  Unit-scale costs, and costs with cost / temp up to 2000: neighbouring
    accumulators differ by far more than 745, where softplus_neg returns its 0.  Every cell of acc and w is written.
    Bound: _soft_dtw_bounds.  worst fwd 0.07, bwd 0.10, w 0.05 (MI355X)."""
    N, T = shape
    B = 2
    worst = {"fwd": 0.0, "bwd": 0.0, "w": 0.0}
    g = _gen(N + T)
    dsum = torch.rand(B, N, T, generator=g) * 48.0
    for ends in ([0, T - 1], [T // 2, max(T - 2, 0)]):
        for temp in (0.7, 5e-4):
            wr, r, wg, _, _ = _check_soft_dtw(env, dsum, 48.0, temp, np.array(ends), f"{N}x{T} end {ends} temp {temp}")
            worst = {k: max(worst[k], wr[k]) for k in worst}
            if ends[0] == 0:
                assert np.allclose(r["w_raw"][0, :, 0], 1.0, atol=1e-9) and abs(float(wg[0, :, 0].double().mean()) * N - 1) < 1e-5
    print(f"[ratio] soft_dtw {N}x{T}: {worst}")


def test_soft_dtw_refuses_more_than_1024_frames(env):
    """T = 1025: GCPX_ERR_UNSUPPORTED and nothing launched — w and acc keep their NaN"""
    status, acc, w, _ = _run_soft_dtw(env, torch.rand(1, 1025, 1025, generator=_gen(1)), 1.0, 1.0, np.array([1024]))
    assert status == UNSUPPORTED, status
    _untouched(w, "w after the refused call")
    _untouched(acc, "acc after the refused call")


@pytest.mark.parametrize("shape", [(70, 65), (511, 300), (600, 513)], ids=lambda s: "%dx%d" % s)
def test_soft_dtw_dtemp_matches_float64_autograd(env, shape):
    """gcpx_soft_dtw_dtemp against float64 autograd of R.soft_dtw_torch (R.soft_dtw_dtemp), on the accumulators gcpx_soft_dtw left.
    T = 65 / 300 / 513: the combine with 4 / 2 / 1 node groups.  A pad mask that is not (t <= end_ind): one frame inside masked out, one
    weighted 0.5.  The gradient slot starts at 0.25 (the kernel accumulates); two launches give equal bits.
    Bound: the gradient is linear in the cost derivative Cdot = cost / temp, which the kernel forms with one f32 rounding less than
    the reference: eps x abs1 (abs-terms over the cells).  The combine rounds the weights to f32 before its four float64 column sums
    S, SD, A, Q; in (A - Q SD / S) / S that is eps on A, on Q, on SD and on each of the two 1 / S: at most 4 eps x abs2 (abs-terms of
    the combine).  Float64 sums of at most N + T + 10 terms: (N + T + 10) u (abs1 + abs2).  The cast of the result to f32 and its add
    to 0.25: 2 eps (0.25 + |g|).
        tol = eps (abs1 + 4 abs2) + (N + T + 10) u (abs1 + abs2) + 2 eps (0.25 + |g|).   worst 0.0009 (MI355X): the bound takes every
    f32 rounding of a weight as adverse, the measured error is that of the final cast."""
    rt, lib, dev = env
    N, T = shape
    B, D, coef, ls, temp = 2, 3.0, 0.37, 0.2, 0.4
    g = _gen(3 * N + T)
    dsum = torch.rand(B, N, T, generator=g) * 1.5 * D
    end = np.array([T - 1, T // 2])
    pad = (torch.arange(T)[None] <= torch.as_tensor(end)[:, None]).float()
    pad[0, 1], pad[1, 0], pad[1, T - 1] = 0.0, 0.5, 0.25
    status, acc, w, (dd, td, ed) = _run_soft_dtw(env, dsum, D, temp, end)
    rt.check(status, "soft_dtw")
    want, abs1, abs2 = R.soft_dtw_dtemp(dsum.numpy(), D, temp, end, pad.numpy(), float(np.float32(ls)), float(np.float32(coef)))
    tol = EPS * (abs1 + 4 * abs2) + (N + T + 10) * U64 * (abs1 + abs2) + 2 * EPS * (0.25 + abs(want))
    pd_, lsd = pad.to(dev), torch.tensor([ls], device=dev)
    got = []
    for _ in range(2):
        tan, part = _nan(2 * B * N * T, dtype=torch.float64), _nan(B, dtype=torch.float64)
        slot = torch.full((1,), 0.25, device=dev)
        rt.check(lib.gcpx_soft_dtw_dtemp(dd.data_ptr(), D, td.data_ptr(), ed.data_ptr(), acc.data_ptr(), pd_.data_ptr(), lsd.data_ptr(),
                                         coef, B, N, T, tan.data_ptr(), part.data_ptr(), slot.data_ptr(), _st()), "soft_dtw_dtemp")
        torch.cuda.synchronize()
        assert bool(torch.isfinite(tan).all()) and bool(torch.isfinite(part).all()), "every tangent cell and partial is written"
        got.append(float(slot))
    assert got[0] == got[1], "two launches: equal bits"
    assert abs(want) > 1e-3
    err = abs(got[0] - 0.25 - want)
    print(f"[ratio] soft_dtw_dtemp {N}x{T}: got {got[0] - 0.25!r} want {want!r} abs1 {abs1:.3g} abs2 {abs2:.3g} err/tol {err / tol:.3g}")
    assert err <= tol, (got[0] - 0.25, want, err, tol)


# ------------------------------------------------------------------------------------------------------------------------------
# d. gcpx_match_stats / gcpx_distance_prune
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("LT", [(1, 1), (4, 12), (7, 65), (8, 200)], ids=lambda s: "L%d-T%d" % s)
def test_match_stats_matches_reference(env, LT):
    """gcpx_match_stats against R.match_stats.  N = 1, 15, 127, 255 and T = 1, 12, 65, 200: one to four trips of either lane-stride
    loop.  The values come from {0, 1/16, 1/8, 1/4, 1/2, 1e-30 (as f32)}: every comparison is exact and ties are everywhere, so every
    arg-max is checked, none excluded.  Planted on top: equal maxima at breadth-first q and q + 64 (two trips of ONE lane: the first
    wins), at two lanes, at the root and its left child (the root is breadth-first 0 but depth-first N / 2: breadth-first order
    decides); equal maxima at frames t and t + 64 and at two lanes; all-zero columns (-> root) and rows (-> frame 0, entropy 0);
    rows that sum above 1 (p_n clamps to exactly 1) and below.  matched_idx given and NULL.
    Bounds: entropy = -sum p logf(p): logf MATH_ULPS ulp and a product per term, then ceil(T / 64) serial adds and a 6-level
    butterfly: (ceil(T/64) + 6 + 2 MATH_ULPS + 1) eps x abs-terms; p_n the same sum without the logarithm: (ceil(T/64) + 6) eps x
    abs-terms.  worst entropy 0.12, p_n 0 (its sums of sixteenths are exact) (MI355X)."""
    from oracle import tree_index_oracle as TI
    rt, lib, dev = env
    L, T = LT
    N, B = 2 ** L - 1, 3
    perm = TI.bf2df_perm(L)
    g = _gen(17 * L + T)
    table = torch.tensor([0.0, 0.0625, 0.125, 0.25, 0.5, 1e-30])
    w = table[torch.randint(0, 6, (B, N, T), generator=g)]
    rho = torch.rand(B, N, 1, generator=g) * min(1.0, 16.0 / T) if T > 1 else torch.ones(B, N, 1)
    w = torch.where(torch.rand(B, N, T, generator=g) < rho, w, torch.zeros(()))
    if T >= 12:
        w[:, :, T - 2:] = 0.0                                     # padded frames: all-zero columns
    if N >= 15:                                                   # rows in sequence 0, columns in sequences 1 and 2
        w[2, 5] = 0.0                                             # a node no frame matches
        w[0, 3, :] = 0.0; w[0, 3, 4] = w[0, 3, 7] = 0.75                      # two lanes
        w[1, :, 1] = 0.0; w[1, perm[5], 1] = w[1, perm[9], 1] = 0.75          # two lanes
        w[1, :, 2] = 0.0; w[1, perm[1], 2] = w[1, perm[0], 2] = 0.75          # left child against the root
    if N > 67:
        w[1, :, 0] = 0.0; w[1, perm[3], 0] = w[1, perm[67], 0] = 0.75         # q and q + 64: one lane, two trips
        w[2, :, 3] = 0.0; w[2, perm[70], 3] = w[2, perm[6], 3] = 0.5
    if T > 64:
        w[0, 2, :] = 0.0; w[0, 2, 0] = w[0, 2, 64] = 0.75                     # t and t + 64: one lane, two trips
    end = np.array([T - 1, T // 2, 0])
    r = R.match_stats(w.numpy(), end, L)
    if N >= 15:
        assert r["frame2node"][1, 1] == perm[5] and r["frame2node"][1, 2] == perm[0] and r["best_t"][0, 3] == 4
        assert (r["p_abs"] > 1.01).any() and ((r["p_abs"] < 0.9) & (r["p_abs"] > 0)).any() and (r["p_abs"] == 0).any()
    if N > 67:
        assert r["frame2node"][1, 0] == perm[3] and r["frame2node"][2, 3] == perm[6]
    if T > 64:
        assert r["best_t"][0, 2] == 0
    wd, ed = w.to(dev), torch.as_tensor(end, dtype=torch.int64).to(dev)
    nt = math.ceil(T / 64) + 6
    for with_midx in (True, False):
        f2n, midx, best = _isent(B * T + 3), (_isent(B * T + 3) if with_midx else None), _isent(B * N + 3)
        ent, pn = _nan(B * N + 3), _nan(B * N + 3)
        rt.check(lib.gcpx_match_stats(wd.data_ptr(), ed.data_ptr(), B, L, T, f2n.data_ptr(), rt.ptr(midx), best.data_ptr(), ent.data_ptr(),
                                      pn.data_ptr(), _st()), "match_stats")
        torch.cuda.synchronize()
        _same(f2n[:B * T].view(B, T), r["frame2node"], "frame2node")
        if with_midx:
            _same(midx[:B * T].view(B, T), r["matched_idx"], "matched_idx")
            _untouched(midx[B * T:], "matched_idx tail", ISENT)
        _same(best[:B * N].view(B, N), r["best_t"], "best_t")
        _within(ent[:B * N].view(B, N), r["entropy"], (nt + 2 * MATH_ULPS + 1) * EPS * r["entropy_abs"], f"entropy L {L} T {T}")
        _within(pn[:B * N].view(B, N), r["p_n"], nt * EPS * r["p_abs"], f"p_n L {L} T {T}")
        assert bool((pn[:B * N].cpu()[torch.from_numpy(r["p_abs"].reshape(-1) > 1.01)] == 1).all()), "sums above 1 clamp to exactly 1"
        for t_, nm in ((f2n[B * T:], "frame2node"), (best[B * N:], "best_t")):
            _untouched(t_, nm + " tail", ISENT)
        _untouched(ent[B * N:], "entropy tail")
        _untouched(pn[B * N:], "p_n tail")


@pytest.mark.parametrize("N", [2, 64, 65, 255])
def test_distance_prune_matches_reference(env, N):
    """gcpx_distance_prune against R.distance_prune: N = 2, 64 (one trip of the 64-node loop, full), 65 (a second trip of one node), 255
    (four trips: the compaction base carried over three boundaries).  Sequences: all kept (no exclusion: count = N, no -1 tail), only
    the root kept, alternating, two random ones.  dist comes from the grid {-3, -1, -0.5, 0.5, 1, 3} and 0: at thresholds 0.5 and 0.7
    every sigmoid is at least 1e-3 from the threshold (asserted) except sigmoid(0) = 0.5 = threshold exactly, which is not above it:
    kept.  target given and NULL.  All outputs are integers: exact."""
    rt, lib, dev = env
    g = _gen(N)
    grid = torch.tensor([-3.0, -1.0, -0.5, 0.5, 1.0, 3.0, 0.0])
    B = 5
    dist = torch.empty(B, N - 1)
    dist[0], dist[1] = -3.0, 3.0
    dist[2] = torch.where(torch.arange(N - 1) % 2 == 0, torch.tensor(3.0), torch.tensor(-3.0))
    dist[3] = grid[torch.randint(0, 6, (N - 1,), generator=g)]
    dist[4] = grid[torch.randint(0, 7, (N - 1,), generator=g)]
    dist[4, 0] = 0.0
    best = torch.randint(0, 3, (B, N), generator=g, dtype=torch.int32)
    dd, bd = dist.to(dev), best.to(dev)
    for thr in (0.5, 0.7):
        r = R.distance_prune(dist.numpy(), thr, best.numpy())
        m = np.abs(r["sig"] - thr)
        assert np.all((m >= 1e-3) | ((dist.numpy() == 0) & (thr == 0.5)))
        assert r["count"][0] == N and r["count"][1] == 1
        if thr == 0.5:
            assert r["leave"][4, 1] == 1                           # the exact-equality node
        for with_target in (True, False):
            leave, kept, cnt = _isent(B * N + 3), _isent(B * N + 3), _isent(B + 3)
            tgt = _isent(B * (N - 1) + 3) if with_target else None
            rt.check(lib.gcpx_distance_prune(dd.data_ptr(), thr, rt.ptr(bd if with_target else None), B, N, leave.data_ptr(),
                                             kept.data_ptr(), cnt.data_ptr(), rt.ptr(tgt), _st()), "distance_prune")
            torch.cuda.synchronize()
            _same(leave[:B * N].view(B, N), r["leave"], f"leave N {N} thr {thr}")
            _same(kept[:B * N].view(B, N), r["kept_idx"], f"kept_idx N {N} thr {thr}")
            _same(cnt[:B], r["count"], f"count N {N} thr {thr}")
            for t_, nm in ((leave[B * N:], "leave"), (kept[B * N:], "kept_idx"), (cnt[B:], "count")):
                _untouched(t_, nm + " tail", ISENT)
            if with_target:
                _same(tgt[:B * (N - 1)].view(B, N - 1), r["target"], f"target N {N}")
                _untouched(tgt[B * (N - 1):], "target tail", ISENT)


# ------------------------------------------------------------------------------------------------------------------------------
# e. gcpx_averaging_nll / gcpx_soft_average
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [48, 12288])
@pytest.mark.parametrize("NT", [(1, 1), (3, 63), (15, 64), (255, 65), (255, 200)], ids=lambda s: "%dx%d" % s)
def test_averaging_nll_matches_float64(env, NT, D):
    """gcpx_averaging_nll against R.averaging_nll.  T = 65 and 200 need a second (fourth) 64-frame block, N = 1 and 3 leave node groups
    empty; D = 12288 makes the constant term D (ls + 0.5 log 2 pi) about 1e4 times the data term; log_sigma -1 (the constant nearly
    cancels: its abs-terms are D (|ls| + 0.919)) and 0.3.
    Bound: expf(-ls) MATH_ULPS ulp (4 eps), squared 9 eps, times 0.5 dsum 10 eps; the constant: its f32 value, an add and a product, 3
    eps; their sum 11, times w 12; then ceil(N / 4) adds per node group and 2 for the four groups:
        tol = (ceil(N / 4) + 14) eps x abs-terms.   worst 0.15 (MI355X)."""
    rt, lib, dev = env
    N, T = NT
    B = 2
    g = _gen(N + T + D)
    w = torch.rand(B, N, T, generator=g)
    w = w / w.sum(1, keepdim=True)
    dsum = torch.rand(B, N, T, generator=g) * 0.2 * D
    wd, dd = w.to(dev), dsum.to(dev)
    worst = 0.0
    for ls in (-1.0, 0.3):
        nll = _nan(B * T + 3)
        lsd = torch.tensor([ls], device=dev)
        rt.check(lib.gcpx_averaging_nll(dd.data_ptr(), wd.data_ptr(), lsd.data_ptr(), float(D), B, N, T, nll.data_ptr(), _st()), "averaging_nll")
        torch.cuda.synchronize()
        ref, ab = R.averaging_nll(dsum.numpy(), w.numpy(), float(np.float32(ls)), float(D))
        worst = max(worst, _within(nll[:B * T].view(B, T), ref, (math.ceil(N / 4) + 14) * EPS * ab, f"averaging_nll {N}x{T} D {D} ls {ls}"))
        _untouched(nll[B * T:], "nll past B T")
    print(f"[ratio] averaging_nll {N}x{T} D {D}: {worst:.3g}")


@pytest.mark.parametrize("D", [48, 65, 256, 300])
def test_soft_average_matches_float64(env, D):
    """gcpx_soft_average against R.soft_average.  D = 65 and 300 put live columns into the wavefronts 1 - 3 of a workgroup (d0 = 256
    blockIdx.x + 64 wave) and, at 300, into a second workgroup, with a partial last 16-column tile; T = 1, 31, 32, 33: one row, a tile
    less one, a tile, a second 32-row tile of one row; N = 1, 3, 4, 5, 255: the k loop of 4 with every remainder.  1e6 stands behind
    the last row of w and of x (nothing may be read there); out has NaN behind its last row.
    Bound: one rounding per MFMA multiply-add over the N nodes: (N + 1) eps x abs-terms.  worst 0.63 (MI355X; 0.5 at N = 1)."""
    rt, lib, dev = env
    B = 2
    worst = 0.0
    for T in (1, 31, 32, 33):
        for N in (1, 3, 4, 5, 255):
            g = _gen(D + 31 * T + N)
            w, x = torch.rand(B, N, T, generator=g), torch.randn(B, N, D, generator=g)
            wbuf, xbuf = torch.full((B * N * T + 64,), SENT), torch.full((B * N * D + 4 * D,), SENT)
            wbuf[:B * N * T], xbuf[:B * N * D] = w.flatten(), x.flatten()
            wd, xd = wbuf.to(dev), xbuf.to(dev)
            out = _nan(B * T * D + D)
            rt.check(lib.gcpx_soft_average(wd.data_ptr(), xd.data_ptr(), out.data_ptr(), B, N, T, D, _st()), "soft_average")
            torch.cuda.synchronize()
            ref, ab = R.soft_average(w.numpy(), x.numpy())
            worst = max(worst, _within(out[:B * T * D].view(B, T, D), ref, (N + 1) * EPS * ab, f"soft_average D {D} T {T} N {N}"))
            _untouched(out[B * T * D:], "out past B T rows")
    print(f"[ratio] soft_average D {D}: {worst:.3g}")


# ------------------------------------------------------------------------------------------------------------------------------
# f. gcpx_dtw_align
# ------------------------------------------------------------------------------------------------------------------------------
def _check_dtw_align(env, C, n_len, t_len, name):
    rt, lib, dev = env
    B, N, T = C.shape
    acc = _nan(B * N * T + 3, dtype=torch.float64)
    inds, path, plen = _isent(B * T + 3), _isent(B * 2 * (N + T) + 3), _isent(B + 3)
    dist = _nan(B + 3, dtype=torch.float64)
    cd = C.to(dev)
    nd = None if n_len is None else torch.as_tensor(n_len, dtype=torch.int32).to(dev)
    td = None if t_len is None else torch.as_tensor(t_len, dtype=torch.int32).to(dev)
    rt.check(lib.gcpx_dtw_align(cd.data_ptr(), rt.ptr(nd), rt.ptr(td), B, N, T, acc.data_ptr(), inds.data_ptr(), path.data_ptr(),
                                plen.data_ptr(), dist.data_ptr(), _st()), "dtw_align")
    torch.cuda.synchronize()
    res = R.dtw_align(C.numpy(), n_len, t_len)
    accv, pathv = acc[:B * N * T].view(B, N, T).cpu(), path[:B * 2 * (N + T)].view(B, 2, N + T).cpu()
    for b, r in enumerate(res):
        n, t = r["n"], r["t"]
        _same(accv[b, :n, :t], r["acc"], f"{name}: acc of sequence {b}")
        outside = torch.ones(N, T, dtype=torch.bool)
        outside[:n, :t] = False
        _untouched(accv[b][outside], f"{name}: acc outside {n} x {t}")
        ln = int(plen[b])
        assert ln == len(r["path"][0]), f"{name}: path_len {ln} against {len(r['path'][0])}"
        _same(pathv[b, 0, :ln].flip(0), r["path"][0], f"{name}: path rows of sequence {b}")
        _same(pathv[b, 1, :ln].flip(0), r["path"][1], f"{name}: path columns of sequence {b}")
        _untouched(pathv[b, :, ln:], f"{name}: path beyond path_len", ISENT)
        _same(inds[b * T:(b + 1) * T], r["inds"], f"{name}: inds of sequence {b}")
        assert float(dist[b]) == r["dist"], (name, b, float(dist[b]), r["dist"])
    for t_, nm, fill in ((acc[B * N * T:], "acc", NAN), (dist[B:], "dist", NAN), (inds[B * T:], "inds", ISENT), (plen[B:], "path_len", ISENT),
                         (path[B * 2 * (N + T):], "path", ISENT)):
        _untouched(t_, f"{name}: {nm} tail", fill)


def test_dtw_align_ragged_lengths_and_ties(env):
    """gcpx_dtw_align against oracle dtw_matches on every sequence's own n_len x t_len corner (R.dtw_align).  B = 3 at N x T = 300 x 280:
    the full lattice (diagonals of up to 280 cells: the `i += 256` stride runs a second trip), a ONE-ROW lattice (1 x 9) and a
    ONE-COLUMN lattice (37 x 1).  The costs are the integers 0, 1, 2 (as f32): the float64 accumulation is exact, equal neighbours are
    everywhere, and the rule diagonal before up before left decides the path — so acc, path, path_len, inds and dist are compared
    bit for bit.  Cells of acc outside n_len x t_len and path entries beyond path_len keep their fill; inds beyond t_len is -1."""
    g = _gen(4)
    C = torch.randint(0, 3, (3, 300, 280), generator=g).float()
    _check_dtw_align(env, C, [300, 1, 37], [280, 9, 1], "ragged")


def test_dtw_align_null_lengths_and_real_costs(env):
    """n_len = t_len = NULL (every sequence is N x T) at 70 x 300, the diagonals' other orientation (more frames than estimates), with
    real-valued costs: the kernel and the reference do the same float64 operations in the same order, so the comparison stays exact."""
    g = _gen(5)
    C = torch.rand(2, 70, 300, generator=g)
    _check_dtw_align(env, C, None, None, "null lengths")
