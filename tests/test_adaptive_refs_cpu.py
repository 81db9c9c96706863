"""The float64 references of tests/adaptive_refs.py, pinned on the CPU: a GPU test that agrees with a wrong reference proves nothing.
Soft-DTW against the goldens of the executed reference (tests/golden/ref_dtw.npz, ref_dtw_dtemp.npz), the rest against
oracle/adaptive_oracle.py at small shapes, the tie and empty-column rules against arrays written by hand."""
import math
import os

import numpy as np
import pytest
import torch

import adaptive_refs as R
from oracle import adaptive_oracle as A

GOLD = os.path.join(os.path.dirname(__file__), "golden")
G = np.load(os.path.join(GOLD, "ref_dtw.npz"))
GT = np.load(os.path.join(GOLD, "ref_dtw_dtemp.npz"))


@pytest.mark.parametrize("i", range(int(G["sd_n"])))
def test_soft_dtw_reference_matches_executed_goldens(i):
    """forward accumulator to 1e-11 and expected edge frequencies to 1e-6: the precision the fixture was stored with"""
    cost, end = G[f"sd{i}_cost"], G[f"sd{i}_end"]
    r = R.soft_dtw(cost, end)
    ref = G[f"sd{i}_fwd"]
    assert np.array_equal(np.isinf(r["fwd"]), np.isinf(ref))
    fin = ~np.isinf(ref)
    assert np.max(np.abs(r["fwd"][fin] - ref[fin])) < 1e-11
    assert np.all(r["fwd_abs"][fin] >= np.abs(ref[fin]))                       # the path bound is a bound
    assert np.max(np.abs(r["w_raw"] - G[f"sd{i}_w"])) < 1e-6
    want = A.normalize(torch.tensor(G[f"sd{i}_w"]).double(), 1).numpy()
    assert np.max(np.abs(r["w"] - want)) < 2e-6
    # the torch restatement gives the same numbers
    wt = R.soft_dtw_torch(-torch.from_numpy(cost).double(), end).numpy()
    assert np.max(np.abs(wt - r["w"])) < 1e-12
    # the backward accumulator, in the orientation of the cost, against the oracle's flipped problem
    B = cost.shape[0]
    C = -cost.astype(np.float64)
    bwd = A.fast_gak(C[:, ::-1, ::-1], cost.shape[2] - end - 1)[:, ::-1, ::-1]
    assert np.array_equal(np.isinf(r["bwd"]), np.isinf(bwd))
    fb = ~np.isinf(bwd)
    assert np.max(np.abs(r["bwd"][fb] - bwd[fb])) < 1e-11


def test_soft_dtw_reference_edges():
    """end = 0: the only alignment goes down column 0, so the raw w[:, 0] is 1 and the normalised one 1 / N; N == T with end = T - 1:
    the only alignment is the diagonal; costs whose neighbours differ by far more than 745: no NaN, columns still sum to one."""
    g = np.random.RandomState(0)
    cost = g.rand(2, 6, 6).astype(np.float32)
    r = R.soft_dtw(cost, np.array([0, 5]))
    assert np.allclose(r["w_raw"][0, :, 0], 1.0, atol=1e-14) and np.all(r["w_raw"][0, :, 1:] == 0)
    assert np.allclose(r["w"][0, :, 0], 1.0 / 6, atol=1e-14)
    assert np.allclose(r["w"][1], np.eye(6), atol=1e-14)
    sharp = R.soft_dtw(cost * 2000 * 6, np.array([3, 5]))
    assert np.all(np.isfinite(sharp["w"]))
    assert np.allclose(sharp["w"][0].sum(0)[:4], 1.0, atol=1e-12) and np.all(sharp["w"][0][:, 4:] == 0)


@pytest.mark.parametrize("i", range(int(GT["n"])))
def test_soft_dtw_temperature_derivative_matches_central_differences(i):
    """the torch restatement differentiated w.r.t. the temperature, cell by cell against central differences of the executed
    reference (tolerance of tests/test_adaptive_oracle.py), and the scalar soft_dtw_dtemp against the same differences"""
    cost, end, t0, h = torch.from_numpy(GT[f"c{i}_cost"]), GT[f"c{i}_end"], float(GT[f"c{i}_temp"]), float(GT["h"])
    t = torch.full((1,), t0, dtype=torch.float64)
    _, dw = torch.autograd.functional.jvp(lambda tv: R.soft_dtw_torch(-(cost.double() / tv), end, normalised=False), t,
                                          torch.ones(1, dtype=torch.float64))
    fd = (GT[f"c{i}_w_plus"].astype(np.float64) - GT[f"c{i}_w_minus"]) / (2 * h)
    scale = np.abs(fd).max()
    assert scale > 1e-3
    assert np.max(np.abs(dw.numpy() - fd)) < 5e-4 * scale + 5e-5
    # the criterion's gradient: D = 1 and dsum = cost * temp make f32_cost the golden's cost up to f32 rounding
    B, N, T = cost.shape
    pad = (np.arange(T)[None] <= end[:, None]).astype(np.float32)
    pad[0, 1] = 0.0
    D, ls, coef = 3.0, 0.2, 0.37
    dsum = (cost * D).numpy()
    g, abs1, abs2 = R.soft_dtw_dtemp(dsum, D, t0, end, pad, ls, coef)
    assert abs1 >= abs(g) and abs2 >= abs(g) * (1 - 1e-9)
    # the forward-mode tangent behind abs2 reproduces the autograd gradient
    c64 = R.f32_cost(dsum, D, t0).astype(np.float64)
    wr, wd = R.soft_dtw_tangent(R.soft_dtw(c64, end), c64 / float(np.float32(t0)), end)
    S = wr.sum(1, keepdims=True)
    Ss = np.where(S > 0, S, 1.0)
    dn = np.where(S > 0, (wd - wr * wd.sum(1, keepdims=True) / Ss) / Ss, 0.0)
    gl = 0.5 * dsum.astype(np.float64) * math.exp(-2 * ls) + D * (ls + 0.5 * math.log(2 * math.pi))
    assert abs(coef * float((gl * dn * pad[:, None, :]).sum()) - g) < 1e-10 * abs1
    tt = torch.full((1,), t0, requires_grad=True)
    w = A.normalize(A.soft_dtw_autograd((torch.from_numpy(dsum) / D) / tt, end), 1)
    val = 0.5 * torch.from_numpy(dsum) * math.exp(-2 * ls) + D * (ls + 0.5 * math.log(2 * math.pi))
    (want,) = torch.autograd.grad(coef * (val * w * torch.from_numpy(pad)[:, None]).sum(), tt)
    assert abs(g - float(want)) <= 2e-5 * abs(float(want)) + 1e-6, (g, float(want))


def test_squared_distance_reference():
    g = torch.Generator().manual_seed(0)
    x, y = torch.randn(2, 5, 32, generator=g), torch.randn(2, 7, 32, generator=g)
    y[1, 3] = x[1, 2]
    out, ab = R.sqdist(x, y)
    want = A.batch_cdist(x.double(), y.double(), "sum")
    assert float((out - want).abs().max()) < 1e-12
    assert float(out[1, 2, 3]) == 0.0 and bool((out >= 0).all()) and bool((ab >= out).all())
    # the cancellation case: the true value, where the quadratic expansion in f32 has lost every digit
    x2, y2 = 100 + 1e-2 * torch.randn(1, 3, 32, generator=g), 100 + 1e-2 * torch.randn(1, 3, 32, generator=g)
    o2, a2 = R.sqdist(x2, y2)
    assert float(o2.max()) < 0.05 and float(a2.min()) > 1e6


@pytest.mark.parametrize("heads", [1, 2])
def test_attention_reference_matches_oracle(heads):
    from video_gcp_amd.hparams import config
    hp = config("c5s", n_attention_heads=heads)
    g = torch.Generator().manual_seed(2)
    B, T, n, dk, nz = 3, 11, 2, hp.nz_attn_key, hp.nz_enc
    M = B * n
    q, k, v = torch.randn(M, dk, generator=g), torch.randn(B, T, dk, generator=g), torch.randn(B, T, nz, generator=g)
    start, end = torch.tensor([0, 2, 4]), torch.tensor([10, 2, 20])
    sd = {"a.temperature": torch.tensor([0.8])}
    for nm, d in (("q_proj", dk), ("k_proj", dk), ("v_proj", nz), ("out_proj", nz)):
        sd[f"a.{nm}.weight"], sd[f"a.{nm}.bias"] = torch.eye(d), torch.zeros(d)
    rep = lambda t: t.repeat_interleave(n, 0)
    want_o, want_a = A.multihead_attention(sd, "a", hp, q, rep(k), rep(v), rep(start), rep(end))
    r = R.attention(q, k, v, start.numpy(), end.numpy(), 0.8, n, heads)
    assert np.max(np.abs(r["att"] - want_a.numpy())) < 1e-6 and np.max(np.abs(r["out"] - want_o.numpy())) < 1e-5
    assert np.all(r["att"][2:4, 2] == 1.0) and np.array_equal(r["out"][2], v[1, 2].double().numpy())   # start == end
    assert np.all(r["score_abs"] >= np.abs(r["score"]) - 1e-15)
    # start == None is start 0
    r0 = R.attention(q, k, v, None, end.numpy(), 0.8, n, heads)
    w0, a0 = A.multihead_attention(sd, "a", hp, q, rep(k), rep(v), torch.zeros(M, dtype=torch.long), rep(end))
    assert np.max(np.abs(r0["att"] - a0.numpy())) < 1e-6


def test_attention_reference_empty_window_is_nan_like_the_oracle():
    from video_gcp_amd.hparams import config
    hp = config("c5s", n_attention_heads=1)
    g = torch.Generator().manual_seed(3)
    dk, nz, T = hp.nz_attn_key, hp.nz_enc, 6
    q, k, v = torch.randn(3, dk, generator=g), torch.randn(3, T, dk, generator=g), torch.randn(3, T, nz, generator=g)
    start, end = torch.tensor([0, 4, 1]), torch.tensor([5, 2, 3])
    sd = {"a.temperature": torch.tensor([1.0])}
    for nm, d in (("q_proj", dk), ("k_proj", dk), ("v_proj", nz), ("out_proj", nz)):
        sd[f"a.{nm}.weight"], sd[f"a.{nm}.bias"] = torch.eye(d), torch.zeros(d)
    want_o, want_a = A.multihead_attention(sd, "a", hp, q, k, v, start, end)
    r = R.attention(q, k, v, start.numpy(), end.numpy(), 1.0, 1, 1)
    assert bool(torch.isnan(want_o[1]).all()) and bool(torch.isnan(want_a[1]).all())
    assert np.all(np.isnan(r["out"][1])) and np.all(np.isnan(r["att"][1]))
    assert np.all(np.isfinite(r["out"][[0, 2]])) and np.all(np.isfinite(r["att"][[0, 2]]))


def test_match_stats_reference_tie_and_empty_column_rules():
    """L = 2: depth-first (left, root, right) = breadth-first (1, 0, 2).  Written by hand."""
    w = np.zeros((1, 3, 5), dtype=np.float32)
    w[0, :, 0] = [0.5, 0.5, 0.5]        # three-way tie: breadth-first 0 is the root, depth-first 1
    w[0, :, 1] = [0.5, 0.25, 0.5]       # tie left / right: breadth-first 1 (left, depth-first 0) comes first
    w[0, :, 2] = [0.0, 0.0, 0.0]        # empty column -> root
    w[0, :, 3] = [0.25, 0.0, 0.5]       # right
    w[0, :, 4] = [0.0, 0.0, 0.0]
    r = R.match_stats(w, np.array([2]), 2)
    assert r["frame2node"].tolist() == [[1, 0, 1, 2, 1]]
    assert r["matched_idx"].tolist() == [[1, 0, 1, -1, -1]]
    assert r["best_t"].tolist() == [[0, 0, 0]]                                # first maximum over frames
    assert r["p_n"].tolist() == [[1.0, 0.75, 1.0]]                            # 1.25, 0.75, 1.5 clamped
    want = -(2 * 0.5 * math.log(0.5) + 0.25 * math.log(0.25))
    assert abs(r["entropy"][0, 0] - want) < 1e-15 and r["entropy"].shape == (1, 3)
    z = R.match_stats(np.zeros((1, 1, 1)), np.array([0]), 1)
    assert z["frame2node"].tolist() == [[0]] and z["best_t"].tolist() == [[0]] and z["entropy"][0, 0] == 0.0


def test_match_stats_reference_matches_oracle():
    from oracle import gcp_model_oracle as O
    from oracle import tree_index_oracle as TI
    g = torch.Generator().manual_seed(3)
    L, T = 4, 12
    w = torch.rand(2, 15, T, generator=g)
    w = w / w.sum(1, keepdim=True)
    r = R.match_stats(w.numpy(), np.array([8, 5]), L)
    assert np.array_equal(r["frame2node"], TI.bf2df_perm(L)[O._bf_of_df(w, L).argmax(1).numpy()])
    assert np.allclose(r["entropy"], A.safe_entropy(w, -1).numpy(), atol=1e-5)
    assert np.allclose(r["p_n"], w.sum(2).clamp(0, 1).numpy(), atol=1e-6)


def test_distance_prune_reference_by_hand():
    dist = np.array([[3.0, -3.0, 0.0, 3.0], [-1.0, -1.0, -1.0, -1.0], [3.0, 3.0, 3.0, 3.0]])
    r = R.distance_prune(dist, 0.5, best_t=np.array([[4, 4, 1, 1, 2]] * 3))
    assert r["leave"].tolist() == [[1, 0, 1, 1, 0], [1, 1, 1, 1, 1], [1, 0, 0, 0, 0]]       # sigmoid(0) == 0.5 is not > 0.5: kept
    assert r["kept_idx"].tolist() == [[0, 2, 3, -1, -1], [0, 1, 2, 3, 4], [0, -1, -1, -1, -1]]
    assert r["count"].tolist() == [3, 5, 1]
    assert r["target"].tolist() == [[1, 0, 1, 0]] * 3
    close = torch.sigmoid(torch.tensor(dist)) > 0.5
    assert np.array_equal(r["leave"][:, 1:].astype(bool), ~close.numpy())


def test_averaging_references_match_oracle():
    g = torch.Generator().manual_seed(4)
    B, N, T, D = 2, 7, 5, 48
    w, dsum, x = torch.rand(B, N, T, generator=g), torch.rand(B, N, T, generator=g) * 50, torch.randn(B, N, D, generator=g)
    for ls in (-1.0, 0.3):
        val, ab = R.averaging_nll(dsum.numpy(), w.numpy(), ls, float(D))
        want = ((0.5 * dsum.double() * math.exp(-ls) ** 2 + D * (ls + 0.5 * math.log(2 * math.pi))) * w.double()).sum(1)
        assert np.max(np.abs(val - want.numpy())) < 1e-10 and np.all(ab >= np.abs(val))
    avg, ab = R.soft_average(w.numpy(), x.numpy())
    assert np.max(np.abs(avg - A.soft_estimates(w.double(), x.double()).numpy())) < 1e-12 and np.all(ab >= np.abs(avg))


def test_dtw_align_reference_slices_to_the_lengths():
    g = np.random.RandomState(5)
    C = g.randint(0, 3, size=(3, 6, 5)).astype(np.float32)
    res = R.dtw_align(C, n_len=[6, 1, 4], t_len=[5, 3, 1])
    for b, r in enumerate(res):
        d, D, path, inds = A.dtw_matches(C[b, :r["n"], :r["t"]])
        assert np.array_equal(r["acc"], D) and r["dist"] == d and np.array_equal(r["inds"][:r["t"]], inds)
        assert np.all(r["inds"][r["t"]:] == -1)
        assert r["path"][0][0] == 0 and r["path"][1][0] == 0 and r["path"][0][-1] == r["n"] - 1 and r["path"][1][-1] == r["t"] - 1
    assert res[1]["path"][0].tolist() == [0, 0, 0] and res[1]["path"][1].tolist() == [0, 1, 2]     # one row: all left moves
    assert res[2]["path"][1].tolist() == [0, 0, 0, 0] and res[2]["inds"].tolist() == [int(np.argmin(np.cumsum(C[2, :4, 0]))), -1, -1, -1, -1]
