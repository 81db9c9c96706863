"""tests/attn_refs.py without a GPU: its float64 restatements against float64 autograd of oracle.adaptive_oracle.multihead_attention /
attention and F.layer_norm, and its rounding bounds against float32 torch evaluation of the same formulas (which must stay inside
them, with room: a bound that f32 arithmetic itself reaches would reject a right kernel)."""
import pytest
import torch
import torch.nn.functional as F

import attn_refs as R


def _f64(case):
    return {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in case.items()}


def _identity_sd(dk, nz, temp):
    sd = {}
    for nm, d in (("q_proj", dk), ("k_proj", dk), ("v_proj", nz), ("out_proj", nz)):
        sd[f"a.{nm}.weight"], sd[f"a.{nm}.bias"] = torch.eye(d, dtype=torch.float64), torch.zeros(d, dtype=torch.float64)
    sd["a.temperature"] = temp
    return sd


@pytest.mark.parametrize("heads", R.HEAD_CASES)
@pytest.mark.parametrize("T,rpb", [(37, 1), (37, 5), (300, 5)])
def test_mha_and_its_gradients_match_autograd_of_the_oracle(heads, T, rpb):
    import video_gcp_amd as V
    from oracle import adaptive_oracle as A
    c = _f64(R.mha_case(T, rpb))
    hp = V.config("c5s", n_attention_heads=heads, nz_attn_key=R.DK, nz_enc=R.NZ)
    q, k, v = (c[n].clone().requires_grad_(True) for n in ("q", "k", "v"))
    temp = torch.tensor([c["temp"]], dtype=torch.float64, requires_grad=True)
    rep = lambda t: t.repeat_interleave(rpb, 0)
    M = q.shape[0]
    out, att = A.multihead_attention(_identity_sd(R.DK, R.NZ, temp), "a", hp, q, rep(k), rep(v), torch.zeros(M, dtype=torch.long),
                                     rep(c["end"]))
    (out * c["dout"]).sum().backward()
    got = R.mha_grads(c["q"], c["k"], c["v"], c["end"], c["temp"], heads, rpb, c["dout"])
    close = lambda a, b, name: torch.testing.assert_close(a, b, rtol=1e-11, atol=1e-13, msg=lambda m: f"{name}: {m}")
    close(got["out"], out.detach(), "out")
    close(got["a"].mean(1), att.detach(), "head-averaged weights")
    close(got["dq"], q.grad, "dq")
    close(got["dK"], k.grad, "dK")
    close(got["dV"], v.grad, "dV")
    close(got["dtemp_row"].sum(), temp.grad[0], "dtemp")
    # the one-frame window: one weight of 1, no gradient to scores or query; keys / values past end_ind get exact zeros
    rows = slice(rpb, 2 * rpb)
    assert bool((got["dS"][rows] == 0).all()) and bool((got["dq"][rows] == 0).all())
    assert bool((got["dK"][1, 1:] == 0).all()) and bool((got["dV"][1, 1:] == 0).all()) and bool((got["dV"][2, 21:] == 0).all())


@pytest.mark.parametrize("heads", R.HEAD_CASES)
@pytest.mark.parametrize("T,rpb", [(37, 1), (37, 5), (300, 5)])
def test_f32_torch_attention_gradients_stay_inside_the_bounds(heads, T, rpb):
    c32 = R.mha_case(T, rpb)
    c = _f64(c32)
    args = lambda d: (d["q"], d["k"], d["v"], d["end"], d["temp"], heads, rpb, d["dout"])
    ref, got, bnd = R.mha_grads(*args(c)), R.mha_grads(*args(c32)), R.mha_bounds(*args(c))
    for name in ("dS", "dq", "dK", "dV", "dtemp_row"):
        assert got[name].dtype == torch.float32
        ratio = ((got[name].double() - ref[name]).abs() / bnd[name]).max()
        assert float(ratio) < 0.5, (name, float(ratio))
    if heads > 1:
        # ... and the bounds bite: the one-head kernels' reading of the saved weights (the mean over heads taken for each head's
        # softmax) is far outside them in every output
        abar = ref["a"].mean(1, keepdim=True).expand_as(ref["a"])
        doh, vh = R._split(c["dout"], heads), R._split(c["v"], heads).repeat_interleave(rpb, 0)
        dA = (doh[:, None] * vh).sum(-1).transpose(1, 2)
        dS_bar = abar * (dA - (abar * dA).sum(-1, keepdim=True))
        dV_bar = (abar.transpose(1, 2)[..., None] * doh[:, None]).reshape(R.B_SEQ, rpb, T, -1).sum(1)
        assert float(((dS_bar - ref["dS"]).abs() / bnd["dS"]).max()) > 100
        assert float(((dV_bar - ref["dV"]).abs() / bnd["dV"]).max()) > 100


@pytest.mark.parametrize("W", [32, 128])
@pytest.mark.parametrize("with_add", [False, True])
def test_layernorm_and_its_gradient_match_autograd_of_F_layer_norm(W, with_add):
    c = _f64(R.layernorm_case(W, with_add))
    x = c["x"].clone().requires_grad_(True)
    add = c["add"].clone().requires_grad_(True) if with_add else None
    s = x + add if with_add else x
    want = F.layer_norm(s, s.shape[1:])
    (want * c["dy"]).sum().backward()
    y, rstd = R.layernorm(c["x"], c["add"])
    dx = R.layernorm_bwd(c["dy"], y, rstd)
    torch.testing.assert_close(y, want.detach(), rtol=1e-11, atol=1e-12)
    torch.testing.assert_close(dx, x.grad, rtol=1e-9, atol=1e-10)
    if with_add:
        torch.testing.assert_close(dx, add.grad, rtol=1e-9, atol=1e-10)
    assert float(y[3].abs().max()) < 1e-10 and abs(float(rstd[3]) - 1e-5 ** -0.5) < 1e-9          # the constant row


@pytest.mark.parametrize("W", [32, 128])
@pytest.mark.parametrize("with_add", [False, True])
def test_f32_torch_layernorm_stays_inside_the_bounds(W, with_add):
    c32 = R.layernorm_case(W, with_add)
    c = _f64(c32)
    y64, rstd64 = R.layernorm(c["x"], c["add"])
    by, brs = R.layernorm_bound(c["x"], c["add"])
    for y32, rs32 in (R.layernorm(c32["x"], c32["add"]),
                      (F.layer_norm(c32["x"] + c32["add"] if with_add else c32["x"], (W,)), None)):
        assert float(((y32.double() - y64).abs() / by).max()) < 0.5
        if rs32 is not None:
            assert float(((rs32.double() - rstd64).abs() / brs).max()) < 0.5
    rows = [r for r in range(c["x"].shape[0]) if r != 3]
    assert float(by[rows].max()) < 1e-4                      # unit-scale outputs: a bound of 1e-4 still sees a wrong mean or variance
    # backward on the f32 y and rstd a kernel is handed
    y32, rs32 = R.layernorm(c32["x"], c32["add"])
    ref = R.layernorm_bwd(c["dy"], y32.double(), rs32.double())
    bnd = R.layernorm_bwd_bound(c["dy"], y32.double(), rs32.double())
    got = R.layernorm_bwd(c32["dy"], y32, rs32)
    assert float(((got.double() - ref).abs() / bnd).max()) < 0.5
    assert float((bnd / ref.abs().max(1, keepdim=True).values).max()) < 1e-4


@pytest.mark.parametrize("heads,layers", [(1, 1), (2, 1), (1, 2), (2, 3)])
def test_layer_loop_restated_with_these_functions_is_the_oracles_attention(heads, layers):
    """Attention.forward (attentive_inference.py:80-85) put together from mha and layernorm above, the projections and Predictors
    taken from the oracle: the same e_tilde and weights as oracle.adaptive_oracle.attention, and its last layer's predictor_layers
    entry has no part in either."""
    import video_gcp_amd as V
    from oracle import adaptive_oracle as A
    from oracle import gcp_model_oracle as O
    hp = V.config("c5s", n_attention_heads=heads, n_attention_layers=layers)
    sd = {k: v.double() for k, v in V.init_params(hp, seed=3, randomize_affine=True).items()}
    p = "tree_module.tree_modules.1.inference.attention"
    for i in range(layers):
        sd[f"{p}.attention_layers.{i}.temperature"].fill_(0.5 + 0.3 * i)
    g = torch.Generator().manual_seed(5)
    B, T, mult, nz, dk = 2, hp.max_seq_len, 3, hp.nz_enc, hp.nz_attn_key
    values, keys = torch.randn(B, T, nz, generator=g).double(), torch.randn(B, T, dk, generator=g).double()
    el, er = torch.randn(B * mult, nz, generator=g).double(), torch.randn(B * mult, nz, generator=g).double()
    end = torch.tensor([T - 1, 4])
    want, want_att = A.attention(sd, p, hp, O.predictor, values, keys, (el, er), torch.zeros(B, dtype=torch.long), end)
    lin = lambda x, n: F.linear(x, sd[f"{n}.weight"], sd[f"{n}.bias"])
    query = O.predictor(sd, f"{p}.query_net", hp, el, er)
    for i in range(layers):
        m = f"{p}.attention_layers.{i}"
        o, a, _ = R.mha(lin(query, f"{m}.q_proj"), lin(keys, f"{m}.k_proj"), lin(values, f"{m}.v_proj"), end,
                        float(sd[f"{m}.temperature"]), heads, mult)
        raw = lin(o, f"{m}.out_proj")
        if i < layers - 1:
            x, _ = R.layernorm(raw)
            query, _ = R.layernorm(O.predictor(sd, f"{p}.predictor_layers.{i}", hp, x), query)
    torch.testing.assert_close(lin(raw, f"{p}.out"), want, rtol=1e-10, atol=1e-12)
    torch.testing.assert_close(a.mean(1), want_att, rtol=1e-10, atol=1e-12)
