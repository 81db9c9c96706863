"""No GPU: pins tests/loss_refs.py, the float64 references and rounding bounds tests/test_gpu_loss_kernels.py holds the loss, KL and
BatchNorm-statistics kernels to.
  1. the references equal oracle.gcp_model_oracle.losses / oracle.aux_models_oracle.l2_loss to 1e-12 relative on hand-built inputs / out
     dicts (non-adaptive branch, with and without the state, inverse and cost heads);
  2. a FLOAT32 restatement of each formula (torch on the CPU, torch's own summation order) stays inside the bound on every input set the
     GPU test uses: the bounds can be met without the code under test;
  3. the same restatement with ONE planted mistake falls outside the bound on at least one of those input sets, for every mistake of
     MISTAKES: the input sets can tell a wrong kernel from a right one."""
import math
from types import SimpleNamespace

import pytest
import torch

import loss_refs as R


def _rel(a, b):
    a, b = float(a), float(b)
    return abs(a - b) / max(abs(a), abs(b), 1e-300)


# ------------------------------------------------------------------------------------------------------------------------------
# 1. against the oracle
# ------------------------------------------------------------------------------------------------------------------------------
class _Float64Target:
    """the oracle casts the existence target with .float(), and F.binary_cross_entropy_with_logits returns the TARGET's dtype: a float32
    value of float64 logits.  The pin is to 1e-12, so the target handed over answers .float() with its float64 form."""
    def __init__(self, t):
        self.t = t

    def float(self):
        return self.t.double()


def _oracle_dicts(c, heads, pad_mask):
    """inputs / out / hp / sd for oracle.gcp_model_oracle.losses from a loss case, in float64 (gaussian decoder over 3 x 8 x 8 frames)
    -> (hp, sd, inputs, out, nll_bt)"""
    B, T, N = c["B"], c["T"], c["N"]
    g = torch.Generator().manual_seed(11)
    traj = torch.randn(B, T, 3, 8, 8, generator=g, dtype=torch.float64)
    mu = torch.randn(B, T, 3, 8, 8, generator=g, dtype=torch.float64)
    ls = torch.tensor(0.3, dtype=torch.float64)
    nll_bt = (0.5 * ((traj - mu) / torch.exp(ls)) ** 2 + ls + 0.5 * math.log(2 * math.pi)).sum((2, 3, 4))
    nz = R.KL_NZ
    q, p = c["q"].double(), c["p"].double()
    bf = dict(q_z_mu=q[..., :nz], q_z_log_sigma=q[..., nz:], p_z_mu=p[..., :nz], p_z_log_sigma=p[..., nz:])
    hp = SimpleNamespace(adaptive=False, decoder_distribution="gaussian", dense_img_rec_weight=c["w_rec"], free_nats=c["kl_fn"],
                         kl_weight=c["w_kl"], regress_length=True, length_pred_weight=c["w_len"], run_state_regressor=heads,
                         attach_inv_mdl=heads, action_rec_weight=c["w_action"], attach_cost_mdl=heads, run_cost_mdl=heads)
    inputs = dict(traj_seq=traj, pad_mask=pad_mask.double(), end_ind=c["end_ind"])
    out = dict(tree_bf=bf, matched_distr=mu, seq_len_logits=c["len_logits"].double(), leave_df=_Float64Target(c["leave"]), existence=c["existence"].double())
    if heads:
        ml = int(c["seq_len"].max())
        inputs["traj_seq_states"] = c["state_target"].double()
        out["regressed_state"] = c["regressed_state"].double()[:, :ml]
        out["actions"] = c["action_pred"].double()
        out["action_targets"] = c["action_seq"].double()[torch.arange(B), c["inv_t0"]]
        out["cost"], out["cost_target"] = c["cost_pred"].double(), c["cost_target"].double()
    return hp, {"decoder.log_sigma": ls}, inputs, out, nll_bt


@pytest.mark.parametrize("heads", [True, False])
@pytest.mark.parametrize("shape", ["T5-B1", "T130-B17", "T64-B4", "T65-B5", "T20-B5"])
def test_references_equal_the_oracle(shape, heads):
    """loss_terms and kl_gauss against oracle.gcp_model_oracle.losses: every term and the total to 1e-12 relative.  The oracle weighs the
    state regression with inputs.pad_mask; a case with a state_mask (the sequential model's convention) asks the oracle twice: once
    with the reconstruction weights, once with the state weights for the state term alone."""
    from oracle import gcp_model_oracle as O
    c = dict(R.loss_case(shape))
    hp, sd, inputs, out, nll_bt = _oracle_dicts(c, heads, c["pad_mask"])
    kl_b, kl_abs = R.kl_gauss(c["q"], c["p"], c["kl_fn"])
    assert bool((kl_abs >= kl_b.abs()).all())
    c.update(nll_bt=nll_bt, kl_b=kl_b)
    if not heads:
        c.update(regressed_state=None, state_target=None, action_pred=None, cost_pred=None)
    ref, mag = R.loss_terms(c)
    assert bool((mag >= ref.abs() * (1 - 1e-12)).all())
    res, total = O.losses(sd, hp, inputs, out)
    if heads and c["state_mask"] is not None:
        res_s, _ = O.losses(sd, hp, dict(inputs, pad_mask=c["state_mask"].double()), out)
        res["state_regression"] = res_s["state_regression"]
        total = sum(v * w for v, w in res.values() if w > 0) / float(torch.tensor(inputs["traj_seq"].shape[1:]).prod())
    assert float(torch.tensor(inputs["traj_seq"].shape[1:]).prod()) == c["total_div"]
    names = dict(dense_img_rec=0, kl=1, len_pred=2, existence_predictor=3, state_regression=4, action_reconst=7, cost_estimation=8)
    assert set(res) == set(names) if heads else set(res) == {"dense_img_rec", "kl", "len_pred", "existence_predictor"}
    for k, (v, w) in res.items():
        assert _rel(ref[names[k]], v) <= 1e-12, (k, float(ref[names[k]]), float(v))
        assert float(ref[names[k]]) != 0.0
    for k, s in names.items():
        if k not in res:
            assert float(ref[s]) == 0.0, k
    assert _rel(ref[5], total) <= 1e-12
    assert _rel(ref[6], res["dense_img_rec"][0] + res["kl"][0]) <= 1e-12


def test_squared_error_terms_equal_l2_loss():
    from oracle import aux_models_oracle as AX
    c = R.loss_case("T65-B5")
    ref, _ = R.loss_terms(c)
    ar = torch.arange(c["B"])
    assert _rel(ref[7], AX.l2_loss(c["action_pred"].double(), c["action_seq"].double()[ar, c["inv_t0"]])) <= 1e-12
    assert _rel(ref[8], AX.l2_loss(c["cost_pred"].double(), c["cost_target"].double())) <= 1e-12
    ml = int(c["seq_len"].max())
    want = AX.l2_loss(c["regressed_state"].double()[:, :ml], c["state_target"].double()[:, :ml], c["state_mask"].double()[:, :ml, None])
    assert _rel(ref[4], want) <= 1e-12


def test_kl_reference_with_node_weights_is_the_weighted_sum_of_the_oracle_elements():
    """the oracle has no node weights: per node, its expression; the reference is the weighted sum of those"""
    c = R.kl_case("wide-nz4-N1100-B1-fn0.1")
    nz = c["nz"]
    q, p = c["q"].double(), c["p"].double()
    mq, lq, mp, lp = q[..., :nz], q[..., nz:], p[..., :nz], p[..., nz:]
    kl = torch.clamp(lp - lq + (torch.exp(2 * lq) + (mq - mp) ** 2) / (2 * torch.exp(2 * lp)) - 0.5, min=c["fn"])       # gcp_model_oracle.py:561-562
    want = (kl.sum(-1) * c["w"].double()).sum(1)
    got, _ = R.kl_gauss(c["q"], c["p"], c["fn"], c["w"])
    assert _rel(got[0], want[0]) <= 1e-12


# ------------------------------------------------------------------------------------------------------------------------------
# 2. / 3. float32 restatements, right and with one planted mistake
# ------------------------------------------------------------------------------------------------------------------------------
def kl_f32(c, bug=None):
    nz, B, N = c["nz"], c["B"], c["N"]
    q, p = c["q"], c["p"]
    mq, lq, mp, lp = q[..., :nz], q[..., nz:], p[..., :nz], p[..., nz:]
    kl = lp - lq + (torch.exp(2 * lq) + (mq - mp) ** 2) / (2 * torch.exp(2 * lp))
    if bug != "half_dropped":
        kl = kl - 0.5
    if bug != "clamp_dropped":
        kl = torch.clamp(kl, min=c["fn"])
    if c["w"] is None:
        w = torch.ones(B, N)
    else:
        flat = torch.cat([c["w_buf"].flatten(), torch.full((2,), R.SENT)])
        idx = c["w_off"] + (1 if bug == "weight_shifted" else 0) + torch.arange(B)[:, None] * c["w_bs"] + torch.arange(N)[None]
        w = flat[idx]
    assert kl.dtype == torch.float32 and w.dtype == torch.float32
    return (kl.sum(-1) * w).sum(1)


def loss_f32(c, bug=None):
    B, T, N = c["B"], c["T"], c["N"]
    ar = torch.arange(B)
    out = torch.zeros(9)
    out[0] = (c["nll_bt"] * c["pad_mask"]).sum() / B
    if c["kl_b"] is not None:
        out[1] = c["kl_b"].sum() / B
    if c["len_logits"] is not None:
        lg = c["len_logits"]
        end = (c["end_ind"] + 1) % T if bug == "end_ind_off_by_one" else c["end_ind"]
        m = lg.max(1).values
        out[2] = (m + torch.log(torch.exp(lg - m[:, None]).sum(1)) - lg[ar, end]).sum() / B
    if c["existence"] is not None:
        x, y = c["existence"], c["leave"].float()
        if bug == "bce_target_inverted":
            y = 1 - y
        out[3] = (x.clamp_min(0) - x * y + torch.log1p(torch.exp(-x.abs()))).sum() / (B * N)
    if c["regressed_state"] is not None and c["state_target"] is not None:
        ml = int(c["seq_len"].max())
        mask = c["state_mask"] if c["state_mask"] is not None and bug != "pad_mask_for_state_mask" else c["pad_mask"]
        e = (c["regressed_state"][:, :ml] - c["state_target"][:, :ml]) ** 2 * mask[:, :ml, None]
        out[4] = e.sum() / (B * (T if bug == "divisor_B_T" else ml) * c["state_dim"])
    if c["action_pred"] is not None:
        t0 = (c["inv_t0"] + 1) % (T - 1) if bug == "inv_t0_off_by_one" else c["inv_t0"]
        out[7] = ((c["action_pred"] - c["action_seq"][ar, t0]) ** 2).sum() / (B * c["n_actions"])
    if c["cost_pred"] is not None:
        out[8] = ((c["cost_pred"] - c["cost_target"]) ** 2).sum() / B
    w = {k: c[k] for k in R.WEIGHTS}
    if c["w_kl_dev"] is not None and bug != "w_kl_although_w_kl_dev":
        w["w_kl"] = c["w_kl_dev"]
    total = torch.zeros(())
    for k, s in R.W_SLOT.items():
        wk = torch.tensor(w[k])
        if w[k] > 0 or bug == "positive_weight_test_dropped":
            total = total + wk * out[s]
        elif w[k] == 0 and bug == "weight_0_term_added":
            total = total + out[s]
    out[5] = total / torch.tensor(c["total_div"])
    out[6] = out[0] + out[1]
    assert out.dtype == torch.float32
    return out


BN_VARIANTS = [(0.1, True), (1.0, True), (0.0, False)]       # momentum, running buffers given


def bn_f32(c, momentum, running, bug=None):
    """the sums in float64 as the kernel keeps them (f32 sums of a channel with |mean| = 1e3 std have no correct digit of the variance
    left), the last block's casts in f32"""
    n, pitch, C, count = c["n_partial"], c["pitch"], c["C"], c["count"]
    rep = pitch // C
    k, ch = torch.arange(rep + (1 if bug == "padding_column_read" else 0))[:, None], torch.arange(C)[None]
    cols = ch * rep + k if bug == "column_c_rep_plus_k" else k * C + ch
    ok = cols < pitch                                                                  # (the planted reads stay inside the row)
    tab = c["partial"].double()[:, :, cols.clamp(max=pitch - 1)] * ok
    s1, s2 = tab[:, 0].sum((0, 1)), tab[:, 1].sum((0, 1))
    mean = s1 / count
    var = (s2 / count - mean ** 2).clamp_min(0)
    rstd = (1 / torch.sqrt(var + R.BN_EPS)).float()
    sc = c["gamma"] * rstd
    got = dict(scale=sc, shift=c["beta"] - mean.float() * sc, mean=mean.float(), rstd=rstd)
    if running:
        m = torch.tensor(momentum)
        unb = var * count / (count - 1) if count > 1 and bug != "biased_running_variance" else var
        got["running_mean"] = (1 - m) * c["running_mean"] + m * mean.float()
        got["running_var"] = (1 - m) * c["running_var"] + m * unb.float()
    assert all(v.dtype == torch.float32 for v in got.values())
    return got


def _kl_outside(c, bug):
    ref, _ = R.kl_gauss(c["q"], c["p"], c["fn"], c["w"])
    tol = R.kl_tol(c["q"], c["p"], c["fn"], c["w"])
    return float(((kl_f32(c, bug).double() - ref).abs() / tol.clamp_min(1e-300)).max())


def _loss_outside(c, bug):
    ref, _ = R.loss_terms(c)
    tol = torch.maximum(R.loss_tol(c, 256), R.loss_tol(c, 1024)) if bug else torch.minimum(R.loss_tol(c, 256), R.loss_tol(c, 1024))
    err = (loss_f32(c, bug).double() - ref).abs()
    return float(torch.where(err == 0, torch.zeros_like(err), err / tol.clamp_min(1e-300)).max())


def _bn_outside(c, bug):
    worst = 0.0
    for momentum, running in BN_VARIANTS:
        kw = dict(momentum=R.f32(momentum), running_mean=c["running_mean"], running_var=c["running_var"]) if running else {}
        ref, tol = R.bn_finalize(c["partial"], c["n_partial"], c["pitch"], c["C"], c["count"], c["gamma"], c["beta"], R.BN_EPS, **kw)
        got = bn_f32(c, momentum, running, bug)
        for k in ref:
            err = (got[k].double() - ref[k]).abs()
            worst = max(worst, float(torch.where(err == 0, torch.zeros_like(err), err / tol[k].clamp_min(1e-300)).max()))
    return worst


@pytest.mark.parametrize("name", sorted(R.KL_CASES))
def test_f32_kl_stays_inside_the_bound(name):
    c = R.kl_case(name)
    w = _kl_outside(c, None)
    print(f"[ratio] f32 restatement, kl {name}: {w:.3g}")
    assert w <= 1.0
    low, high = R.kl_clamp_shares(c)
    assert low >= 0.15 and high >= 0.15, (low, high)


@pytest.mark.parametrize("name", R.LOSS_CASES)
def test_f32_loss_terms_stay_inside_the_bound(name):
    w = _loss_outside(R.loss_case(name), None)
    print(f"[ratio] f32 restatement, loss {name}: {w:.3g}")
    assert w <= 1.0


@pytest.mark.parametrize("shape", R.BN_CASES, ids=lambda s: "%dx%dx%d" % s)
def test_f32_bn_finalize_stays_inside_the_bound(shape):
    w = _bn_outside(R.bn_case(*shape), None)
    print(f"[ratio] f32 restatement, bn_finalize {shape}: {w:.3g}")
    assert w <= 1.0


MISTAKES = {
    "divisor_B_T": "loss", "pad_mask_for_state_mask": "loss", "end_ind_off_by_one": "loss", "inv_t0_off_by_one": "loss",
    "weight_shifted": "kl", "clamp_dropped": "kl", "half_dropped": "kl",
    "positive_weight_test_dropped": "loss", "weight_0_term_added": "loss", "w_kl_although_w_kl_dev": "loss", "bce_target_inverted": "loss",
    "column_c_rep_plus_k": "bn", "padding_column_read": "bn", "biased_running_variance": "bn",
}


@pytest.mark.parametrize("bug", sorted(MISTAKES))
def test_every_planted_mistake_falls_outside_the_bound_on_some_case(bug):
    """(a term with weight 0 added to the total: planted twice, as the `w > 0` test dropped — a weight 0 then adds 0 x term, a negative
    weight subtracts — and as a weight-0 term entering at weight 1)"""
    kind = MISTAKES[bug]
    if kind == "kl":
        ratios = {n: _kl_outside(R.kl_case(n), bug) for n in sorted(R.KL_CASES)}
    elif kind == "loss":
        ratios = {n: _loss_outside(R.loss_case(n), bug) for n in R.LOSS_CASES}
    else:
        ratios = {"%dx%dx%d" % s: _bn_outside(R.bn_case(*s), bug) for s in R.BN_CASES}
    caught = {n: r for n, r in ratios.items() if r > 1.0}
    print(f"{bug}: outside the bound on {len(caught)} of {len(ratios)} cases, least clear {min(caught.values(), default=0):.3g} x the bound")
    assert caught, f"no case tells {bug} from the right formula: a case is missing"
    # a caught mistake is caught clearly: it is no rounding effect
    assert max(caught.values()) > 100.0
