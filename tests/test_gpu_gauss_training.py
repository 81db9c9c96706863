"""-m gpu: training with decoder_distribution = "gaussian" (the reference's own default, hyperparameters.py:69: a learned
decoder.log_sigma), tree model and flat model, against torch autograd over the oracles.  The tolerances are the project's, as
tests/test_gpu_training.py and tests/test_gpu_sequential.py state them: a parameter gradient within 1e-3 of that gradient's max-abs
(+ 5e-7); the total loss within 2e-5 (tree) / 1e-4 (flat) relative; after optimizer steps the parameters within 2e-3 * lr per step.

decoder.log_sigma is set to -0.7 everywhere: at its initial 0 the factor exp(-2 log_sigma) is 1 and a gradient without it would pass."""
import pytest
import torch

from helpers import make_inputs

pytestmark = pytest.mark.gpu
LOG_SIGMA = -0.7
HEAD = ("decoder.log_sigma", "decoder.gen_head.conv.weight", "decoder.gen_head.conv.bias")


def _tree(graph, name="c1", exact_f32=False, **over):
    import video_gcp_amd as V
    from video_gcp_amd.model import GCPTreeModel
    from video_gcp_amd.training import GCPTrainStep
    hp = V.config(name, decoder_distribution="gaussian", **over)
    sd = V.init_params(hp, seed=1, randomize_affine=True)
    sd["decoder.log_sigma"] = torch.full_like(sd["decoder.log_sigma"], LOG_SIGMA)
    model = GCPTreeModel(hp, params=sd, device="cuda")
    if exact_f32:
        model.split_f16 = False
    model.use_graph = graph
    return hp, sd, model, GCPTrainStep(model, lr=1e-3)


def _flat(name="c1", **over):
    import video_gcp_amd as V
    from video_gcp_amd.sequential import GCPSequentialModel
    from video_gcp_amd.training_sequential import SequentialTrainStep
    hp = V.config(name, decoder_distribution="gaussian", nz_mid_lstm=128, lstm_init="zero", **over)
    sd = V.init_params_sequential(hp, seed=1, randomize_affine=True)
    sd["decoder.log_sigma"] = torch.full_like(sd["decoder.log_sigma"], LOG_SIGMA)
    model = GCPSequentialModel(hp, params=sd, device="cuda")
    return hp, sd, model, SequentialTrainStep(model, lr=1e-3)


def _compare_grads(gref, got, rtol=1e-3, atol=5e-7):
    bad = []
    for k, g in gref.items():
        err, scale = float((got[k].cpu() - g).abs().max()), float(g.abs().max())
        if err > rtol * scale + atol:
            bad.append((k, err, scale))
    assert not bad, bad[:10]
    for k in HEAD:                        # the head and log_sigma receive a gradient (the table of the issue: d log_sigma of order 1)
        assert float(gref[k].abs().max()) > 1e-6 and float(got[k].abs().max()) > 0, k


@pytest.mark.parametrize("mode", ["eager", "graph", "exact_f32"])
def test_tree_gradients_match_autograd_c1(mode):
    """Tree model, c1, 17 padded frames (variant B): every parameter gradient — decoder.log_sigma, the head's weight and bias among
    them — of the explicit backward behind gcpx_gauss_nll_bwd against autograd over the oracle; eager, with the forward as a captured
    graph (second call replays it), and on the exact-f32 build (model.split_f16 = False)."""
    from oracle import gcp_model_oracle as O
    hp, sd, model, tr = _tree(mode == "graph", exact_f32=(mode == "exact_f32"))
    inputs, noise, _ = make_inputs(hp, seed=7, variant="B")
    dev_in = {k: v.cuda() for k, v in inputs.items()}
    for _ in range(2):
        out = tr.backward(dev_in, noise.cuda())
    torch.cuda.synchronize()
    gref, res, total, _ = O.gradients(sd, hp, inputs, noise)
    print(f"[gauss] tree {mode}: total {float(total):.4f} d log_sigma {float(gref['decoder.log_sigma']):.4f} "
          f"got {float(tr.named_grads()['decoder.log_sigma']):.4f}")
    assert abs(float(out.raw["losses"][5]) - float(total)) <= 2e-5 * abs(float(total))
    _compare_grads(gref, tr.named_grads())


def _flat_oracle_f64(sd, hp, inputs, noise):
    """autograd over the flat oracle, run in float64 (its recurrent state starts from torch.zeros: the default dtype is switched for
    the call) and returned as float32"""
    from oracle import gcp_sequential_oracle as S
    d = lambda t: t.double() if torch.is_tensor(t) and t.is_floating_point() else t
    torch.set_default_dtype(torch.float64)
    try:
        g, res, total, _ = S.gradients({k: d(v) for k, v in sd.items()}, hp, {k: d(v) for k, v in inputs.items()}, d(noise))
    finally:
        torch.set_default_dtype(torch.float32)
    return {k: v.float() for k, v in g.items()}, res, float(total)


@pytest.mark.parametrize("case", ["B", "A", "vmpc_s"])
def test_flat_gradients_match_autograd(case):
    """Flat model: c1 (nz_mid_lstm 128, lstm_init zero) with padded (B) and full-length (A) sequences, and the deterministic,
    action-conditioned, non-goal-conditioned vmpc_s predictor, each with the gaussian head.  Row (b, 0) of the likelihood compares I_0
    with itself and weighs 0.
    The oracle runs in float64, for the reason test_gradients_full_length_sequences_c1 gives for its float64 oracle: the bound is not
    widened where the float32 reference is the noisy side.  decoder.net.input.conv.bias sits in front of a BatchNorm, its gradient is
    exactly 0 (the HIP backward reports 0); float32 autograd over 19 recurrent steps reports 6.2e-7 to 6.7e-7 of rounding noise there
    at this log_sigma (exp(1.4) = 4 times the gradients of log_sigma = 0), above the 5e-7 the bound grants such noise; in float64 it
    reports 1.5e-15.  Same bound, same oracle, same inputs and seed."""
    hp, sd, model, tr = _flat("vmpc_s") if case == "vmpc_s" else _flat()
    inputs, noise, _ = make_inputs(hp, seed=7, variant="B" if case == "vmpc_s" else case)
    noise = noise[:, :hp.max_seq_len - 1].contiguous() if hp.nz_vae else None
    dev_in = {k: v.cuda() for k, v in inputs.items()}
    for _ in range(2):
        out = tr.backward(dev_in, noise.cuda() if noise is not None else None)
    torch.cuda.synchronize()
    gref, res, total = _flat_oracle_f64(sd, hp, inputs, noise)
    print(f"[gauss] flat {case}: total {float(total):.4f} d log_sigma {float(gref['decoder.log_sigma']):.4f} "
          f"got {float(tr.named_grads()['decoder.log_sigma']):.4f}")
    assert abs(float(out.raw["losses"][5]) - float(total)) <= 1e-4 * abs(float(total))
    _compare_grads(gref, tr.named_grads())


def test_tree_two_radam_steps():
    """two optimisation steps of the tree model against two steps of the oracle loop: losses, parameters within 2e-3 * lr per step,
    and log_sigma has moved"""
    from oracle import gcp_model_oracle as O
    from oracle.radam_oracle import RAdamOracle
    hp, sd, model, tr = _tree(True)
    ref_sd = {k: v.clone() for k, v in sd.items()}
    opt = RAdamOracle(lr=1e-3)
    for step in range(2):
        inputs, noise, _ = make_inputs(hp, seed=20 + step, variant="B")
        out = tr.step({k: v.cuda() for k, v in inputs.items()}, noise.cuda())
        torch.cuda.synchronize()
        gref, res, total, _ = O.gradients(ref_sd, hp, inputs, noise)
        assert abs(float(out.raw["losses"][5]) - float(total)) <= 2e-5 * abs(float(total)), step
        opt.step(ref_sd, gref)
        worst = max(float((model.sd[k].cpu() - ref_sd[k]).abs().max()) for k in gref)
        assert worst <= 2e-3 * 1e-3 * (step + 1) + 1e-7, (step, worst)
    assert abs(float(model.sd["decoder.log_sigma"]) - LOG_SIGMA) > 1e-4


@pytest.mark.parametrize("which", ["tree", "flat"])
def test_two_trainers_keep_identical_parameters(which):
    """two trainers fed the same minibatches hold bit-identical parameters and moments after two steps: the likelihood gradient, its
    column sums and the log_sigma reduction have a fixed order"""
    if which == "tree":
        (hp, _, m1, tr1), (_, _, m2, tr2) = _tree(True), _tree(True)
    else:
        (hp, _, m1, tr1), (_, _, m2, tr2) = _flat(), _flat()
    for step in range(2):
        inputs, noise, _ = make_inputs(hp, seed=40 + step, variant="B")
        noise = (noise if which == "tree" else noise[:, :hp.max_seq_len - 1].contiguous()).cuda()
        dev_in = {k: v.cuda() for k, v in inputs.items()}
        tr1.step(dev_in, noise)
        tr2.step(dev_in, noise)
    torch.cuda.synchronize()
    assert torch.equal(m1.theta, m2.theta) and torch.equal(tr1.exp_avg, tr2.exp_avg) and torch.equal(tr1.exp_avg_sq, tr2.exp_avg_sq)
    assert float(m1.sd["decoder.log_sigma"]) != LOG_SIGMA


def test_adaptive_gaussian_training_is_refused():
    """the adaptive model's backward takes the image gradient through the mixture mean: with the gaussian head the trainer says so"""
    import video_gcp_amd as V
    from video_gcp_amd.model import GCPTreeModel
    from video_gcp_amd.training import GCPTrainStep
    hp = V.config("c5s", decoder_distribution="gaussian")
    model = GCPTreeModel(hp, params=V.init_params(hp, seed=1), device="cuda")
    with pytest.raises(ValueError, match="gaussian"):
        GCPTrainStep(model, lr=1e-3)
