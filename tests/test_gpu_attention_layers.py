"""-m gpu: the attentive posterior with several heads and several attention layers (hyperparameters.py:24-25; Attention.forward,
attentive_inference.py:80-86) through the forward and backward plans at c5s (B = 2, T = 12, 32 x 32, four tree levels), against the CPU
oracle and torch autograd over it -- the tests of tests/test_gpu_adaptive.py for (heads, layers) = (1, 1), with their tolerances, at
(2, 1), (1, 2) and (2, 2).  Tied tree levels (untied_layers = False) share one attention module: their forward is checked at (2, 2); the
attentive training step is built for untied levels only, at every (heads, layers), as it was at (1, 1)."""
import functools

import pytest
import torch

from helpers import make_inputs, assert_close

pytestmark = pytest.mark.gpu

LAT_ATOL, LAT_RTOL = 5e-5, 1e-4         # tests/test_gpu_adaptive.py
PIX_ATOL = 2e-5
WIDE = [(2, 1), (1, 2), (2, 2)]
ATT = "inference.attention"


def _hp(heads, layers, untied=True):
    import video_gcp_amd as V
    return V.config("c5s", n_attention_heads=heads, n_attention_layers=layers, untied_layers=untied)


@functools.lru_cache(maxsize=None)
def _params(heads, layers, untied=True):
    """parameters as tests/test_gpu_adaptive.py::_build sets them; every attention layer gets a temperature of its own"""
    import video_gcp_amd as V
    hp = _hp(heads, layers, untied)
    sd = V.init_params(hp, seed=1, randomize_affine=True)
    sd["decoder.log_sigma"].fill_(0.2)
    sd["tree_module.tree_modules.0.binding.temp"].fill_(0.3)
    for k in sd:
        if k.endswith(".temperature"):
            sd[k].fill_(0.7 + 0.2 * int(k.split(".")[-2]))
    return sd


def _model(heads, layers, untied=True):
    from video_gcp_amd.model import GCPTreeModel
    hp = _hp(heads, layers, untied)
    return hp, GCPTreeModel(hp, params={k: v.clone() for k, v in _params(heads, layers, untied).items()}, device="cuda")


@functools.lru_cache(maxsize=None)
def _oracle(heads, layers, untied, seed, with_grads):
    """the oracle's forward (and autograd gradients) of one configuration, computed once on the CPU"""
    from oracle import gcp_model_oracle as O
    hp, sd = _hp(heads, layers, untied), _params(heads, layers, untied)
    inputs, noise, _ = make_inputs(hp, seed=seed, variant="B")
    if with_grads:
        gref, _, total, _ = O.gradients(sd, hp, inputs, noise)
        return inputs, noise, gref, float(total.detach())
    return inputs, noise, O.forward(sd, hp, inputs, noise=noise, training_bn=True), None


@pytest.mark.parametrize("heads,layers,untied", [(h, l, True) for h, l in WIDE] + [(2, 2, False)])
def test_forward_matches_the_oracle(heads, layers, untied):
    hp, model = _model(heads, layers, untied)
    model.train(True)
    inputs, noise, ref, _ = _oracle(heads, layers, untied, 11, False)
    dev_in = {k: v.cuda() for k, v in inputs.items()}
    for _ in range(2):
        out = model(dev_in, "train", noise=noise.cuda())
    torch.cuda.synchronize()
    bf, tree = ref["tree_bf"], out.tree
    assert_close(tree.bf.e_tilde, bf["e_tilde"], LAT_ATOL, LAT_RTOL, "e_tilde")
    assert_close(tree.bf.gamma, bf["gamma"], 1e-6, 1e-4, "gamma (last layer, mean over heads)")
    for k_dev, k_ref in (("z", "z"), ("q_z_mu", "q_z_mu"), ("q_z_log_sigma", "q_z_log_sigma"), ("p_z_mu", "p_z_mu")):
        assert_close(getattr(tree.bf, k_dev), bf[k_ref], LAT_ATOL, LAT_RTOL, k_dev)
    assert_close(tree.bf.images, bf["images"], PIX_ATOL, 0, "images")


def _compare_grads(gref, got, rtol=1e-3, atol=5e-7):          # tests/test_gpu_adaptive.py
    bad = []
    for k, g in gref.items():
        h = got[k].cpu()
        err, scale = float((h - g).abs().max()), float(g.abs().max())
        if err > rtol * scale + atol:
            bad.append((k, err, scale))
    assert not bad, bad[:12]


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("heads,layers", WIDE)
def test_gradients_match_autograd(heads, layers, graph):
    """every parameter's gradient against torch autograd over the oracle, at the tolerance of
    tests/test_gpu_adaptive.py::test_adaptive_gradients_match_autograd_c5s: 1e-3 of each gradient's max-abs (+5e-7).  The last layer's
    predictor_layers entry is computed and dropped by the reference: its gradient is exactly zero, here and in autograd."""
    from video_gcp_amd.training import GCPTrainStep
    hp, model = _model(heads, layers)
    model.use_graph = graph
    tr = GCPTrainStep(model, lr=1e-3)
    inputs, noise, gref, total = _oracle(heads, layers, True, 31, True)
    dev_in = {k: v.cuda() for k, v in inputs.items()}
    for _ in range(2):
        out = tr.backward(dev_in, noise.cuda())
    torch.cuda.synchronize()
    assert abs(float(out.raw["losses"][5]) - total) <= 1e-4 * abs(total)
    got = tr.named_grads()
    _compare_grads(gref, got)
    last = f"{ATT}.predictor_layers.{layers - 1}."
    unused = [k for k in got if last in k]
    assert len(unused) == hp.hierarchy_levels * 12
    for k in unused:
        assert float(got[k].abs().max()) == 0.0 and float(gref[k].abs().max()) == 0.0, k
    # ... and what the widened attention adds does get a gradient
    for l in range(hp.hierarchy_levels):
        a = f"tree_module.tree_modules.{l}.{ATT}"
        for i in range(layers):
            for nm in ("q_proj.weight", "k_proj.weight", "v_proj.weight", "out_proj.weight", "temperature"):
                assert float(got[f"{a}.attention_layers.{i}.{nm}"].abs().max()) > 0, (l, i, nm)
        for i in range(layers - 1):
            assert float(got[f"{a}.predictor_layers.{i}.input.linear.weight"].abs().max()) > 0, (l, i)


def _theta_after(heads, layers, steps, heads_export=False, graph=True):
    from video_gcp_amd.training import GCPTrainStep
    hp, model = _model(heads, layers)
    model.use_graph = graph
    tr = GCPTrainStep(model, lr=1e-3)
    tr.attn_bwd_heads_export = heads_export
    inputs, noise, _ = make_inputs(hp, seed=31, variant="B")
    dev_in = {k: v.cuda() for k, v in inputs.items()}
    for _ in range(steps):
        out = tr.step(dev_in, noise.cuda())
    torch.cuda.synchronize()
    return model.theta.clone().view(torch.int32), float(out.raw["losses"][5])


def test_two_training_steps_are_reproducible_to_the_bit():
    a, la = _theta_after(2, 2, 2)
    b, lb = _theta_after(2, 2, 2)
    assert torch.equal(a, b) and la == lb


def test_one_head_one_layer_step_has_the_same_bits_through_the_heads_export():
    """(1, 1) issues the launches it always did (gcpx_attention_bwd on the saved weights); the same step with the softmax backward
    sent through gcpx_attention_bwd_heads, which computes the weights again, ends in the same parameters bit for bit"""
    a, la = _theta_after(1, 1, 2)
    b, lb = _theta_after(1, 1, 2, heads_export=True)
    assert torch.equal(a, b) and la == lb


def test_attention_panels_and_match_stats_read_the_last_layers_weights():
    """--log_images' attention panels and gcpx_match_stats take gamma of the last layer: at (2, 2) its rows are distributions over the
    frames and the panels of tests/test_gpu_image_log.py compose to their numpy restatement"""
    import test_gpu_image_log as TIL
    import video_gcp_amd as V
    from video_gcp_amd import image_log as IL
    from video_gcp_amd.model import GCPTreeModel
    hp = V.config("c5s", batch_size=5, n_attention_heads=2, n_attention_layers=2)          # the panels show three samples
    sd = V.init_params(hp, seed=1, randomize_affine=True)
    sd["decoder.log_sigma"].fill_(0.2)
    sd["tree_module.tree_modules.0.binding.temp"].fill_(0.05)
    model = GCPTreeModel(hp, params=sd, device="cuda")
    inputs, noise, _ = make_inputs(hp, seed=5, variant="B")
    dev_in = {k: v.cuda() for k, v in inputs.items()}
    out = model(dev_in, "train", noise=noise.cuda())
    torch.cuda.synchronize()
    gamma = out.tree.bf.gamma
    assert gamma.shape[0] == hp.batch_size and gamma.shape[-1] == hp.max_seq_len
    assert bool(((gamma.sum(-1) - 1).abs() < 1e-5).all()) and bool((gamma >= 0).all())
    assert out.raw["frame2node"].shape == (hp.batch_size, hp.max_seq_len)
    TIL._check_panels(model, IL.tree_panels(model, out, dev_in, "train"),
                      ["hierarchical_splits", "pruned_seq_gif", "match_overview", "gt_target_gif", "attention_masks"])
