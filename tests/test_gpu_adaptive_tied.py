"""-m gpu: the attentive training step with TIED tree levels (untied_layers = False: hyperparameters.py:117's default, what
base_configs/gcp_adaptive.py trains).  One tree module serves every level: the levels share the attention's projected keys / values,
whose gradient is the sum over the levels (gcpx_add_col_blocks, level L - 1 first), and every shared weight accumulates.

Shapes: c5s (B = 2, T = 12, 32 x 32, L = 4, N = 15) and c5s with max_seq_len = 7 (L = 3, N = 7 = T: the smallest tree soft-DTW takes, an
odd T).  Parameters as tests/test_gpu_attention_layers.py::_params sets them.  Tolerances are the project's own
(tests/test_gpu_adaptive.py, tests/test_gpu_attention_layers.py): a parameter gradient within 1e-3 of that gradient's max-abs + 5e-7,
the total loss 1e-4 relative, parameters after optimizer steps within 2e-3 * lr per step."""
import functools

import pytest
import torch

from helpers import make_inputs

pytestmark = pytest.mark.gpu

ATT = "tree_module.tree_modules.0.inference.attention"
TEMP = "tree_module.tree_modules.0.binding.temp"
SHAPES = [12, 7]


def _hp(heads, layers, T, learn_temp=False):
    import video_gcp_amd as V
    return V.config("c5s", max_seq_len=T, n_attention_heads=heads, n_attention_layers=layers, untied_layers=False,
                    learn_matching_temp=learn_temp)


@functools.lru_cache(maxsize=None)
def _params(heads, layers, T, learn_temp=False, temp=0.3):
    import video_gcp_amd as V
    hp = _hp(heads, layers, T, learn_temp)
    sd = V.init_params(hp, seed=1, randomize_affine=True)
    sd["decoder.log_sigma"].fill_(0.2)
    sd[TEMP].fill_(temp)
    for k in sd:
        if k.endswith(".temperature"):
            sd[k].fill_(0.7 + 0.2 * int(k.split(".")[-2]))
    return sd


def _trainer(heads, layers, T, learn_temp=False, graph=True, temp=0.3, **kw):
    from video_gcp_amd.model import GCPTreeModel
    from video_gcp_amd.training import GCPTrainStep
    hp = _hp(heads, layers, T, learn_temp)
    model = GCPTreeModel(hp, params={k: v.clone() for k, v in _params(heads, layers, T, learn_temp, temp).items()}, device="cuda")
    model.use_graph = graph
    return hp, model, GCPTrainStep(model, lr=1e-3, **kw)


@functools.lru_cache(maxsize=None)
def _oracle_grads(heads, layers, T, learn_temp, seed, temp=0.3):
    """autograd over the oracle (which handles tied attentive models), once per configuration on the CPU"""
    from oracle import gcp_model_oracle as O
    hp, sd = _hp(heads, layers, T, learn_temp), _params(heads, layers, T, learn_temp, temp)
    inputs, noise, _ = make_inputs(hp, seed=seed, variant="B")
    gref, _, total, _ = O.gradients(sd, hp, inputs, noise)
    return inputs, noise, gref, float(total.detach())


def _compare_grads(gref, got, rtol=1e-3, atol=5e-7):          # tests/test_gpu_adaptive.py
    bad = []
    for k, g in gref.items():
        h = got[k].cpu()
        err, scale = float((h - g).abs().max()), float(g.abs().max())
        if err > rtol * scale + atol:
            bad.append((k, err, scale))
    assert not bad, bad[:12]


def _backward_twice(tr, inputs, noise):
    dev_in = {k: v.cuda() for k, v in inputs.items()}
    for _ in range(2):
        out = tr.backward(dev_in, noise.cuda())
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("T", SHAPES)
@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("heads,layers", [(1, 1), (2, 2)])
def test_tied_gradients_match_autograd(heads, layers, graph, T):
    """every parameter's gradient of the one tree module against torch autograd over the oracle"""
    hp, model, tr = _trainer(heads, layers, T, graph=graph)
    inputs, noise, gref, total = _oracle_grads(heads, layers, T, False, 31)
    out = _backward_twice(tr, inputs, noise)
    assert abs(float(out.raw["losses"][5]) - total) <= 1e-4 * abs(total)
    got = tr.named_grads()
    assert not any(".tree_modules.1." in k for k in got) and set(gref) <= set(got)
    _compare_grads(gref, got)
    # the last layer's predictor_layers entry is computed and dropped by the reference: exactly zero, here and in autograd
    last = f"{ATT}.predictor_layers.{layers - 1}."
    unused = [k for k in got if last in k]
    assert len(unused) == 12
    for k in unused:
        assert float(got[k].abs().max()) == 0.0 and float(gref[k].abs().max()) == 0.0, k
    # what the levels share does get a gradient
    for i in range(layers):
        for nm in ("q_proj.weight", "k_proj.weight", "v_proj.weight", "out_proj.weight", "temperature"):
            assert float(got[f"{ATT}.attention_layers.{i}.{nm}"].abs().max()) > 0, (i, nm)
    assert float(got[f"{ATT}.query_net.input.linear.weight"].abs().max()) > 0
    assert float(got[TEMP].abs().max()) == 0.0


@pytest.mark.parametrize("T,temp", [(12, 0.3), (7, 0.3), (12, 0.02)])
def test_tied_gradients_with_a_learned_matching_temperature(T, temp):
    """learn_matching_temp = True: binding.temp receives the criterion's gradient through the matching weights.  At the temperature
    of _params (0.3) it is ~1e-6, of the size of the absolute part of the bound; the sharp posterior of
    tests/test_gpu_adaptive.py::test_adaptive_gradients_match_autograd_c5s (0.02) is checked as well, where the relative part decides"""
    hp, model, tr = _trainer(1, 1, T, learn_temp=True, graph=False, temp=temp)
    inputs, noise, gref, total = _oracle_grads(1, 1, T, True, 31, temp)
    out = _backward_twice(tr, inputs, noise)
    assert abs(float(out.raw["losses"][5]) - total) <= 1e-4 * abs(total)
    got = tr.named_grads()
    _compare_grads(gref, got)
    g, want = float(got[TEMP]), float(gref[TEMP])
    print(f"[tied] T {T} temp {temp}: d total / d binding.temp {g:.6e} (autograd {want:.6e})")
    assert want != 0.0 and abs(g - want) <= 1e-3 * abs(want) + 5e-7
    assert temp > 0.1 or abs(want) > 1e-4


def test_tied_two_radam_steps():
    """two optimisation steps against two steps of the oracle loop (tests/test_gpu_gauss_training.py::test_tree_two_radam_steps)"""
    from oracle import gcp_model_oracle as O
    from oracle.radam_oracle import RAdamOracle
    hp, model, tr = _trainer(1, 1, 12)
    ref_sd = {k: v.clone() for k, v in _params(1, 1, 12).items()}
    opt = RAdamOracle(lr=1e-3)
    for step in range(2):
        inputs, noise, _ = make_inputs(hp, seed=20 + step, variant="B")
        out = tr.step({k: v.cuda() for k, v in inputs.items()}, noise.cuda())
        torch.cuda.synchronize()
        gref, res, total, _ = O.gradients(ref_sd, hp, inputs, noise)
        assert abs(float(out.raw["losses"][5]) - float(total)) <= 1e-4 * abs(float(total)), step
        opt.step(ref_sd, gref)
        worst = max(float((model.sd[k].cpu() - ref_sd[k]).abs().max()) for k in gref)
        assert worst <= 2e-3 * 1e-3 * (step + 1) + 1e-7, (step, worst)


def _state_after(heads, layers, T, seeds, **kw):
    hp, model, tr = _trainer(heads, layers, T, **kw)
    for seed in seeds:
        inputs, noise, _ = make_inputs(hp, seed=seed, variant="B")
        tr.step({k: v.cuda() for k, v in inputs.items()}, noise.cuda())
    torch.cuda.synchronize()
    return model, tr


def test_two_tied_trainers_keep_identical_parameters():
    """two trainers fed the same two minibatches end with the same bits: the levels' key / value gradients are summed in a fixed order"""
    (m1, t1), (m2, t2) = _state_after(2, 2, 12, (40, 41)), _state_after(2, 2, 12, (40, 41))
    assert torch.equal(m1.theta, m2.theta) and torch.equal(t1.exp_avg, t2.exp_avg) and torch.equal(t1.exp_avg_sq, t2.exp_avg_sq)
    kp = m1.sd[f"{ATT}.attention_layers.1.k_proj.weight"].cpu()
    assert not torch.equal(kp, _params(2, 2, 12)[f"{ATT}.attention_layers.1.k_proj.weight"])          # ... and the shared weights moved


def test_tied_trainer_options_one_cycle():
    """accumulate = 2 with clipping and the non-finite guard: one full cycle runs, twice to the same bits, nothing non-finite"""
    opts = dict(accumulate=2, gradient_clip=1.0, nan_guard="skip")
    (m1, t1), (m2, t2) = _state_after(1, 1, 12, (50, 51), **opts), _state_after(1, 1, 12, (50, 51), **opts)
    assert t1.stepped and t2.stepped
    assert torch.equal(m1.theta, m2.theta) and torch.equal(t1.exp_avg, t2.exp_avg) and torch.equal(t1.exp_avg_sq, t2.exp_avg_sq)
    assert t1.health().summary.tolist() == [0, 0, 0, 0, -1, 0, 0, 0]
    assert bool(torch.isfinite(t1.grad).all()) and float(t1.exp_avg.abs().max()) > 0
    assert not torch.equal(m1.sd[f"{ATT}.attention_layers.0.v_proj.weight"].cpu(), _params(1, 1, 12)[f"{ATT}.attention_layers.0.v_proj.weight"])


@pytest.mark.parametrize("nblocks", [1, 2, 8])
@pytest.mark.parametrize("width", [32, 128])
@pytest.mark.parametrize("rows", [7, 24])
def test_add_col_blocks_matches_float64(rows, width, nblocks):
    """gcpx_add_col_blocks: the left-to-right f32 sum of nblocks column blocks, against float64.  Bound per element: nblocks - 1
    additions, each within 2^-24 of a partial sum that is at most the sum of the |x|: (nblocks - 1) 2^-24 sum |x|.  ld is larger than
    nblocks * width; the columns outside the blocks, the source and everything of dst beyond `width` stay what they were."""
    from video_gcp_amd import runtime as rt
    lib = rt.load_library()
    st = torch.cuda.current_stream().cuda_stream
    ld, ldd, off = nblocks * width + 12, width + 4, 4
    g = torch.Generator().manual_seed(rows + width + nblocks)
    src = (torch.rand(rows, ld, generator=g) * 2 - 1) * 10.0 ** torch.randint(-2, 3, (rows, ld), generator=g).float()
    src[:, :off] = 1.0e6
    src[:, off + nblocks * width:] = 1.0e6                                     # wherever the kernel must not read
    sd_, dst = src.cuda(), torch.full((rows, ldd), float("nan"), device="cuda")
    rt.check(lib.gcpx_add_col_blocks(sd_.data_ptr() + 4 * off, ld, nblocks, dst.data_ptr(), ldd, rows, width, st), "add_col_blocks")
    torch.cuda.synchronize()
    blocks = src[:, off:off + nblocks * width].double().view(rows, nblocks, width)
    want, scale = blocks.sum(1), blocks.abs().sum(1)
    got = dst[:, :width].double().cpu()
    assert bool(torch.isfinite(got).all())
    err = (got - want).abs()
    tol = (nblocks - 1) * 2.0 ** -24 * scale
    assert bool((err <= tol).all()), (float((err - tol).max()), float(err.max()))
    print(f"[ratio] add_col_blocks rows {rows} width {width} nblocks {nblocks}: worst err/tol "
          f"{float((err / tol.clamp_min(1e-300)).max()) if nblocks > 1 else 0.0:.3g}")
    assert bool(torch.isnan(dst[:, width:]).all()) and torch.equal(sd_.cpu(), src)
    # the order is the blocks' order: the f32 sum taken left to right, bit for bit
    acc = src[:, off:off + width].clone()
    for k in range(1, nblocks):
        acc = acc + src[:, off + k * width:off + (k + 1) * width]
    assert torch.equal(dst[:, :width].cpu(), acc)
    # in place: dst = block 0 of src; the other blocks and the columns around them are untouched
    rt.check(lib.gcpx_add_col_blocks(sd_.data_ptr() + 4 * off, ld, nblocks, sd_.data_ptr() + 4 * off, ld, rows, width, st), "add_col_blocks")
    torch.cuda.synchronize()
    after = sd_.cpu()
    assert torch.equal(after[:, off:off + width], acc)
    assert torch.equal(after[:, :off], src[:, :off]) and torch.equal(after[:, off + width:], src[:, off + width:])
    # bad sizes are refused before anything is launched
    assert lib.gcpx_add_col_blocks(sd_.data_ptr(), nblocks * width - 1, nblocks, dst.data_ptr(), ldd, rows, width, st) != 0
    assert lib.gcpx_add_col_blocks(sd_.data_ptr(), ld, nblocks, dst.data_ptr(), width - 1, rows, width, st) != 0
