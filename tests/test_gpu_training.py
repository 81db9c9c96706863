"""Training step on MI355X (HIP forward + explicit backward + RAdam) against torch autograd over the CPU oracle.

The reference's loop: optimizer.zero_grad -> model(inputs) -> loss -> total -> backward -> optimizer.step
(/root/reference/gcp/prediction/train.py:155-163).  Stated tolerances: a parameter gradient may differ from the autograd
gradient by 1e-3 of that gradient's max-abs (+5e-7 absolute: conv biases in front of a BatchNorm have an exactly-zero
gradient which autograd reports as ~1e-7 rounding noise); after optimizer steps the parameters may differ by 2e-3 * lr
per step (RAdam's normalised update magnifies tiny gradient differences where |g| ~ eps)."""
import pytest
import torch

from helpers import make_inputs

pytestmark = pytest.mark.gpu


def _setup(name, graph, **over):
    import video_gcp_amd as V
    from video_gcp_amd.model import GCPTreeModel
    from video_gcp_amd.training import GCPTrainStep
    hp = V.config(name, **over)
    sd = V.init_params(hp, seed=1, randomize_affine=True)
    model = GCPTreeModel(hp, params=sd, device="cuda")
    model.use_graph = graph
    return hp, sd, model, GCPTrainStep(model, lr=1e-3)


def _compare_grads(gref, got, rtol=1e-3, atol=5e-7):
    bad = []
    for k, g in gref.items():
        h = got[k].cpu()
        err, scale = float((h - g).abs().max()), float(g.abs().max())
        if err > rtol * scale + atol:
            bad.append((k, err, scale))
    assert not bad, bad[:10]


@pytest.mark.parametrize("graph", [False, True])
def test_gradients_match_autograd_c1(graph):
    from oracle import gcp_model_oracle as O
    hp, sd, model, tr = _setup("c1", graph)
    inputs, noise, _ = make_inputs(hp, seed=7, variant="B")
    dev_in = {k: v.cuda() for k, v in inputs.items()}
    for _ in range(2):                      # second call replays the captured graphs
        out = tr.backward(dev_in, noise.cuda())
    torch.cuda.synchronize()
    gref, res, total, _ = O.gradients(sd, hp, inputs, noise)
    assert abs(float(out.raw["losses"][5]) - float(total)) <= 2e-5 * abs(float(total))
    got = tr.named_grads()
    _compare_grads(gref, got)
    # the inverse model and the cost model are trained (base_gcp.py:275-280): their heads receive a gradient
    assert "action_reconst" in res and "cost_estimation" in res
    for pre in ("inv_mdl.action_pred.", "cost_mdl.cost_pred."):
        ks = [k for k in gref if k.startswith(pre)]
        assert ks and all(float(got[k].abs().max()) > 0 for k in ks), pre


def _quantized_inputs(hp, seed):
    """make_inputs with the targets on the loader's 256 levels (k / 255 * 2 - 1, data_loader.py:220) and saturated bands at -1 / +1
    (every 25-room frame has them): the x = -1 / +1 branches of the likelihood and its gradient run.  I_0 / I_g follow the new frames."""
    inputs, noise, _ = make_inputs(hp, seed=seed, variant="B")
    tr = torch.round((inputs["traj_seq"] + 1) * 127.5) / 127.5 - 1
    tr[..., :3, :] = -1.0
    tr[..., -3:, :] = 1.0
    tr[..., 5, :] = 1 - 2 / 255.0
    tr = tr * inputs["pad_mask"][:, :, None, None, None]
    B = tr.shape[0]
    inputs.update(traj_seq=tr, I_0=tr[:, 0].clone(), I_g=tr[torch.arange(B), inputs["end_ind"]].clone())
    return inputs, noise


@pytest.mark.parametrize("mode", ["materialize_distr", "exact_f32"])
def test_gradients_match_autograd_c1_stored_params_likelihood(mode):
    """The balanced model's training step through the stored-parameters likelihood backward (gcpx_gather_rows + gcpx_dlm_nll_bwd,
    forward_plan.py:704-717) instead of the head's fused gradient: with materialize_distr=True, and on the exact-f32 build
    (model.split_f16 = False, fused_head_nll = False).  Quantized targets with saturated regions.  Every parameter gradient within the
    1e-3 of this file's header."""
    import video_gcp_amd as V
    from video_gcp_amd.model import GCPTreeModel
    from video_gcp_amd.training import GCPTrainStep
    from oracle import gcp_model_oracle as O
    hp = V.config("c1")
    sd = V.init_params(hp, seed=1, randomize_affine=True)
    model = GCPTreeModel(hp, params=sd, device="cuda", materialize_distr=(mode == "materialize_distr"))
    if mode == "exact_f32":
        model.split_f16 = False
        model.fused_head_nll = False
    model.use_graph = False
    tr = GCPTrainStep(model, lr=1e-3)
    inputs, noise = _quantized_inputs(hp, 7)
    assert bool((inputs["traj_seq"] == -1).any()) and bool((inputs["traj_seq"] == 1).any())
    dev_in = {k: v.cuda() for k, v in inputs.items()}
    out = tr.backward(dev_in, noise.cuda())
    torch.cuda.synchronize()
    gref, res, total, _ = O.gradients(sd, hp, inputs, noise)
    assert abs(float(out.raw["losses"][5]) - float(total)) <= 2e-5 * abs(float(total))
    _compare_grads(gref, tr.named_grads())


def test_gradients_match_autograd_c1_free_nats_burn_in():
    """The reference gcp_sequential configuration's KL settings on the tree model: free_nats = 1 (the per-dimension clamp of
    kl_bwd_kernel runs: dimensions below the floor get no gradient) and kl_weight_burn_in (the weight read from device memory,
    gcpx_kl_bwd_scheduled) after 4 model steps of a 10-step ramp.  The oracle runs with the weight the model reports.  Every
    parameter gradient within the 1e-3 of this file's header."""
    import dataclasses
    from oracle import gcp_model_oracle as O
    hp, sd, model, tr = _setup("c1", False, free_nats=1.0, kl_weight_burn_in=10)
    for _ in range(4):
        model.step()
    assert abs(model.kl_weight_now - 0.4 * hp.kl_weight) < 1e-12
    inputs, noise, _ = make_inputs(hp, seed=7, variant="B")
    dev_in = {k: v.cuda() for k, v in inputs.items()}
    out = tr.backward(dev_in, noise.cuda())
    torch.cuda.synchronize()
    hp_o = dataclasses.replace(hp, kl_weight=model.kl_weight_now, kl_weight_burn_in=None)
    gref, res, total, _ = O.gradients(sd, hp_o, inputs, noise)
    assert abs(float(out.raw["losses"][5]) - float(total)) <= 2e-5 * abs(float(total))
    _compare_grads(gref, tr.named_grads())


def _grad_errors(gref, got):
    """per parameter: max |difference| relative to the gradient's max-abs (parameters whose gradient is rounding noise skipped)"""
    return {k: float((got[k].cpu() - g).abs().max()) / float(g.abs().max()) for k, g in gref.items() if float(g.abs().max()) > 1e-6}


def _oracle_gradients_f64(sd, hp, inputs, noise, tol=None, force=None):
    """the oracle's gradients in float64 with the LeakyReLU kink probe (oracle.gcp_model_oracle.KINKS): returns (gradients, units with
    |pre-activation| < tol)"""
    from oracle import gcp_model_oracle as O
    d = lambda t: t.double() if torch.is_tensor(t) and t.is_floating_point() else t
    O.KINKS = {"tol": tol if tol is not None else 0.0, "force": force or {}}
    try:
        g, _, _, _ = O.gradients({k: d(v) for k, v in sd.items()}, hp, {k: d(v) for k, v in inputs.items()}, d(noise))
        found = list(O.KINKS.get("found", []))
    finally:
        O.KINKS = None
    return {k: v.float() for k, v in g.items()}, found


def test_gradients_full_length_sequences_c1():
    """variant A: every sequence uses all T frames (the planner's shape, cem_simulator.py:22), three input seeds, every parameter
    gradient within the 1e-3 stated at the top of this file — with the one exception the loss itself has: it is only piecewise smooth
    (LeakyReLU in every Predictor and conv block), and a unit whose pre-activation lies within the implementations' rounding
    difference of zero is differentiated on one side by the HIP kernels and possibly on the other by the oracle.  That is not
    asserted away with a loose bound but checked.  The oracle runs in float64 with a kink probe that lists the units with
    |pre-activation| < 5e-6 (a few f32 roundings of O(1) activations).  When the plain comparison misses 1e-3, each listed unit is
    flipped alone (one oracle run each; flips act additively on the gradient to first order), the flips that explain the residual are
    selected by projection, and ONE more oracle run with exactly those units on the other side must match the HIP gradient to 1e-3 in
    every parameter; the failure message names the units.  A seed without such units has no excuse."""
    flat = lambda g, keys: torch.cat([g[k].reshape(-1).double().cpu() / (float(gref[k].abs().max()) + 1e-30) for k in keys])
    for seed in (3, 5, 7):
        hp, sd, model, tr = _setup("c1", False, batch_size=3)
        inputs, noise, _ = make_inputs(hp, seed=seed, variant="A")
        tr.backward({k: v.cuda() for k, v in inputs.items()}, noise.cuda())
        torch.cuda.synchronize()
        got = tr.named_grads()
        gref, kinks = _oracle_gradients_f64(sd, hp, inputs, noise, tol=5e-6)
        err = _grad_errors(gref, got)
        worst = max(err, key=err.get)
        if err[worst] <= 1e-3:
            continue
        assert kinks, (seed, worst, err[worst], "no LeakyReLU unit near its kink: nothing explains the difference")
        kinks = sorted(kinks, key=lambda k: abs(k[2]))[:24]
        keys = [k for k in gref if float(gref[k].abs().max()) > 1e-6]
        resid = flat(got, keys) - flat(gref, keys)
        chosen = {}
        for c, i, v in kinks:
            side = -1 if v > 0 else 1
            g1, _ = _oracle_gradients_f64(sd, hp, inputs, noise, force={(c, i): side})
            delta = flat(g1, keys) - flat(gref, keys)
            if float(delta.abs().max()) > 1e-4 and float(resid @ delta) > 0.5 * float(delta @ delta):
                chosen[(c, i)] = side
        assert chosen, (seed, worst, err[worst], "no single flip of a near-kink unit explains the difference", kinks)
        g2, _ = _oracle_gradients_f64(sd, hp, inputs, noise, force=chosen)
        e2 = _grad_errors(g2, got)
        w2 = max(e2, key=e2.get)
        assert e2[w2] <= 1e-3, (seed, "plain:", worst, err[worst], "with units", chosen, "on the other side:", w2, e2[w2])


def test_radam_kernel_matches_oracle():
    from oracle.radam_oracle import RAdamOracle
    from video_gcp_amd import runtime as rt
    lib = rt.load_library()
    g = torch.Generator().manual_seed(0)
    n = 10007
    theta = torch.randn(n, generator=g)
    ref = {"p": theta.clone()}
    opt = RAdamOracle(lr=1e-2)
    th, m, v, st = theta.cuda(), torch.zeros(n).cuda(), torch.zeros(n).cuda(), torch.zeros(4).cuda()
    for step in range(8):                   # crosses the rho_t >= 5 switch (t = 6 for beta2 = 0.999)
        grad = torch.randn(n, generator=g) * (10.0 ** (step % 3 - 2))
        opt.step(ref, {"p": grad})
        gd = grad.cuda()
        rt.check(lib.gcpx_radam_step(th.data_ptr(), gd.data_ptr(), m.data_ptr(), v.data_ptr(), st.data_ptr(), n, 1e-2, 0.9, 0.999,
                                     1e-8, 1.0, torch.cuda.current_stream().cuda_stream), "radam")
        torch.cuda.synchronize()
        assert float((th.cpu() - ref["p"]).abs().max()) < 2e-6, step
    assert float(st[0]) == 8.0


def test_optimizer_slices_equal_one_call():
    """gcpx_optim_range over the slices of a step (tick with the last) leaves the bits of one gcpx_radam_step / gcpx_optim_step call"""
    from video_gcp_amd import runtime as rt
    lib = rt.load_library()
    g = torch.Generator().manual_seed(3)
    n, cuts = 20011, [0, 4096, 4101, 12000, 20011]        # (4101: a slice the 16-byte path cannot take)
    st_ = torch.cuda.current_stream().cuda_stream
    for kind, p1, p2 in [(0, 0.9, 0.999), (1, 0.9, 0.999), (2, 0.9, 0.99), (3, 0.9, 0.0)]:
        a = [torch.randn(n, generator=g).cuda(), torch.zeros(n).cuda(), torch.zeros(n).cuda(), torch.zeros(4).cuda()]
        b = [t.clone() for t in a]
        for step in range(7):
            gd = (torch.randn(n, generator=g) * 0.1).cuda()
            if kind == 0:
                rt.check(lib.gcpx_radam_step(a[0].data_ptr(), gd.data_ptr(), a[1].data_ptr(), a[2].data_ptr(), a[3].data_ptr(), n, 1e-2, p1, p2,
                                             1e-8, 0.5, st_), "radam")
            else:
                rt.check(lib.gcpx_optim_step(a[0].data_ptr(), gd.data_ptr(), a[1].data_ptr(), a[2].data_ptr(), a[3].data_ptr(), n, kind, 1e-2, p1,
                                             p2, 1e-8, 0.5, st_), "optim")
            order = list(zip(cuts[:-1], cuts[1:]))
            order = order[::-1] if step % 2 else order
            for j, (lo, hi) in enumerate(order):
                rt.check(lib.gcpx_optim_range(b[0].data_ptr() + 4 * lo, gd.data_ptr() + 4 * lo, b[1].data_ptr() + 4 * lo, b[2].data_ptr() + 4 * lo,
                                              b[3].data_ptr(), hi - lo, kind, 1e-2, p1, p2, 1e-8, 0.5, int(j == len(order) - 1), (0, 3, 64)[j % 3], st_), "range")
            torch.cuda.synchronize()
            for x, y in zip(a, b):
                assert torch.equal(x, y), (kind, step)
        assert float(b[3][0]) == 7.0


@pytest.mark.parametrize("name", ["c1", "c5s"])
def test_step_with_slices_applied_during_the_backward_equals_the_late_step(name):
    """step() updates a tree level's slice of the parameters (and re-packs its weights) on the caller's stream as soon as the backward
    marks it final; with GCPX_NO_EARLY_OPTIMIZER (early_optimizer = False) everything happens behind the backward.  Same bits in the
    parameters, both moment vectors, the counter and every packed weight after three steps — an update that ran before a late reader
    of its weights, or a pack left stale, shows up here."""
    hp, sd, ma, ta = _setup(name, True)
    _, _, mb, tb = _setup(name, True)
    tb.early_optimizer = False
    assert len(ta._ranges) == hp.hierarchy_levels + 1
    for step in range(3):
        inputs, noise, _ = make_inputs(hp, seed=30 + step, variant="B")
        dev_in = {k: v.cuda() for k, v in inputs.items()}
        oa = ta.step(dev_in, noise.cuda())
        if step == 0:
            assert ta._applied == set() and ta._early_on is False         # consumed by the optimizer step
        ob = tb.step(dev_in, noise.cuda())
        torch.cuda.synchronize()
        assert torch.equal(oa.raw["losses"], ob.raw["losses"]), step
        for x, y, what in [(ma.theta, mb.theta, "theta"), (ta.exp_avg, tb.exp_avg, "exp_avg"), (ta.exp_avg_sq, tb.exp_avg_sq, "exp_avg_sq"),
                           (ta.opt_state, tb.opt_state, "state"), (ma._arena, mb._arena, "packed weights")]:
            assert torch.equal(x, y), (step, what)
        for k in ma.pk_split:
            assert torch.equal(ma.pk_split[k]["out"], mb.pk_split[k]["out"]), (step, k)
    assert float(ta.opt_state[0]) == 3.0


def test_grouped_level_launches_give_the_gradient_of_single_launches():
    """A level's posterior + prior Predictor backward as one grouped launch (gcpx_mlp_bwd_group: the same function per workgroup) and the
    three layers' d h_prev GEMMs as one batched launch (same GEMM, blockIdx.z = layer; the launch heuristics may pick another tile for
    the larger grid, so sums may be ordered differently): 3 launches per level less on the chain, the same gradient to f32 rounding."""
    hp, sd, ma, ta = _setup("c1", False)
    _, _, mb, tb = _setup("c1", False)
    tb.group_mlp_bwd, tb.batch_dh = False, False
    inputs, noise, _ = make_inputs(hp, seed=41, variant="B")
    dev_in = {k: v.cuda() for k, v in inputs.items()}
    ta.backward(dev_in, noise.cuda())
    tb.backward(dev_in, noise.cuda())
    torch.cuda.synchronize()
    na = sum(1 for op in ta.last_bplan.ops if not op[0].startswith("@"))
    nb = sum(1 for op in tb.last_bplan.ops if not op[0].startswith("@"))
    assert nb - na == 3 * hp.hierarchy_levels, (na, nb)
    ga, gb = ta.named_grads(), tb.named_grads()
    for k in ga:
        scale = float(gb[k].abs().max())
        assert float((ga[k] - gb[k]).abs().max()) <= 2e-6 * scale + 1e-12, k
    # the grouped Predictor launch itself is bit-identical
    tb2 = tb
    tb2.group_mlp_bwd = True
    tb2._drop_bplans()
    tb2.backward(dev_in, noise.cuda())
    torch.cuda.synchronize()
    gc = tb2.named_grads()
    for k in gb:
        assert torch.equal(gb[k], gc[k]), k


@pytest.mark.parametrize("name,over", [("c1", {}), ("c5s", {"learn_matching_temp": True})])
def test_two_trainers_keep_identical_parameters(name, over):
    """Two trainers fed the same minibatches hold bit-identical parameters and optimizer moments after three steps (balanced model;
    adaptive model with the learned matching temperature): no float atomics, fixed summation orders, every hand-over between the lanes,
    the optimizer's stream and torch's own launches ordered (the flat model's twin test found one that was not)."""
    hp, sd, m1, t1 = _setup(name, "auto", **over)
    _, _, m2, t2 = _setup(name, "auto", **over)
    for step in range(3):
        inputs, noise, _ = make_inputs(hp, seed=60 + step, variant="B")
        dev_in, nz = {k: v.cuda() for k, v in inputs.items()}, noise.cuda()
        t1.step(dev_in, nz)
        t2.step(dev_in, nz)
    torch.cuda.synchronize()
    assert torch.equal(m1.theta, m2.theta) and torch.equal(t1.exp_avg, t2.exp_avg) and torch.equal(t1.exp_avg_sq, t2.exp_avg_sq)
    assert torch.equal(t1.grad, t2.grad)


def test_two_training_steps_c1():
    """losses of two consecutive optimisation steps and the updated parameters against the oracle loop"""
    from oracle import gcp_model_oracle as O
    from oracle.radam_oracle import RAdamOracle
    hp, sd, model, tr = _setup("c1", True)
    ref_sd = {k: v.clone() for k, v in sd.items()}
    opt = RAdamOracle(lr=1e-3)
    for step in range(2):
        inputs, noise, _ = make_inputs(hp, seed=20 + step, variant="B")
        out = tr.step({k: v.cuda() for k, v in inputs.items()}, noise.cuda())
        torch.cuda.synchronize()
        gref, res, total, _ = O.gradients(ref_sd, hp, inputs, noise)
        assert abs(float(out.raw["losses"][5]) - float(total)) <= 5e-5 * abs(float(total)), step
        opt.step(ref_sd, gref)
        worst = max(float((model.sd[k].cpu() - ref_sd[k]).abs().max()) for k in gref)
        assert worst <= 2e-3 * 1e-3 * (step + 1) + 1e-7, (step, worst)


def test_training_step_c2_shapes_runs_and_decreases_loss():
    """full-size shapes (64x64, T=80, L=7; batch 4 to bound the run time): finite gradients, loss goes down on a fixed batch"""
    hp, sd, model, tr = _setup("c2", True, batch_size=4)
    tr.lr = 2e-3
    inputs, noise, _ = make_inputs(hp, seed=5, variant="B")
    dev_in = {k: v.cuda() for k, v in inputs.items()}
    losses = []
    for _ in range(6):
        out = tr.step(dev_in, noise.cuda())
        losses.append(float(out.raw["losses"][5]))
    assert all(torch.isfinite(torch.tensor(losses)))
    assert torch.isfinite(tr.grad).all()
    assert losses[-1] < losses[0], losses


@pytest.mark.parametrize("name", ["c1", "c5s", "c5s+temp"])
def test_bucket_marks_follow_every_write_of_their_slice(name):
    """The data-parallel exchange starts a bucket's all-reduce at its `mark` in the backward plan (training.py: plan.mark("bucket", i)
    behind the level's flush).  That is only right if NOTHING writes into the bucket's slice of the flat gradient after the mark: a late
    write either races the collective or leaves a rank-local gradient that RAdam still scales by 1 / world.  The real backward plan of
    GCPTrainStep is replayed eagerly with the mark hook taking a snapshot of the bucket's slice (after waiting for every lane); the
    final gradient must equal the snapshots bit for bit.  c5s covers the attentive posterior, whose k_proj / v_proj weight gradients
    were once issued after the tree loop, i.e. after their level's mark (round-2 advisor finding); "c5s+temp": the learned matching
    temperature, a parameter of tree module 0 whose gradient is issued from the loss section on a side lane."""
    from video_gcp_amd.dist import gradient_bucket_ranges
    hp, sd, model, tr = _setup(name.split("+")[0], False, **({"learn_matching_temp": True} if name.endswith("+temp") else {}))
    ranges = gradient_bucket_ranges(model._poff, hp.hierarchy_levels, hp.untied_layers)
    assert len(ranges) == hp.hierarchy_levels + 1               # one bucket per level L-1 .. 0, then the rest
    tr._bucket_index = {n: i for i, (n, _, _) in enumerate(ranges)}      # what a process group switches on (training.py:53)
    snaps = {}

    def hook(tag, i):
        if tag != "bucket":
            return
        assert i not in snaps
        torch.cuda.synchronize()
        _, lo, hi = ranges[i]
        snaps[i] = tr.grad[lo:hi].clone()
    tr._on_mark = hook
    inputs, noise, _ = make_inputs(hp, seed=11, variant="B")
    tr.backward({k: v.cuda() for k, v in inputs.items()}, noise.cuda())
    torch.cuda.synchronize()
    assert sorted(snaps) == list(range(len(ranges) - 1)), sorted(snaps)      # every tree level's bucket was marked, in plan order
    names = tr.named_grads()
    for i, snap in snaps.items():
        n, lo, hi = ranges[i]
        assert float(snap.abs().max()) > 0, n
        if not torch.equal(tr.grad[lo:hi], snap):
            late = [k for k, (o, shp) in model._poff.items() if lo <= o < hi and
                    not torch.equal(names[k].reshape(-1), snap[o - lo:o - lo + names[k].numel()])]
            raise AssertionError(f"bucket {n}: written after its mark: {late[:8]}")


@pytest.mark.parametrize("kind,momentum", [("adam", 0.0), ("rmsprop", 0.0), ("rmsprop", 0.9), ("sgd", 0.0), ("sgd", 0.9)])
@pytest.mark.parametrize("clip", [None, 0.5])
def test_other_optimizers_and_gradient_clip_match_torch(kind, momentum, clip):
    """the trainer's `optimizer` / `momentum` / `gradient_clip` options (gcp_builder.py:174-186,255-263): Adam, RMSprop and SGD as
    torch.optim defines them (the classes the reference instantiates), gradient clipping = torch.nn.utils.clip_grad_norm_ over all
    parameters (spec of blox' get_clipped_optimizer, absent), on a flat vector through the kernels GCPTrainStep.optimizer_step calls"""
    from video_gcp_amd import runtime as rt
    lib = rt.load_library()
    g = torch.Generator().manual_seed(3)
    n = 10007
    p_ref = torch.nn.Parameter(torch.randn(n, generator=g))
    opt = {"adam": lambda: torch.optim.Adam([p_ref], lr=1e-2, betas=(0.9, 0.999), eps=1e-8),
           "rmsprop": lambda: torch.optim.RMSprop([p_ref], lr=1e-2, alpha=0.99, eps=1e-8, momentum=momentum),
           "sgd": lambda: torch.optim.SGD([p_ref], lr=1e-2, momentum=momentum)}[kind]()
    th, m, v, st = p_ref.detach().clone().cuda(), torch.zeros(n).cuda(), torch.zeros(n).cuda(), torch.zeros(4).cuda()
    part = torch.empty(256).cuda()
    code = {"adam": 1, "rmsprop": 2, "sgd": 3}[kind]
    p1, p2 = (0.9, 0.999) if kind == "adam" else ((momentum, 0.99) if kind == "rmsprop" else (momentum, 0.0))
    s = torch.cuda.current_stream().cuda_stream
    for step in range(6):
        grad = torch.randn(n, generator=g) * (10.0 ** (step % 3 - 1))
        p_ref.grad = grad.clone()
        if clip:
            torch.nn.utils.clip_grad_norm_([p_ref], clip)
        opt.step()
        gd = (2.0 * grad).cuda()                       # two ranks' summed gradient, averaged through grad_scale = 0.5
        if clip:
            rt.check(lib.gcpx_grad_clip_coef(gd.data_ptr(), n, 0.5, clip, part.data_ptr(), 256, st.data_ptr(), s), "clip")
        rt.check(lib.gcpx_optim_step(th.data_ptr(), gd.data_ptr(), m.data_ptr(), v.data_ptr(), st.data_ptr(), n, code, 1e-2, p1, p2, 1e-8,
                                     0.5, s), "optim")
        torch.cuda.synchronize()
        if clip:
            assert abs(float(st[2]) - float(grad.norm())) <= 1e-5 * float(grad.norm())
        assert float((th.cpu() - p_ref.detach()).abs().max()) < 5e-6, (kind, step)
    assert float(st[0]) == 6.0


def test_training_step_with_adam_and_clipping_c1():
    """GCPTrainStep(optimizer='adam', gradient_clip=...) end to end against the oracle's gradients pushed through torch.optim.Adam"""
    import video_gcp_amd as V
    from oracle import gcp_model_oracle as O
    from video_gcp_amd.model import GCPTreeModel
    from video_gcp_amd.training import GCPTrainStep
    hp = V.config("c1")
    sd = V.init_params(hp, seed=1, randomize_affine=True)
    model = GCPTreeModel(hp, params=sd, device="cuda")
    tr = GCPTrainStep(model, lr=1e-3, optimizer="adam", gradient_clip=0.05)
    names = [k for k in sd if not k.endswith(("running_mean", "running_var"))]
    ref = {k: torch.nn.Parameter(sd[k].clone()) for k in names}
    opt = torch.optim.Adam(list(ref.values()), lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
    for step in range(2):
        inputs, noise, _ = make_inputs(hp, seed=40 + step, variant="B")
        # every step starts from the HIP model's own parameters (Adam turns rounding-noise gradients into +-lr moves, see below: the
        # two trajectories would drift apart in exactly those elements and take the rest with them)
        for k, p in ref.items():
            p.data.copy_(model.sd[k].cpu())
        tr.step({k: v.cuda() for k, v in inputs.items()}, noise.cuda())
        torch.cuda.synchronize()
        cur = dict(sd, **{k: p.detach() for k, p in ref.items()})
        gref, _, _, _ = O.gradients(cur, hp, inputs, noise)
        for k, p in ref.items():
            p.grad = gref[k].clone()
        total = torch.nn.utils.clip_grad_norm_(list(ref.values()), 0.05)
        assert abs(float(tr.opt_state[2]) - float(total)) <= 2e-3 * float(total)     # the clipped quantity: the global gradient norm
        opt.step()
        # Adam normalises every element by its own magnitude: an element whose gradient is rounding noise (conv biases in front of a
        # BatchNorm: exactly zero, ~1e-7 in either implementation) moves by +-lr on the noise's sign.  Compared: the elements whose
        # gradient stands clear of that noise in every step so far
        if step == 0:
            solid = {k: torch.ones_like(gref[k], dtype=torch.bool) for k in names}
        for k in names:
            solid[k] &= gref[k].abs() > 0.2 * float(gref[k].abs().max()) + 1e-5
        worst = max(float((model.sd[k].cpu() - ref[k].detach())[solid[k]].abs().max()) for k in names if bool(solid[k].any()))
        assert sum(int(m_.sum()) for m_ in solid.values()) > 1000
        # a gradient element is matched to 1e-3 of its tensor's max-abs, i.e. to <= 0.5 % of its own value here, and Adam's update is
        # lr x (a ratio of such elements): 2e-2 lr; a wrong formula or a missing clip is off by O(lr)
        assert worst <= 2e-2 * 1e-3, (step, worst)
    with pytest.raises(ValueError):
        GCPTrainStep(model, optimizer="lbfgs")


@pytest.mark.parametrize("tree_lstm,lstm_init", [("sum", "zero"), ("linear", "mlp"), ("", "mlp")])
def test_gradients_tree_lstm_variants_c1(tree_lstm, lstm_init):
    """training step with the Sum / Lin TreeLSTM merge and the zero initialiser (tree_lstm.py:11-27,68-70): every parameter gradient
    against autograd over the oracle.  5e-3 here: a wrong or missing merge backward is off by O(1) in the projection / upstream
    gradients; differences of 2-3e-3 in a few tensors are LeakyReLU units on the other side of their kink (dissected, unit by unit, in
    test_gradients_full_length_sequences_c1)."""
    from oracle import gcp_model_oracle as O
    hp, sd, model, tr = _setup("c1", False, tree_lstm=tree_lstm, lstm_init=lstm_init)
    inputs, noise, _ = make_inputs(hp, seed=9, variant="B")
    tr.backward({k: v.cuda() for k, v in inputs.items()}, noise.cuda())
    torch.cuda.synchronize()
    gref, _, _, _ = O.gradients(sd, hp, inputs, noise)
    _compare_grads(gref, tr.named_grads(), rtol=5e-3)


def test_kl_weight_burn_in_follows_the_step_counter():
    """kl_weight_burn_in (hyperparameters.py:42, base_gcp.py:121-128; the 25-room gcp_sequential conf sets 1e4): the KL weight starts at 0
    and is kl_weight * min(1, steps / burn_in) after `steps` calls of model.step() (LinearUpdater is blox, absent: this build's spec).
    The weight lives in a device scalar, so the CAPTURED forward graph and the backward plan built at weight 0 must give the loss and
    every gradient of the oracle at the current weight."""
    import dataclasses
    from oracle import gcp_model_oracle as O
    hp, sd, model, tr = _setup("c1", True, kl_weight_burn_in=4.0)
    inputs, noise, _ = make_inputs(hp, seed=11, variant="B")
    dev_in = {k: v.cuda() for k, v in inputs.items()}
    for steps, w in ((0, 0.0), (2, 0.5), (9, 1.0)):
        while getattr(model, "n_steps", 0) < steps:
            model.step()
        assert abs(model.kl_weight_now - w * hp.kl_weight) < 1e-12
        out = tr.backward(dev_in, noise.cuda())
        torch.cuda.synchronize()
        hp_w = dataclasses.replace(hp, kl_weight=w * hp.kl_weight, kl_weight_burn_in=None)
        gref, res, total, _ = O.gradients(sd, hp_w, inputs, noise)
        assert abs(float(out.raw["losses"][5]) - float(total)) <= 2e-5 * abs(float(total)), (steps, float(out.raw["losses"][5]), float(total))
        assert abs(float(model.loss(dev_in, out)["kl"].weight) - w * hp.kl_weight) < 1e-12
        _compare_grads(gref, tr.named_grads(), rtol=2e-3)


@pytest.mark.parametrize("cfg", ["c1", "c5s"])
def test_seq_enc_none_forward_and_gradients(cfg):
    """seq_enc = 'none' (base_gcp.py:131-132: build_temporal_inf_encoder returns Identity — the posterior gathers / attends over the
    encoded frames themselves, and so does the attention-key encoder's temporal part): no inf_encoder parameters, the forward against
    the oracle and every parameter gradient against autograd over it"""
    from oracle import gcp_model_oracle as O
    import video_gcp_amd as V
    hp, sd, model, tr = _setup(cfg, False, seq_enc="none")
    assert not any(k.startswith("inf_encoder.") or k.startswith("inf_key_encoder.0.") for k in sd)
    inputs, noise, _ = make_inputs(hp, seed=11, variant="B")
    dev_in = {k: v.cuda() for k, v in inputs.items()}
    out = tr.backward(dev_in, noise.cuda())
    torch.cuda.synchronize()
    gref, res, total, ref = O.gradients(sd, hp, inputs, noise)
    assert abs(float(out.raw["losses"][5]) - float(total)) <= (1e-4 if cfg == "c5s" else 2e-5) * abs(float(total))
    _compare_grads(gref, tr.named_grads(), rtol=5e-3)
    from video_gcp_amd.model import GCPTreeModel
    with pytest.raises(ValueError):                                  # 'lstm' / 'bi-lstm' are blox modules: refused, not approximated
        GCPTreeModel(V.config("c1", seq_enc="lstm"), device="cuda")


def test_supervised_decoder_leaves_the_state_regressor_out():
    """supervised_decoder=True (hyperparameters.py:118) as base_gcp.py:252-256 is written: the regressor call sits inside
    `if not supervised_decoder:`, so no `regressed_state`, no state-regression loss, zero gradient for the regressor's (still present)
    parameters; everything else trains as before — total loss and every gradient against autograd over the oracle"""
    from oracle import gcp_model_oracle as O
    hp, sd, model, tr = _setup("c1", False, supervised_decoder=True)
    assert hp.attach_state_regressor and not hp.run_state_regressor and any(k.startswith("state_regressor.") for k in sd)
    inputs, noise, _ = make_inputs(hp, seed=13, variant="B")
    dev_in = {k: v.cuda() for k, v in inputs.items()}
    out = tr.backward(dev_in, noise.cuda())
    torch.cuda.synchronize()
    gref, res, total, ref = O.gradients(sd, hp, inputs, noise)
    assert "state_regression" not in res and "regressed_state" not in ref
    assert abs(float(out.raw["losses"][5]) - float(total)) <= 2e-5 * abs(float(total))
    got = tr.named_grads()
    _compare_grads(gref, got)
    assert all(float(got[k].abs().max()) == 0.0 for k in got if k.startswith("state_regressor."))
    fwd = model(dev_in, "train", noise=noise.cuda())
    assert "regressed_state" not in fwd


def test_a_trainer_whose_plans_are_dropped_keeps_identical_parameters():
    """Trainer A takes four steps; trainer B two, then model._clear_plans() — which closes B's forward plans and, through the listener,
    its backward plans: events and graphs destroyed behind a device synchronise — then two more on rebuilt plans.  Same bits in the
    parameters and both moment vectors."""
    hp, sd, ma, ta = _setup("c1", "auto", batch_size=3)
    _, _, mb, tb = _setup("c1", "auto", batch_size=3)
    for step in range(4):
        inputs, noise, _ = make_inputs(hp, seed=70 + step, variant="B")
        dev_in, nz = {k: v.cuda() for k, v in inputs.items()}, noise.cuda()
        ta.step(dev_in, nz)
        tb.step(dev_in, nz)
        if step == 1:
            old_f, old_b = mb._last_plan, tb.last_bplan
            assert not old_f.closed and not old_b.closed and tb._bplans[old_f.key] is old_b
            mb._clear_plans()
            assert old_f.closed and old_b.closed and mb._plans == {} and tb._bplans == {}
    torch.cuda.synchronize()
    assert tb.last_bplan is not old_b and not tb.last_bplan.closed and len(tb._bplans) == 1
    assert torch.equal(ma.theta, mb.theta) and torch.equal(ta.exp_avg, tb.exp_avg) and torch.equal(ta.exp_avg_sq, tb.exp_avg_sq)


def test_a_sequential_trainer_whose_segment_graphs_are_dropped_keeps_identical_gradients():
    """The flat model's trainer replays runs of its backward plan as small graphs by default (`bplan.segments`, captured in the first
    backward, replayed from the second).  Three backwards, the plans dropped (the segment graphs destroyed with them), three more — against
    a twin that never dropped: the same gradient bit for bit."""
    import video_gcp_amd as V
    from video_gcp_amd.sequential import GCPSequentialModel
    from video_gcp_amd.training_sequential import SequentialTrainStep
    hp = V.config("c1", nz_mid_lstm=128, lstm_init="zero", batch_size=3)
    sd = V.init_params_sequential(hp, seed=1, randomize_affine=True)
    m1, m2 = (GCPSequentialModel(hp, params=sd, device="cuda") for _ in range(2))
    tr1, tr2 = SequentialTrainStep(m1, lr=1e-3), SequentialTrainStep(m2, lr=1e-3)
    has_graph = lambda bplan: any(op[0] == "@graph" for op in bplan.segments or [])
    for i in range(6):
        inputs, noise, _ = make_inputs(hp, seed=80 + i, variant="B")
        dev_in, nz = {k: v.cuda() for k, v in inputs.items()}, noise[:, :hp.max_seq_len - 1].contiguous().cuda()
        tr1.backward(dev_in, nz)
        tr2.backward(dev_in, nz)
        if i == 2:
            old = tr2.last_bplan
            assert has_graph(old) and not old.closed
            m2._clear_plans()
            assert old.closed and old.segments is None and tr2._bplans == {}
    torch.cuda.synchronize()
    assert tr2.last_bplan is not old and has_graph(tr2.last_bplan) and has_graph(tr1.last_bplan)
    assert torch.equal(tr1.grad, tr2.grad)
