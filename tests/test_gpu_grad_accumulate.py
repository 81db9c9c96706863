"""Gradient accumulation on the GPU (GCPTrainStep(accumulate=k), train.py --accumulate_steps k; csrc/scalar_f32.hip:
gcpx_grad_accumulate):
  1. the kernel, bit for bit against numpy.float32 addition / the copy: every size at which it takes another path (the 16-byte loop,
     its second access, the scalar remainder, unaligned slices), both `assign` values, a launch held to one workgroup, guards around
     dst, and a vector cut into slices;
  2. the accumulated gradient of the tree model against the float64 sum of the micro-gradients, and what must not move before the
     cycle's last micro-step;
  3. the step behind a cycle against the float64 optimizer reference of tests/optim_refs.py (plain, with gradient_clip, with
     early_optimizer off);
  4. the same as 2 for the sequential model;
  5. the guard: one verdict per cycle, `skip` drops the cycle, `raise` raises on its last micro-step;
  6. mean_losses();
  7. the trainer loop (global_step counts optimizer steps, checkpoint / resume) and the two dataset loaders.
A single IEEE addition leaves no tolerance to argue about in 1; 2 and 4 allow the k - 1 = 2 float32 additions of a sum of three:
gam(2) sum |g_j| per element (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., (4.4))."""
import os

import numpy as np
import pytest
import torch

import dataset_fixture as FX
import optim_refs as R
from helpers import make_inputs

pytestmark = pytest.mark.gpu

GUARD = 64                                         # floats in front of and behind dst (256 bytes: the slice's alignment is `off` alone)
SIZES = (0, 1, 3, 4, 5, 255, 256, 257, 2 * 256 * 4 * 2 + 7)      # 4103: one workgroup's two float4 accesses, twice over, + a remainder
ALL_OFFSETS = (257, 2 * 256 * 4 * 2 + 7)           # the sizes that run all 16 (dst, src) offsets; the others the diagonal
K = 3


# ----------------------------------------------------------------------------------------------------------------------
# 1. the kernel
# ----------------------------------------------------------------------------------------------------------------------
def _values(rng, n):
    """random signs, magnitudes 2^U(-20, 20): the sum of two is never subnormal unless it is an exact 0"""
    return (np.where(rng.rand(n) < 0.5, -1.0, 1.0) * 2.0 ** rng.uniform(-20, 20, n)).astype(np.float32)


def _pair(n, seed):
    rng = np.random.RandomState(seed)
    d, s = _values(rng, n), _values(rng, n)
    if n >= 3:
        s[n - 1] = np.nan                          # the last element: the scalar remainder (or the last float4)
    if n >= 4:
        s[0] = np.inf
    if n >= 5:
        d[1] = -s[1]                               # an exact cancellation
    if n >= 255:
        d[2:6] = (0.0, -0.0, -0.0, 0.0)
        s[2:6] = (-0.0, -0.0, 0.0, 0.0)
        d[100:110] = -s[100:110]
        d[n - 2] = -np.inf                         # -Inf + finite
        s[n // 2] = -np.inf
        d[n // 2] = np.inf                         # +Inf + -Inf = NaN
    return d, s


def _same_bits(got, want, what):
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN elements differ"
    ok = R.bits(got)[~nan] == R.bits(want)[~nan]
    assert ok.all(), f"{what}: {int((~ok).sum())} elements differ, first at {int(np.flatnonzero(~ok)[0])} of the non-NaN ones"


def _st():
    return torch.cuda.current_stream().cuda_stream


def _framed(values, off, seed):
    """`values` at GUARD + off floats of a buffer of random finite floats; host array"""
    buf = _values(np.random.RandomState(seed), GUARD + 4 + len(values) + GUARD)
    buf[GUARD + off:GUARD + off + len(values)] = values
    return buf


@pytest.mark.parametrize("n", SIZES)
def test_kernel_equals_float32_addition_bit_for_bit(gcpx_lib, n):
    from video_gcp_amd import runtime as rt
    d, s = _pair(n, 100 + n)
    with np.errstate(invalid="ignore"):
        want_add = d + s
    offsets = [(a, b) for a in range(4) for b in range(4)] if n in ALL_OFFSETS else [(a, a) for a in range(4)]
    for od, os_ in offsets:
        hd, hs = _framed(d, od, 7 + od), _framed(s, os_, 11 + os_)
        src = torch.from_numpy(hs).cuda()
        assert src.data_ptr() % 16 == 0
        for assign in (0, 1):
            want = hd.copy()
            want[GUARD + od:GUARD + od + n] = s if assign else want_add
            for max_blocks in (0, 1):
                dst = torch.from_numpy(hd).cuda()
                assert dst.data_ptr() % 16 == 0
                rt.check(gcpx_lib.gcpx_grad_accumulate(dst.data_ptr() + 4 * (GUARD + od), src.data_ptr() + 4 * (GUARD + os_), n, assign,
                                                       max_blocks, _st()), "grad_accumulate")
                got = dst.cpu().numpy()
                name = f"n={n} dst+{od} src+{os_} assign={assign} max_blocks={max_blocks}"
                _same_bits(got[GUARD + od:GUARD + od + n], want[GUARD + od:GUARD + od + n], name)
                assert np.array_equal(R.bits(got[:GUARD + od]), R.bits(want[:GUARD + od])), name + ": the floats in front of dst changed"
                assert np.array_equal(R.bits(got[GUARD + od + n:]), R.bits(want[GUARD + od + n:])), name + ": the floats behind dst changed"
                assert np.array_equal(R.bits(src.cpu().numpy()), R.bits(hs)), name + ": src changed"


def test_kernel_arguments(gcpx_lib):
    st = _st()
    assert gcpx_lib.gcpx_grad_accumulate(None, None, 0, 0, 0, st) == 0            # n = 0: a no-op
    x = torch.zeros(8, device="cuda")
    assert gcpx_lib.gcpx_grad_accumulate(x.data_ptr(), x.data_ptr() + 16, 0, 1, 0, st) == 0
    assert gcpx_lib.gcpx_grad_accumulate(x.data_ptr(), x.data_ptr() + 16, -1, 0, 0, st) == -1
    assert gcpx_lib.gcpx_grad_accumulate(x.data_ptr(), x.data_ptr() + 16, 4, 2, 0, st) == -1
    assert gcpx_lib.gcpx_grad_accumulate(x.data_ptr(), x.data_ptr() + 16, 4, 0, -1, st) == -1
    assert gcpx_lib.gcpx_grad_accumulate(None, x.data_ptr(), 4, 0, 0, st) == -1
    assert gcpx_lib.gcpx_grad_accumulate(x.data_ptr() + 2, x.data_ptr() + 16, 2, 0, 0, st) == -1      # not 4-byte aligned
    torch.cuda.synchronize()
    assert not x.any()


def test_kernel_slices_leave_the_bits_of_one_call(gcpx_lib):
    """one call over 4103 elements (the 16-byte loop + remainder) and three slices cut at 1001 and 2603 (the second and third start
    1 and 3 floats off a 16-byte boundary: the scalar loop)"""
    from video_gcp_amd import runtime as rt
    n = SIZES[-1]
    d, s = _pair(n, 5)
    src = torch.from_numpy(s).cuda()
    one, cut = torch.from_numpy(d).cuda(), torch.from_numpy(d).cuda()
    rt.check(gcpx_lib.gcpx_grad_accumulate(one.data_ptr(), src.data_ptr(), n, 0, 0, _st()), "grad_accumulate")
    for lo, hi in ((0, 1001), (1001, 2603), (2603, n)):
        assert lo % 4 or lo == 0
        rt.check(gcpx_lib.gcpx_grad_accumulate(cut.data_ptr() + 4 * lo, src.data_ptr() + 4 * lo, hi - lo, 0, 0, _st()), "grad_accumulate")
    with np.errstate(invalid="ignore"):
        want = d + s
    _same_bits(one.cpu().numpy(), want, "one call")
    _same_bits(cut.cpu().numpy(), want, "three slices")


# ----------------------------------------------------------------------------------------------------------------------
# the models
# ----------------------------------------------------------------------------------------------------------------------
def _tree(**kw):
    import video_gcp_amd as V
    from video_gcp_amd.model import GCPTreeModel
    from video_gcp_amd.training import GCPTrainStep
    hp = V.config("tiny")
    model = GCPTreeModel(hp, params=V.init_params(hp, seed=1, randomize_affine=True), device="cuda")
    return hp, model, GCPTrainStep(model, **kw)


def _sequential(**kw):
    import video_gcp_amd as V
    from video_gcp_amd.sequential import GCPSequentialModel
    from video_gcp_amd.training_sequential import SequentialTrainStep
    hp = V.config("c1", nz_mid_lstm=128, lstm_init="zero")            # the smallest configuration tests/test_gpu_sequential.py trains
    model = GCPSequentialModel(hp, params=V.init_params_sequential(hp, seed=1, randomize_affine=True), device="cuda")
    return hp, model, SequentialTrainStep(model, **kw)


def _micro_batches(hp, seeds=(21, 22, 23), n_latents=None):
    """three different micro-batches with fixed latent noise (n_latents: the sequential model draws one per step, T - 1)"""
    out = []
    for s in seeds:
        inputs, noise, _ = make_inputs(hp, seed=s, variant="B")
        if n_latents is not None:
            noise = noise[:, :n_latents].contiguous()
        out.append(({k: v.cuda() for k, v in inputs.items()}, noise.cuda()))
    return out


def _param_index(model):
    """the entries of theta that are parameters (model._poff without its buffers, as scalar_log.grad_tables names them); the rest are
    BatchNorm running statistics, which every training forward updates, and padding"""
    from video_gcp_amd.scalar_log import grad_tables
    names = grad_tables(model._poff)[0]
    assert 0 < len(names) < len(model._poff)
    idx = [np.arange(o, o + int(np.prod(shp, dtype=np.int64))) for o, shp in (model._poff[n] for n in names)]
    return np.concatenate(idx)


def _snapshot(tr):
    torch.cuda.synchronize()
    return dict(theta=tr.m.theta.cpu().numpy().copy(), m=tr.exp_avg.cpu().numpy().copy(), v=tr.exp_avg_sq.cpu().numpy().copy(),
                state=tr.opt_state.cpu().numpy().copy())


def _assert_unmoved(tr, before, pidx, what, state=slice(0, 4)):
    """state: the entries of opt_state that must keep their bits (a dropped cycle leaves its verdict in the gate, opt_state[3])"""
    now = _snapshot(tr)
    assert np.array_equal(R.bits(now["theta"][pidx]), R.bits(before["theta"][pidx])), what + ": parameters moved"
    for k in ("m", "v"):
        assert np.array_equal(R.bits(now[k]), R.bits(before[k])), f"{what}: {k} moved"
    assert np.array_equal(R.bits(now["state"][state]), R.bits(before["state"][state])), f"{what}: opt_state moved"


def _accumulated_gradient(make, n_latents=None):
    """test 2 / 4: trainer A (accumulate = 3, lr = 0) against the float64 sum of trainer B's three gradients"""
    hp, model_a, A = make(lr=0.0, accumulate=K)
    _, model_b, B = make(lr=0.0)
    assert torch.equal(model_a.theta, model_b.theta)
    batches = _micro_batches(hp, n_latents=n_latents)
    pidx = _param_index(model_a)
    assert A.micro_index == 0 and A.accumulate == K and B.accumulate == 1
    before = _snapshot(A)
    seen = []
    for j, (inputs, noise) in enumerate(batches):
        A.step(inputs, noise)
        seen.append((A.stepped, A.micro_index))
        if j < K - 1:
            _assert_unmoved(A, before, pidx, f"micro-step {j + 1}")
    assert seen == [(False, 1), (False, 2), (True, 0)], seen
    torch.cuda.synchronize()
    got = A.grad.cpu().numpy().astype(np.float64)
    assert float(A.opt_state[0]) == 1.0                      # the cycle stepped once (lr = 0: theta keeps its bits all the same)
    gs = []
    for inputs, noise in batches:
        B.backward(inputs, noise)
        torch.cuda.synchronize()
        gs.append(B.grad.cpu().numpy().astype(np.float64))
    assert B.micro_index == 0 and float(B.opt_state[0]) == 0.0
    want, mag = gs[0] + gs[1] + gs[2], np.abs(gs[0]) + np.abs(gs[1]) + np.abs(gs[2])
    assert np.isfinite(got).all() and float(mag[pidx].max()) > 0
    assert all(float(np.abs(g[pidx]).max()) > 0 for g in gs) and not np.array_equal(gs[0], gs[1])
    err, tol = np.abs(got - want), R.gam(K - 1) * mag
    worst = float((err / np.maximum(tol, 1e-300))[err > 0].max()) if (err > 0).any() else 0.0
    print(f"accumulated gradient: worst err / tol = {worst:.3g} over {got.size} elements")
    bad = err > tol
    assert not bad.any(), f"{int(bad.sum())} elements outside gam(2) sum|g_j|; first at {int(np.flatnonzero(bad)[0])}; worst {worst:.3g}"


def test_accumulated_gradient_tree():
    _accumulated_gradient(_tree)


def test_accumulated_gradient_sequential():
    _accumulated_gradient(_sequential, n_latents=19)               # c1: max_seq_len - 1


# ----------------------------------------------------------------------------------------------------------------------
# 3. the step behind a cycle
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["plain", "gradient_clip", "no_early_optimizer"])
def test_step_after_a_cycle_matches_float64(variant):
    """theta, m, v after the cycle within ref_step's one-step bounds, from the state before the cycle, the gradient buffer as the device
    left it (the cycle's sum) and grad_scale = f32(1 / 3).  gradient_clip: the coefficient the device left in opt_state[1] is held to
    ref_clip on that sum within clip_tol (the trainer's 1024 partials), and ref_step then reads the coefficient the kernel read."""
    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-8
    kw = dict(gradient_clip=1.0) if variant == "gradient_clip" else {}
    hp, model, A = _tree(lr=lr, betas=(b1, b2), eps=eps, accumulate=K, **kw)
    if variant == "no_early_optimizer":
        A.early_optimizer = False
    pidx = _param_index(model)
    before = _snapshot(A)
    for inputs, noise in _micro_batches(hp):
        A.step(inputs, noise)
    assert A.stepped and A.micro_index == 0
    after = _snapshot(A)
    grad = A.grad.cpu().numpy()
    assert float(after["state"][0]) == float(before["state"][0]) + 1.0 == 1.0
    scale = 1.0 / K
    state = before["state"].copy()
    if variant == "gradient_clip":
        rn, rc = R.ref_clip(grad, scale, 1.0)
        tn, tc = R.clip_tol(grad, scale, 1.0, 1024)
        print(f"clip: norm {float(after['state'][2])!r} (ref {rn!r}), coefficient {float(after['state'][1])!r} (ref {rc!r})")
        assert rc < 1.0                                      # the case clips
        R.ratio(after["state"][2], rn, tn, "clip norm")
        R.ratio(after["state"][1], rc, tc, "clip coefficient")
        state[1] = after["state"][1]
    else:
        assert float(after["state"][1]) == 0.0
    r = R.ref_step(0, before["theta"][pidx], grad[pidx], before["m"][pidx], before["v"][pidx], state, lr, b1, b2, eps, scale)
    worst = max(R.ratio(after["theta"][pidx], r["theta"], r["tol_theta"], "theta"), R.ratio(after["m"][pidx], r["m"], r["tol_m"], "m"),
                R.ratio(after["v"][pidx], r["v"], r["tol_v"], "v"))
    print(f"{variant}: worst err / tol = {worst:.3g}")
    assert not np.array_equal(after["theta"][pidx], before["theta"][pidx])
    # gradient_stats() of the completed cycle: the accumulated gradient under 1 / k (and the clip coefficient), float64 per parameter.
    # (1e-4: a float32 sum of positive squares over at most a few hundred roundings per path is good to ~1e-5; a forgotten 1 / 3 is 3x)
    stats = A.gradient_stats()
    torch.cuda.synchronize()
    coef = R.clip_factor(float(after["state"][1]))
    g64 = grad.astype(np.float64) * R.f32(scale) * coef
    want = np.array([np.sqrt(np.sum(g64[o:o + int(np.prod(shp, dtype=np.int64))] ** 2)) for o, shp in (model._poff[n] for n in stats.names)])
    got = stats.seg_norm.cpu().numpy().astype(np.float64)
    assert np.all(np.abs(got - want) <= 1e-4 * want + 1e-30), float(np.max(np.abs(got - want) / np.maximum(want, 1e-30)))


# ----------------------------------------------------------------------------------------------------------------------
# 5. guards
# ----------------------------------------------------------------------------------------------------------------------
def _poisoned(batches):
    inputs, noise = batches[1]
    bad = {k: v.clone() for k, v in inputs.items()}
    bad["traj_seq"][0, 0, 0, 0, 0] = float("nan")
    return [batches[0], (bad, noise), batches[2]]


def test_guard_skip_drops_the_whole_cycle():
    hp, model, A = _tree(lr=1e-3, accumulate=K, nan_guard="skip")
    pidx = _param_index(model)
    batches = _micro_batches(hp)
    before = _snapshot(A)
    for inputs, noise in _poisoned(batches):
        A.step(inputs, noise)
    assert A.stepped and A.micro_index == 0                  # the cycle is over, dropped on the device
    _assert_unmoved(A, before, pidx, "skipped cycle", state=slice(0, 1))
    assert float(A.opt_state[3]) == 1.0                      # the gate the health kernel closed
    s = A.health().summary.cpu().numpy()
    assert s[6] == 1 and s[7] == 1, s.tolist()
    for inputs, noise in batches:
        A.step(inputs, noise)
    after = _snapshot(A)
    s = A.health().summary.cpu().numpy()
    assert s[6] == 0 and s[7] == 1, s.tolist()
    assert float(after["state"][0]) == 1.0 and float(after["state"][3]) == 0.0
    assert not np.array_equal(after["theta"][pidx], before["theta"][pidx]) and np.isfinite(after["theta"][pidx]).all()


def test_guard_raise_raises_on_the_last_micro_step():
    from video_gcp_amd.health import NonFiniteGradients
    hp, model, A = _tree(lr=1e-3, accumulate=K, nan_guard="raise")
    pidx = _param_index(model)
    bad = _poisoned(_micro_batches(hp))
    before = _snapshot(A)
    A.step(*bad[0])
    A.step(*bad[1])
    assert (A.stepped, A.micro_index) == (False, 2)
    with pytest.raises(NonFiniteGradients):
        A.step(*bad[2])
    assert A.micro_index == 0
    _assert_unmoved(A, before, pidx, "raised cycle", state=slice(0, 1))


# ----------------------------------------------------------------------------------------------------------------------
# 6. losses
# ----------------------------------------------------------------------------------------------------------------------
def test_mean_losses_is_the_cycle_mean():
    """two float32 additions and one division: gam(3) of the mean of the magnitudes, per entry"""
    hp, model, A = _tree(lr=0.0, accumulate=K)
    seen = []
    for inputs, noise in _micro_batches(hp):
        out = A.step(inputs, noise)
        torch.cuda.synchronize()
        seen.append(out.raw["losses"].cpu().numpy().astype(np.float64))
    got = A.mean_losses()
    assert got.is_cuda and got.shape == (16,)
    got = got.cpu().numpy().astype(np.float64)
    want, mag = sum(seen) / K, sum(np.abs(x) for x in seen) / K
    assert want[5] != 0 and seen[0][5] != seen[1][5]
    err = np.abs(got - want)
    print("mean_losses: worst err / tol =", float((err / np.maximum(R.gam(K) * mag, 1e-300)).max()))
    assert np.all(err <= R.gam(K) * mag), (got, want)
    _, _, plain = _tree(lr=0.0)
    with pytest.raises(ValueError):
        plain.mean_losses()


# ----------------------------------------------------------------------------------------------------------------------
# 7. the trainer loop and the loaders
# ----------------------------------------------------------------------------------------------------------------------
def test_model_trainer_counts_optimizer_steps_and_resumes(tmp_path, capsys):
    from video_gcp_amd.train import ModelTrainer, get_cmd_args
    exp = str(tmp_path / "exp")
    argv = ["--path", exp, "--config", "tiny", "--accumulate_steps", "2", "--feed_random_data", "1", "--num_epochs", "1",
            "--batches_per_epoch", "5", "--log_outputs_interval", "1"]
    tr = ModelTrainer(get_cmd_args(argv))
    assert "[train] micro-batch 2 x accumulate_steps 2 x world 1 = effective batch 4" in capsys.readouterr().out
    assert tr.trainer.accumulate == 2 and len(tr.train_loader) == 4
    tr.run()
    assert tr.global_step == 2 and tr.model.n_steps == 2 and float(tr.trainer.opt_state[0]) == 2.0
    assert [s for s, _ in tr.log] == [0, 1] and all(np.isfinite(l) for _, l in tr.log)
    ck = torch.load(os.path.join(exp, "weights", "weights_ep0.pth"), map_location="cpu")
    assert set(ck) == {"epoch", "global_step", "state_dict", "optimizer"} and ck["global_step"] == 2
    tr2 = ModelTrainer(get_cmd_args(argv + ["--resume", "latest", "--num_epochs", "2", "--skip_first_val", "1"]))
    tr2.run()
    assert tr2.global_step == 4 and tr2.model.n_steps == 4 and float(tr2.trainer.opt_state[0]) == 4.0
    assert [s for s, _ in tr2.log] == [2, 3]


def test_both_loaders_hand_over_the_same_micro_batches(tmp_path):
    """HostFedLoader and ResidentLoader with accumulate = 2 over a seeded dataset: bit-identical micro-batches, and micro-batch g·2 + j
    is the numpy batch g of virtual rank j of 2 (two passes per epoch, 7 items: a pass drops 3 where the plain loader drops 1)"""
    import video_gcp_amd as V
    from video_gcp_amd import dataset as DS
    from video_gcp_amd import dataset_resident as DR
    from video_gcp_amd.model import GCPTreeModel
    hp = V.config("c1")
    model = GCPTreeModel(hp, params=V.init_params(hp, seed=1), device="cuda")
    T, img, B = hp.max_seq_len, hp.img_sz, hp.batch_size
    FX.write_random_dataset(str(tmp_path), T=T, img=img, n_files=1, traj_per_file=11, phases=("train",), min_len=5)
    ds = DS.VideoDataset(str(tmp_path), DS.load_spec(str(tmp_path)), "train", img, randomize_length=True)
    assert len(ds) == 11

    def collect(loader):
        loader.set_epoch(1)
        out = []
        for got in loader:
            torch.cuda.synchronize()
            out.append({k: v.cpu().clone() for k, v in got.items()})
        return out

    host = collect(DS.HostFedLoader(ds, model, B, n_repeat=2, seed=3, accumulate=2))
    res = collect(DR.ResidentLoader(ds, model, B, n_repeat=2, seed=3, accumulate=2))
    assert len(host) == len(res) == 2 * 2 * (11 // 4) == 8 and len(DS.HostFedLoader(ds, model, B, n_repeat=2, seed=3)) == 10
    ranks = [[DS.numpy_batch(ds, b, 3) for b in DS.epoch_schedule(len(ds), B, 2, 3, 1, True, rank=j, world=2)] for j in range(2)]
    for i, (h, r) in enumerate(zip(host, res)):
        want = ranks[i % 2][i // 2]
        assert set(h) == set(r)
        for k in h:
            assert torch.equal(h[k], r[k]), (i, k)
            assert torch.equal(h[k], torch.from_numpy(want[k])), (i, k)
