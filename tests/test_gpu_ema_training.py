"""The weight average in the trainer (GCPTrainStep(ema_decay=...), training.py) on the GPU, tree model (`tiny`) and flat model (the small
sequential configuration of tests/test_gpu_sequential.py):
  1. it only reads: an averaging trainer and a plain one, fed the same batches and noise, end with the same bits everywhere;
  2. the average follows the float64 recurrence over the per-step snapshots of theta with the warm-up decays, within the two-rounding
     bounds of tests/ema_refs.py -- per step against the device's own previous average, and summed over the steps against the pure
     float64 recurrence (|E_k| <= (1 - omd_k) |E_k-1| + b_k <= |E_k-1| + b_k: the update contracts the error it inherits);
  3. a step the guard drops and the micro-steps of an accumulation cycle leave every bit of it;
  4. ema_weights(): the forward inside is the forward of a model loaded from ema_state(), and everything is back afterwards;
  5. checkpoint and resume, through the trainer and through train.py."""
import os
import warnings

import numpy as np
import pytest
import torch

import ema_refs as E
from helpers import make_inputs

pytestmark = pytest.mark.gpu

DECAY = 0.999
STEPS = 4


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
    hp = V.config("c1", nz_mid_lstm=128, lstm_init="zero")
    model = GCPSequentialModel(hp, params=V.init_params_sequential(hp, seed=1, randomize_affine=True), device="cuda")
    return hp, model, SequentialTrainStep(model, **kw)


def _batches(hp, n=STEPS, n_latents=None, first_seed=31):
    out = []
    for s in range(first_seed, first_seed + n):
        inputs, noise, _ = make_inputs(hp, seed=s, variant="B")
        if n_latents is not None:
            noise = noise[:, :n_latents].contiguous()
        out.append(({k: v.cuda() for k, v in inputs.items()}, noise.cuda()))
    return out


def _bits(t):
    torch.cuda.synchronize()
    return E.bits(t.detach().cpu().numpy())


def _state(tr):
    return dict(theta=_bits(tr.m.theta), m=_bits(tr.exp_avg), v=_bits(tr.exp_avg_sq), state=_bits(tr.opt_state))


VARIANTS = {"tree": (_tree, {}, None), "tree_clip": (_tree, dict(gradient_clip=1.0), None), "sequential": (_sequential, {}, 19)}
_RUNS = {}


def _run(variant):
    """4 steps of an averaging trainer and of a plain one on the same batches and noise; the snapshots both tests below read"""
    if variant not in _RUNS:
        make, kw, n_latents = VARIANTS[variant]
        hp, model_a, A = make(lr=1e-3, ema_decay=DECAY, **kw)
        _, model_b, B = make(lr=1e-3, **kw)
        assert B.ema is None and B.ema_decay is None and torch.is_tensor(A.ema) and A.ema_updates == 0
        assert A.ema.data_ptr() != model_a.theta.data_ptr() and np.array_equal(_bits(A.ema), _bits(model_a.theta))
        early = []
        inner = A._apply_slice
        A._apply_slice = lambda i, tick, on, after=(), max_blocks=0: (early.append(max_blocks), inner(i, tick, on, after, max_blocks))[1]
        r = dict(theta=[_bits(model_a.theta).view(np.float32)], ema=[_bits(A.ema).view(np.float32)], losses_a=[], losses_b=[])
        for inputs, noise in _batches(hp, n_latents=n_latents):
            out = A.step(inputs, noise)
            r["losses_a"].append(_bits(out.raw["losses"]))
            r["theta"].append(_bits(model_a.theta).view(np.float32))
            r["ema"].append(_bits(A.ema).view(np.float32))
            out = B.step(inputs, noise)
            r["losses_b"].append(_bits(out.raw["losses"]))
        r.update(a=_state(A), b=_state(B), updates=A.ema_updates, early_slices=sum(1 for b in early if b > 0), n_ranges=len(A._ranges))
        _RUNS[variant] = r
    return _RUNS[variant]


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_the_average_only_reads(variant):
    r = _run(variant)
    if variant == "tree":
        assert r["n_ranges"] > 1 and r["early_slices"] > 0, "the default trainer of `tiny` applies early optimizer slices"
    if variant == "tree_clip":
        assert r["early_slices"] == 0                      # the whole-vector path
    for k in ("theta", "m", "v", "state"):
        assert np.array_equal(r["a"][k], r["b"][k]), f"{variant}: {k} differs between the averaging and the plain trainer"
    for i, (la, lb) in enumerate(zip(r["losses_a"], r["losses_b"])):
        assert np.array_equal(la, lb), f"{variant}: loss vector of step {i} differs"
    assert float(r["a"]["state"].view(np.float32)[0]) == STEPS


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_the_average_follows_the_recurrence(variant):
    r = _run(variant)
    assert r["updates"] == STEPS
    ref = r["theta"][0].astype(np.float64)                  # the average starts as a copy of theta
    budget = np.zeros_like(ref)
    worst = 0.0
    for k in range(STEPS):
        decay = E.warmup_decay(DECAY, k)
        theta_k = r["theta"][k + 1]
        assert not np.array_equal(theta_k, r["theta"][k])
        worst = max(worst, E.check_update(r["ema"][k + 1], r["ema"][k], theta_k, decay, f"{variant} step {k}"))
        ref, b = E.ref_update(ref, theta_k, decay)
        budget += b
    err = np.abs(r["ema"][STEPS].astype(np.float64) - ref)
    bad = ~(err <= budget)
    print(f"{variant}: worst per-step err / bound = {worst:.3g}; summed: worst err / budget = "
          f"{float((err[budget > 0] / budget[budget > 0]).max()):.3g}")
    assert not bad.any(), f"{variant}: {int(bad.sum())} elements outside the summed bounds; first at {int(np.flatnonzero(bad)[0])}"
    assert [E.warmup_decay(DECAY, k) for k in range(STEPS)] == [0.1, 2 / 11, 3 / 12, 4 / 13]
    # the last update read the step's final theta: an average built from the theta of one step earlier is far outside the bound
    stale, b = E.ref_update(r["ema"][STEPS - 1], r["theta"][STEPS - 1], E.warmup_decay(DECAY, STEPS - 1))
    assert (np.abs(r["ema"][STEPS].astype(np.float64) - stale) > 100 * b).any()


def _poisoned(batch):
    inputs, noise = batch
    bad = {k: v.clone() for k, v in inputs.items()}
    bad["traj_seq"][0, 0, 0, 0, 0] = float("nan")
    return bad, noise


def test_a_skipped_step_leaves_every_bit_of_the_average():
    hp, model, A = _tree(lr=1e-3, ema_decay=DECAY, nan_guard="skip")
    b = _batches(hp, 3)
    start = _bits(A.ema)
    A.step(*b[0])
    after1, theta1 = _bits(A.ema), _bits(model.theta)
    assert not np.array_equal(after1, start)
    A.step(*_poisoned(b[1]))
    assert np.array_equal(_bits(A.ema), after1), "the dropped step moved the average"
    assert np.array_equal(_bits(model.theta), theta1) and float(A.opt_state[3]) == 1.0
    assert A.ema_updates == 2                               # issued updates: the host does not read the gate
    A.step(*b[2])
    after3 = _bits(A.ema)
    assert not np.array_equal(after3, after1) and float(A.opt_state[3]) == 0.0 and A.ema_updates == 3
    # ... with the decay of update 2, from where update 0 left it
    E.check_update(after3.view(np.float32), after1.view(np.float32), _bits(model.theta).view(np.float32), E.warmup_decay(DECAY, 2), "step 3")
    assert np.isfinite(after3.view(np.float32)).all()


def test_the_average_moves_on_the_last_micro_step_only():
    hp, model, A = _tree(lr=1e-3, ema_decay=DECAY, accumulate=2)
    b = _batches(hp, 2)
    start = _bits(A.ema)
    A.step(*b[0])
    assert not A.stepped and A.ema_updates == 0 and np.array_equal(_bits(A.ema), start), "micro-step 1 moved the average"
    A.step(*b[1])
    assert A.stepped and A.ema_updates == 1
    after = _bits(A.ema)
    assert not np.array_equal(after, start)
    E.check_update(after.view(np.float32), start.view(np.float32), _bits(model.theta).view(np.float32), E.warmup_decay(DECAY, 0), "cycle")


def _packed(model):
    out = {"arena": _bits(model._arena)}
    for name, d in model.pk_split.items():
        out["split." + name] = d["out"].cpu().numpy().copy()
        out["log2." + name] = d["log2"].cpu().numpy().copy()
    for i, (ws, es) in enumerate(model._gsplit.values()):             # the row GEMMs' split-f16 twins the trainer keeps live
        out[f"gsplit.{i}"] = ws.cpu().numpy().copy()
        out[f"gsplit_log2.{i}"] = es.cpu().numpy().copy()
    return out


def _eval_forward(model, inputs, noise):
    model.eval()
    try:
        with model.val_mode(pred_length=False):
            out = model(inputs, "test", noise=noise)
            torch.cuda.synchronize()
            return out.tree.bf.images.detach().cpu().numpy().copy()
    finally:
        model.train()


def test_ema_weights_context():
    hp, model, A = _tree(lr=1e-3, ema_decay=DECAY)
    b = _batches(hp, 4)
    for inputs, noise in b[:3]:
        A.step(inputs, noise)
    theta0, ema0, packed0 = _bits(model.theta), _bits(A.ema), _packed(model)
    assert not np.array_equal(theta0, ema0)
    addr = (model.theta.data_ptr(), A.ema.data_ptr(), model._arena.data_ptr())
    plain = _eval_forward(model, *b[3])
    st = A.ema_state()
    assert set(st) == {"decay", "warmup", "updates", "state_dict"} and (st["decay"], st["warmup"], st["updates"]) == (DECAY, True, 3)
    assert set(st["state_dict"]) == set(model.state_dict())
    assert all(st["state_dict"][k].shape == v.shape and not st["state_dict"][k].is_cuda for k, v in model.state_dict().items())

    with A.ema_weights():
        assert np.array_equal(_bits(model.theta), ema0) and np.array_equal(_bits(A.ema), theta0)
        assert not np.array_equal(_packed(model)["arena"], packed0["arena"])
        inside = _eval_forward(model, *b[3])
        with pytest.raises(RuntimeError):
            A.step(*b[3])
        with pytest.raises(RuntimeError):
            A.backward(*b[3])
        with pytest.raises(RuntimeError):
            with A.ema_weights():
                pass

    def assert_restored(what):
        assert np.array_equal(_bits(model.theta), theta0) and np.array_equal(_bits(A.ema), ema0), what + ": theta / ema"
        now = _packed(model)
        assert set(now) == set(packed0)
        for k in now:
            assert np.array_equal(now[k], packed0[k]), f"{what}: packed buffer {k}"
        assert (model.theta.data_ptr(), A.ema.data_ptr(), model._arena.data_ptr()) == addr
    assert_restored("after exit")
    assert np.array_equal(_eval_forward(model, *b[3]), plain)
    assert not np.array_equal(inside, plain)

    class Boom(Exception):
        pass
    with pytest.raises(Boom):
        with A.ema_weights():
            assert np.array_equal(_bits(model.theta), ema0)
            raise Boom()
    assert_restored("after a raising body")
    assert not A._ema_swapped

    # a fresh model (with a trainer of its own: the same launch plans) loaded from ema_state()
    _, fresh, _ = _tree(lr=1e-3)
    fresh.load_state_dict(st["state_dict"])
    for k, (o, shp) in model._poff.items():
        n = int(np.prod(shp, dtype=np.int64))
        assert np.array_equal(_bits(fresh.theta[o:o + n]), ema0[o:o + n]), k
    assert np.array_equal(_eval_forward(fresh, *b[3]), inside), "the forward inside ema_weights() is not the averaged weights' forward"
    # training goes on where it was
    A.step(*b[3])
    assert A.ema_updates == 4
    _, _, plain_tr = _tree(lr=1e-3)
    with pytest.raises(ValueError):
        with plain_tr.ema_weights():
            pass
    with pytest.raises(ValueError):
        plain_tr.ema_state()


def test_resume_continues_the_average_bit_for_bit(tmp_path):
    from video_gcp_amd import checkpoint as CK
    hp, model, A = _tree(lr=1e-3, ema_decay=DECAY)
    b = _batches(hp, 3)
    A.step(*b[0])
    A.step(*b[1])
    saved_ema = _bits(A.ema)
    with_ema = CK.save_checkpoint(model, str(tmp_path / "a"), 0, 2, A.optimizer_state(), ema_state=A.ema_state())
    plain = CK.save_checkpoint(model, str(tmp_path / "b"), 0, 2, A.optimizer_state())
    A.step(*b[2])
    want_theta, want_ema = _bits(model.theta), _bits(A.ema)

    _, model_b, B = _tree(lr=1e-3, ema_decay=DECAY)
    _, _, opt = CK.load_weights(with_ema, model_b)
    B.load_optimizer_state(opt)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        B.load_ema_state(CK.read_ema_state(with_ema))
    assert B.ema_updates == 2 and np.array_equal(_bits(B.ema), saved_ema)
    B.step(*b[2])
    assert B.ema_updates == 3
    assert np.array_equal(_bits(model_b.theta), want_theta), "theta after the resumed step"
    assert np.array_equal(_bits(B.ema), want_ema), "the average after the resumed step"
    # the averaged weights load into a model like any weights
    CK.load_weights(with_ema, model_b, use_ema=True)
    for k, (o, shp) in model_b._poff.items():
        n = int(np.prod(shp, dtype=np.int64))
        assert np.array_equal(_bits(model_b.theta[o:o + n]), saved_ema[o:o + n]), k
    # a checkpoint without an average: warns, starts from the loaded weights
    CK.load_weights(plain, model_b)
    assert CK.read_ema_state(plain) is None
    with pytest.warns(UserWarning, match="no weight average"):
        B.load_ema_state(CK.read_ema_state(plain))
    assert B.ema_updates == 0 and np.array_equal(_bits(B.ema), _bits(model_b.theta))
    with pytest.raises(ValueError):
        CK.load_weights(plain, model_b, use_ema=True)


def test_train_entry_point(tmp_path, capsys):
    from video_gcp_amd.train import ModelTrainer, get_cmd_args
    exp = str(tmp_path / "exp")
    argv = ["--path", exp, "--config", "tiny", "--feed_random_data", "1", "--num_epochs", "1", "--batches_per_epoch", "5",
            "--log_outputs_interval", "1", "--skip_first_val", "1"]
    tr = ModelTrainer(get_cmd_args(argv + ["--ema_decay", "0.9"]))
    assert torch.is_tensor(tr.trainer.ema) and tr.trainer.ema_decay == 0.9 and tr.trainer.ema_warmup and tr.eval_ema
    seen = []
    inner = tr._val
    tr._val = lambda: (seen.append((tr.trainer._ema_swapped, _bits(tr.model.theta))), inner())[1]
    tr.run()
    assert tr.global_step == 5 and tr.trainer.ema_updates == 5 and np.isfinite(tr.last_val) and not tr.trainer._ema_swapped
    ema = _bits(tr.trainer.ema)
    assert len(seen) == 1 and seen[0][0] and np.array_equal(seen[0][1], ema), "validation did not run on the averaged weights"
    assert not np.array_equal(_bits(tr.model.theta), ema)
    ck = torch.load(os.path.join(exp, "weights", "weights_ep0.pth"), map_location="cpu")
    assert set(ck) == {"epoch", "global_step", "state_dict", "optimizer", "ema"}
    assert (ck["ema"]["decay"], ck["ema"]["warmup"], ck["ema"]["updates"]) == (0.9, True, 5)
    # --eval_ema 0: validation on the weights themselves
    tr.eval_ema = False
    seen.clear()
    tr.val()
    assert len(seen) == 1 and not seen[0][0] and np.array_equal(seen[0][1], _bits(tr.model.theta))
    # resume with an average: restored
    tr2 = ModelTrainer(get_cmd_args(argv + ["--ema_decay", "0.9", "--resume", "latest"]))
    assert tr2.resume("latest") == 1
    assert tr2.trainer.ema_updates == 5 and np.array_equal(_bits(tr2.trainer.ema), ema)
    assert np.array_equal(_bits(tr2.model.theta), _bits(tr.model.theta))
    # --metric on that checkpoint with --ema_decay 0: the trainer as it always was (no average), the averaged weights in the model;
    # with --eval_ema 0 the weights themselves
    tr3 = ModelTrainer(get_cmd_args(argv + ["--ema_decay", "0", "--metric", "1", "--resume", "latest", "--dont_save", "1"]))
    assert tr3.trainer.ema is None and tr3.trainer.ema_decay is None
    tr3.resume("latest")
    assert tr3._ema_loaded
    for k, (o, shp) in tr3.model._poff.items():
        n = int(np.prod(shp, dtype=np.int64))
        assert np.array_equal(_bits(tr3.model.theta[o:o + n]), ema[o:o + n]), k
    tr3.eval_ema, tr3._ema_loaded = False, False
    tr3.resume("latest")
    assert not tr3._ema_loaded and np.array_equal(_bits(tr3.model.theta), _bits(tr.model.theta))
