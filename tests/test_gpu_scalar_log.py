"""Scalar logs on the GPU (video_gcp_amd/scalar_log.py, csrc/train_stats.hip):
  * gcpx_grad_segment_norms on a synthetic vector (odd lengths, one segment of 2^23 + 5 elements, NaN in every padding slot) against
    float64, within the bound its own summation shape gives, and bit-repeatable;
  * GCPTrainStep.gradient_stats() after a training step (c1, the sequential model, c1 with gradient clipping) against
    torch.norm(g.double()) over named_grads();
  * gcpx_kl_layerwise against float64 from out.tree.bf.q_z_* / p_z_*, with free_nats > 0 and with a level whose entries are all zero;
  * train.py --log_scalars 1 end to end, and the same run without the flag.
Every test runs under a time limit of its own."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch

from helpers import make_inputs
from test_scalar_log_cpu import float64_norms, read_event_file, synthetic_segments

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

U = 2.0 ** -24


def _norm_bound():
    from video_gcp_amd import scalar_log as SL
    # a thread adds at most S squares with one rounding each (fmaf), a tree of depth D adds the threads' sums: (S + D) u on the sum of
    # squares, half of it on its root; the chunks add in f64; root and scale in f64, rounded to f32 once: + u
    return 0.5 * (SL.GRAD_NORM_SERIAL + SL.GRAD_NORM_TREE_DEPTH + 2) * U


def _launch_norms(lib, g, chunks, seg0, scale=1.0, coef=None):
    from video_gcp_amd import runtime as rt
    ch = torch.from_numpy(chunks.view(np.uint8).copy()).cuda()
    s0 = torch.from_numpy(seg0).cuda()
    partial = torch.full((2 * len(chunks),), float("nan"), device="cuda")
    norm = torch.full((len(seg0) - 1,), float("nan"), device="cuda")
    stats = torch.full((4,), float("nan"), device="cuda")
    rt.check(lib.gcpx_grad_segment_norms(g.data_ptr(), g.numel(), ch.data_ptr(), len(chunks), s0.data_ptr(), len(seg0) - 1, scale,
                                         rt.ptr(coef), partial.data_ptr(), partial.numel(), norm.data_ptr(), stats.data_ptr(),
                                         torch.cuda.current_stream().cuda_stream), "grad_segment_norms")
    torch.cuda.synchronize()
    return norm.cpu().numpy(), stats.cpu().numpy(), partial.cpu().numpy()


def test_segment_norms_on_a_synthetic_vector(gcpx_lib):
    from video_gcp_amd import scalar_log as SL
    rng = np.random.default_rng(1)
    lengths = [1, 2, 3, 4, 5, 6, 7, 63, 1001, 16384, 16383, 16385, 2 ** 23 + 5, 9, 131075, 11]
    g_np, poff = synthetic_segments(rng, lengths, zero=(8,))
    names, chunks, seg0 = SL.grad_tables(poff)
    assert np.isnan(g_np).sum() >= len(lengths)                   # padding and the slots around the buffer hold NaN
    g = torch.from_numpy(g_np).cuda()
    norm, stats, partial = _launch_norms(gcpx_lib, g, chunks, seg0, scale=0.5)
    ref, counted = float64_norms(g_np, poff, names, 0.5)
    bound = _norm_bound()
    rel = np.abs(norm - ref) / np.maximum(ref, 1e-300)
    print(f"segment norms: max relative error {rel[counted].max():.3e}, bound {bound:.3e}; stats {stats}")
    assert not counted[8] and norm[8] == 0 and counted.sum() == len(lengths) - 1
    assert np.all(np.abs(norm - ref) <= bound * ref), (rel.max(), bound)
    mean, mx = ref[counted].mean(), ref[counted].max()
    assert abs(stats[0] - mean) <= 2 * bound * mean and abs(stats[1] - mx) <= bound * mx
    assert stats[2] == counted.sum() and stats[3] == 0
    # the numpy mirror differs from the kernel by its second rounding per element only
    m_norm, m_stats = SL.segment_norms_numpy(g_np, chunks, seg0, 0.5)
    assert np.all(np.abs(m_norm - norm) <= (bound + 0.5 * SL.GRAD_NORM_SERIAL * U) * 2 * ref) and np.array_equal(m_stats[2:], stats[2:])
    # bit-repeatable
    norm2, stats2, partial2 = _launch_norms(gcpx_lib, g, chunks, seg0, scale=0.5)
    assert np.array_equal(norm, norm2) and np.array_equal(stats, stats2) and np.array_equal(partial, partial2)
    # the clip coefficient: a device scalar, 0 = none; an inf poisons its own segment only and is counted
    coef = torch.tensor([0.25], device="cuda")
    norm_c, stats_c, _ = _launch_norms(gcpx_lib, g, chunks, seg0, scale=0.5, coef=coef)
    assert np.all(np.abs(norm_c - 0.25 * ref) <= bound * 0.25 * ref)
    norm_0, _, _ = _launch_norms(gcpx_lib, g, chunks, seg0, scale=0.5, coef=torch.zeros(1, device="cuda"))
    assert np.array_equal(norm_0, norm)
    # a negative slot = a coefficient of ZERO (gcpx_grad_clip_coef after an overflowed norm): the step applies no gradient, the log says 0
    norm_n, stats_n, _ = _launch_norms(gcpx_lib, g, chunks, seg0, scale=0.5, coef=torch.full((1,), -1.0, device="cuda"))
    assert np.all(norm_n == 0) and not np.signbit(norm_n).any() and stats_n[0] == 0 and stats_n[1] == 0 and stats_n[2] == stats[2]
    g[poff["p13.weight"][0] + 3] = float("inf")
    norm_i, stats_i, _ = _launch_norms(gcpx_lib, g, chunks, seg0, scale=0.5)
    keep = np.arange(len(lengths)) != 13
    assert np.isinf(norm_i[13]) and np.array_equal(norm_i[keep], norm[keep])
    assert stats_i[3] == 1 and stats_i[2] == stats[2] and np.isinf(stats_i[0]) and np.isinf(stats_i[1])
    # a chunk that leaves the vector is skipped, not read
    bad = chunks.copy()
    bad["first"][-1] = g.numel() - 4
    norm_b, _, _ = _launch_norms(gcpx_lib, g, bad, seg0, scale=0.5)
    assert norm_b[-1] == 0 and np.array_equal(norm_b[:-1], norm_i[:-1])


def _check_gradient_stats(tr, clip_coef=1.0):
    st = tr.gradient_stats()
    torch.cuda.synchronize()
    norm, stats = st.seg_norm.cpu().numpy(), st.stats.cpu().numpy()
    grads = tr.named_grads()
    assert st.names == [k for k in tr.m._poff if not k.endswith(("running_mean", "running_var"))]
    ref = np.array([float(torch.norm(grads[k].double())) * clip_coef for k in st.names])
    counted = np.array([bool((grads[k] != 0).any()) for k in st.names])
    bound = _norm_bound()
    print(f"gradient_stats: {counted.sum()} of {len(counted)} counted, max relative error "
          f"{(np.abs(norm - ref)[counted] / ref[counted]).max():.3e}, bound {bound:.3e}, stats {stats}")
    assert counted.sum() > 100 and np.isfinite(ref).all()
    assert np.all(np.abs(norm - ref) <= bound * ref)
    mean, mx = ref[counted].mean(), ref[counted].max()
    assert abs(stats[0] - mean) <= 2 * bound * mean and abs(stats[1] - mx) <= bound * mx
    assert stats[2] == counted.sum() and stats[3] == 0
    return st, counted


def test_gradient_stats_after_a_step_c1():
    from test_gpu_training import _setup
    hp, sd, model, tr = _setup("c1", False)
    inputs, noise, _ = make_inputs(hp, seed=7, variant="B")
    tr.step({k: v.cuda() for k, v in inputs.items()}, noise.cuda())
    st, counted = _check_gradient_stats(tr)
    # the stand-in for `p.grad is None`: with learn_matching_temp off (balanced binding) nothing writes binding.temp's gradient
    off = [k for k, c in zip(st.names, counted) if not c]
    print("not counted:", off)
    theta0 = model.theta.clone()
    tr.gradient_stats()                                            # reading changes nothing
    torch.cuda.synchronize()
    assert torch.equal(theta0, model.theta)


def test_gradient_stats_after_a_step_sequential():
    from test_gpu_sequential import _train_setup
    hp, sd, model, tr = _train_setup()
    inputs, noise, _ = make_inputs(hp, seed=7, variant="B")
    tr.step({k: v.cuda() for k, v in inputs.items()}, noise[:, :hp.max_seq_len - 1].contiguous().cuda())
    _check_gradient_stats(tr)


def test_gradient_stats_are_of_the_clipped_gradient():
    import video_gcp_amd as V
    from video_gcp_amd.model import GCPTreeModel
    from video_gcp_amd.training import GCPTrainStep
    hp = V.config("c1")
    model = GCPTreeModel(hp, params=V.init_params(hp, seed=1, randomize_affine=True), device="cuda")
    clip = 1e-3                                                # far below any gradient norm of this model: the step clips
    tr = GCPTrainStep(model, lr=1e-3, optimizer="adam", gradient_clip=clip)
    inputs, noise, _ = make_inputs(hp, seed=40, variant="B")
    tr.step({k: v.cuda() for k, v in inputs.items()}, noise.cuda())
    torch.cuda.synchronize()
    coef, total = float(tr.opt_state[1]), float(tr.opt_state[2])
    print(f"clip coefficient {coef}, global norm {total}")
    assert 0 < coef < 1 and abs(coef - clip / (total + 1e-6)) <= 1e-6 * coef          # this step clips
    st, counted = _check_gradient_stats(tr, clip_coef=coef)
    # clip_grad_norm_ leaves a global norm of max_norm: the clipped per-parameter norms add up to it
    glob = math.sqrt(float((st.seg_norm.double() ** 2).sum()))
    assert abs(glob - clip) <= 1e-4 * clip


def _kl_levels_float64(bf, free_nats, L):
    mq, lq, mp, lp = (getattr(bf, k).double().cpu() for k in ("q_z_mu", "q_z_log_sigma", "p_z_mu", "p_z_log_sigma"))
    ratio = (torch.exp(2 * lq) + (mq - mp) ** 2) / (2 * torch.exp(2 * lp))
    kl = torch.clamp(lp - lq + ratio - 0.5, min=free_nats)
    mag = lp.abs() + lq.abs() + ratio + 0.5                       # the terms one element is made of
    v, a = kl.mean(-1), mag.mean(-1)                              # [B, N] breadth-first
    res, tol = [], []
    nz = kl.shape[-1]
    for l in range(L):
        vl, al = v[:, 2 ** l - 1:2 ** (l + 1) - 1], a[:, 2 ** l - 1:2 ** (l + 1) - 1]
        keep = vl != 0
        res.append(float(vl[keep].mean()) if keep.any() else float("nan"))
        # an element: two exp (1 u each), the difference, its square, the sum, the quotient: <= 6 u on the ratio; three more sums at u of
        # their size: <= 9 u (|lp| + |lq| + ratio + 0.5).  A sum of n terms in any order: <= (n - 1) u sum |x| -- over nz, then the level
        n_l = int(keep.sum())
        tol.append(U * (9 * float(al.mean()) + (nz - 1 + max(n_l, 1) - 1 + 2) * float(vl.abs().mean())) if keep.any() else 0.0)
    return np.array(res), np.array(tol)


@pytest.mark.parametrize("free_nats", [0.0, 0.05])
def test_kl_layerwise_against_float64(gcpx_lib, free_nats):
    import video_gcp_amd as V
    from video_gcp_amd import runtime as rt
    from video_gcp_amd import scalar_log as SL
    from video_gcp_amd.model import GCPTreeModel
    hp = V.config("c1", free_nats=free_nats)
    model = GCPTreeModel(hp, params=V.init_params(hp, seed=1, randomize_affine=True), device="cuda")
    inputs, noise, _ = make_inputs(hp, seed=3, variant="B")
    out = model({k: v.cuda() for k, v in inputs.items()}, "train", noise=noise.cuda())
    L, nv = hp.hierarchy_levels, hp.nz_vae
    got = SL.kl_layerwise(model, out)
    torch.cuda.synchronize()
    ref, tol = _kl_levels_float64(out.tree.bf, free_nats, L)
    err = np.abs(got.cpu().numpy() - ref)
    print(f"kl_layerwise free_nats={free_nats}: {got.cpu().numpy()}, max err / tol {np.max(err / tol):.3f}")
    assert np.isfinite(ref).all() and np.all(err <= tol), (err, tol)
    # a level whose posterior equals its prior exactly: every entry is zero -> NaN (free_nats = 0); the floor otherwise
    QZ, PZ = out.raw["QZ"].clone(), out.raw["PZ"].clone()
    B, PS = QZ.shape[:2]
    lvl = 2
    pos = [1 + (2 * j + 1) * 2 ** (L - 1 - lvl) - 1 for j in range(2 ** lvl)]          # slot 1 + depth-first position
    QZ[:, pos] = PZ[:, pos]
    node_v, res = torch.empty(B * (2 ** L - 1), device="cuda"), torch.empty(L, device="cuda")
    rt.check(gcpx_lib.gcpx_kl_layerwise(QZ.data_ptr() + 8 * nv, PZ.data_ptr() + 8 * nv, B, L, nv, PS * 2 * nv, 2 * nv, free_nats,
                                        node_v.data_ptr(), res.data_ptr(), torch.cuda.current_stream().cuda_stream), "kl_layerwise")
    res2 = torch.empty_like(res)
    rt.check(gcpx_lib.gcpx_kl_layerwise(QZ.data_ptr() + 8 * nv, PZ.data_ptr() + 8 * nv, B, L, nv, PS * 2 * nv, 2 * nv, free_nats,
                                        node_v.data_ptr(), res2.data_ptr(), torch.cuda.current_stream().cuda_stream), "kl_layerwise")
    torch.cuda.synchronize()
    res, res2 = res.cpu().numpy(), res2.cpu().numpy()
    assert np.array_equal(res, res2, equal_nan=True)
    others = np.arange(L) != lvl
    assert np.array_equal(res[others], got.cpu().numpy()[others])
    if free_nats == 0:
        assert np.isnan(res[lvl])
    else:
        assert abs(res[lvl] - free_nats) <= 4 * U * free_nats
    # node_v is in depth-first order: the level of position p is L - 1 - ctz(p + 1)
    v = node_v.view(B, -1).cpu()
    lev = [L - 1 - (((p + 1) & -(p + 1)).bit_length() - 1) for p in range(2 ** L - 1)]
    for l in range(L):
        cols = [p for p in range(2 ** L - 1) if lev[p] == l]
        assert len(cols) == 2 ** l
        if free_nats == 0:
            assert bool((v[:, cols] == 0).all()) == (l == lvl) and bool((v[:, cols] != 0).all()) == (l != lvl)


def _run_trainer(tmp_path, monkeypatch, name, extra, conf=None, record=False):
    from video_gcp_amd.model import GCPTreeModel
    from video_gcp_amd.train import ModelTrainer, get_cmd_args
    exp = tmp_path / name
    exp.mkdir()
    (exp / "conf.json").write_text(json.dumps(conf or {"config": "c5s", "overrides": {"batch_size": 5}}))
    argv = ["--path", str(exp), "--num_epochs", "2", "--batches_per_epoch", "5", "--log_outputs_interval", "2", "--deterministic", "1"] + extra
    monkeypatch.setattr(GCPTreeModel, "_n_models", 0)          # the same noise stream for the runs compared (see test_gpu_image_log)
    tr = ModelTrainer(get_cmd_args(argv))
    seen = {}
    if record:                                                 # model.loss() of every training step, read right behind the step
        step = tr.trainer.step

        def recording_step(inputs, noise=None):
            out = step(inputs, noise)
            losses = tr.model.loss(inputs, out)
            seen[tr.global_step] = {k: float(v.value if isinstance(v, dict) else v) for k, v in losses.items()}
            return out
        tr.trainer.step = recording_step
    printed = []
    import builtins
    real_print = builtins.print
    monkeypatch.setattr(builtins, "print", lambda *a, **k: (printed.append(" ".join(str(x) for x in a)), real_print(*a, **k))[1])
    tr.run()
    monkeypatch.setattr(builtins, "print", real_print)
    return tr, str(exp), seen, printed


@pytest.mark.parametrize("kind", ["tree", "sequential"])
def test_trainer_logs_scalars_and_logging_does_not_disturb_the_run(tmp_path, monkeypatch, kind):
    conf = None if kind == "tree" else {"config": "c1", "model": "SequentialModel", "lr": 1e-3,
                                        "overrides": {"nz_mid_lstm": 128, "lstm_init": "zero", "batch_size": 5}}
    tr, exp, seen, printed = _run_trainer(tmp_path, monkeypatch, "with", ["--log_scalars", "1"], conf, record=True)
    ev_dir = os.path.join(exp, "events")
    files = sorted(os.listdir(ev_dir))
    assert len(files) == 2 and files[0].startswith("events.out.tfevents.") and files[1] == "scalar_data.json"
    d = json.load(open(os.path.join(ev_dir, "scalar_data.json")))
    events = read_event_file(os.path.join(ev_dir, files[0]))
    assert events[0]["file_version"] == "brain.Event:2" and len(events) == 1 + sum(len(r) for r in d.values())
    by_tag = {}
    for e in events[1:]:
        by_tag.setdefault(e["tag"], []).append((e["step"], e["value"]))
    for tag, rows in d.items():                                # the two sinks hold the same numbers (f32 in the event file)
        assert [s for _, s, _ in rows] == [s for s, _ in by_tag[tag]]
        assert np.array_equal(np.float32([v for _, _, v in rows]), np.float32([v for _, v in by_tag[tag]]), equal_nan=True)
    log_steps = [0, 2, 4, 6, 8]
    assert tr.global_step == 10 and [s for s, _ in tr.log] == log_steps
    # the loss terms of a logging step are model.loss() of that step, bit for bit; the total is trainer.log
    terms = [k for k in seen[0] if k != "_total"]
    assert {"dense_img_rec", "kl"} <= set(terms) and ("nll" in terms) == (kind == "tree")
    for k in terms:
        rows = d[f"{k}_loss_train"]
        assert [s for _, s, _ in rows] == log_steps
        assert [v for _, _, v in rows] == [seen[s][k] for s in log_steps], k
    assert [(s, v) for _, s, v in d["total_loss_train"]] == tr.log
    assert [v for _, v in tr.log] == [seen[s]["_total"] for s in log_steps]
    for tag in ("gradients/mean_norm_train", "gradients/max_norm_train", "gradients/nonfinite_train", "time/batch_train",
                "time/data_load_train"):
        assert [s for _, s, _ in d[tag]] == log_steps and all(math.isfinite(v) and v >= 0 for _, _, v in d[tag]), tag
    assert all(0 < m <= x for (_, _, m), (_, _, x) in zip(d["gradients/mean_norm_train"], d["gradients/max_norm_train"]))
    assert all(v == 0 for _, _, v in d["gradients/nonfinite_train"])
    # validation: before the first epoch and after each (steps 0, 5, 10): the averages, the total equal to the printed average
    val_steps = [0, 5, 10]
    for k in terms + ["total"]:
        assert [s for _, s, _ in d[f"{k}_loss_val"]] == val_steps, k
    assert d["total_loss_val"][-1][2] == tr.last_val
    shown = [float(p.split("Average loss: ")[1].split(" in")[0]) for p in printed if "Average loss" in p]
    assert shown == [float("{:.4f}".format(v)) for _, _, v in d["total_loss_val"]]
    L = tr.model._hp.hierarchy_levels
    layer_tags = [t for t in d if t.startswith("kl_loss_layerwise/")]
    if kind == "tree":
        assert sorted(layer_tags) == sorted(f"kl_loss_layerwise/level_{l}_{ph}" for l in range(L) for ph in ("train", "val"))
        assert all(math.isfinite(v) and v > 0 for t in layer_tags for _, _, v in d[t])
    else:
        assert not layer_tags
    # the same run without the flag: no directory, no logger, the same losses and weights bit for bit
    tr0, exp0, _, _ = _run_trainer(tmp_path, monkeypatch, "without", [], conf)
    assert not os.path.exists(os.path.join(exp0, "events")) and tr0.model.scalar_log is None and tr0.scalar_log is None
    assert tr.log == tr0.log and tr.last_val == tr0.last_val
    assert torch.equal(tr.model.theta, tr0.model.theta)
    # --dont_save: no logger either
    tr1, exp1, _, _ = _run_trainer(tmp_path, monkeypatch, "dont", ["--log_scalars", "1", "--dont_save", "1"], conf)
    assert not os.path.exists(os.path.join(exp1, "events")) and tr1.model.scalar_log is None
