"""The training guard on the GPU (video_gcp_amd/health.py, csrc/train_stats.hip, csrc/scalar_f32.hip):
  * gcpx_grad_health against its numpy restatement, exactly: every path of the chunk kernel (16-byte loads, the len % 4 tail, single
    loads of unaligned segments, full and partial chunks, chunk seams), NaN-filled gaps, the gate, the running count, extra scalars;
  * the gate in every optimizer entry point: closed, nothing moves; open, the step is applied;
  * GCPTrainStep(nan_guard=...) on clean steps equals the trainer without a guard bit for bit;
  * a planted +Inf: "raise" raises and names the parameter with everything untouched, "skip" goes on, no guard poisons theta;
  * the gate does not travel through optimizer_state() / load_optimizer_state();
  * train.py --nan_guard raise / skip end to end, the weight check in front of save_checkpoint, and the sequential model."""
import json
import os

import numpy as np
import pytest
import torch

from helpers import make_inputs

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

NAN_BITS = (0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF)
POS_INF, NEG_INF = 0x7F800000, 0xFF800000
FINITE_EDGE = (0x7F7FFFFF, 0xFF7FFFFF, 0x00000001, 0x807FFFFF, 0x80000000, 0x00800000)
LENGTHS = [1, 3, 4, 5, 255, 256, 257, 16383, 16384, 16385, 32775]


def _synthetic():
    """every length twice -- on a 16-byte boundary, and 1, 2 or 3 floats off it -- with NaN in every gap; (bits, poff)"""
    rng = np.random.default_rng(11)
    poff, off = {}, 4
    for rep in range(2):
        for i, n in enumerate(LENGTHS):
            start = off + (0 if rep == 0 else 1 + i % 3)
            poff[f"s{rep}_{n}.weight"] = (start, (n,))
            off = (start + n + 3) // 4 * 4 + 4 * (1 + i % 2)
    bits = np.full(off + 4, 0x7FC00000, np.uint32)
    for name, (start, (n,)) in poff.items():
        v = (rng.standard_normal(n) * 10.0 ** rng.integers(-30, 30, n)).astype(np.float32).view(np.uint32)
        v[rng.integers(0, n, max(1, n // 16))] = rng.choice(np.array(FINITE_EDGE, np.uint32), max(1, n // 16))
        bits[start:start + n] = v
    return bits, poff


def _plant(bits, poff):
    """NaN / +Inf / -Inf at every segment's first and last element, on both sides of every chunk seam and in the len % 4 tail"""
    kinds = [POS_INF, NEG_INF] + list(NAN_BITS)
    k = 0
    bad = bits.copy()
    for name, (start, (n,)) in poff.items():
        spots = {0, n - 1}
        spots |= {e for seam in range(16384, n, 16384) for e in (seam - 1, seam)}
        spots |= set(range(n - n % 4, n))
        for e in sorted(spots):
            bad[start + e] = kinds[k % len(kinds)]
            k += 1
    return bad


def _health(lib, x, chunks, seg0, extra=None, summary=None, gate=None, partial=None):
    from video_gcp_amd import runtime as rt
    ch = torch.from_numpy(chunks.view(np.uint8).copy()).cuda()
    s0 = torch.from_numpy(seg0).cuda()
    n_seg = len(seg0) - 1
    partial = torch.full((3 * len(chunks),), -7, dtype=torch.int32, device="cuda") if partial is None else partial
    seg_bad = torch.full((n_seg, 3), -7, dtype=torch.int32, device="cuda")
    summary = torch.zeros(8, dtype=torch.int32, device="cuda") if summary is None else summary
    rt.check(lib.gcpx_grad_health(x.data_ptr(), x.numel(), ch.data_ptr(), len(chunks), s0.data_ptr(), n_seg, rt.ptr(extra),
                                  0 if extra is None else extra.numel(), partial.data_ptr(), partial.numel(), seg_bad.data_ptr(),
                                  summary.data_ptr(), rt.ptr(gate), torch.cuda.current_stream().cuda_stream), "grad_health")
    torch.cuda.synchronize()
    return seg_bad.cpu().numpy(), summary.cpu().numpy()


def test_health_kernel_equals_its_numpy_mirror(gcpx_lib):
    from video_gcp_amd import health as H
    from video_gcp_amd import scalar_log as SL
    bits, poff = _synthetic()
    names, chunks, seg0 = SL.grad_tables(poff)
    assert len(names) == 2 * len(LENGTHS) and any(c["first"] % 4 for c in chunks) and len(chunks) == 2 * (len(LENGTHS) + 1 + 2)
    clean = torch.from_numpy(bits.view(np.float32).copy()).cuda()
    gate = torch.full((1,), 7.0, device="cuda")
    summary = torch.zeros(8, dtype=torch.int32, device="cuda")
    # clean: the NaN of the gaps is read by nobody
    seg_bad, s = _health(gcpx_lib, clean, chunks, seg0, summary=summary, gate=gate)
    m_bad, m_s = H.health_numpy(bits.view(np.float32), chunks, seg0)
    assert not seg_bad.any() and s.tolist() == [0, 0, 0, 0, -1, 0, 0, 0] and float(gate) == 0.0
    assert np.array_equal(seg_bad, m_bad) and np.array_equal(s, m_s)
    # planted
    bad_bits = _plant(bits, poff)
    bad = torch.from_numpy(bad_bits.view(np.float32).copy()).cuda()
    assert np.array_equal(bad.cpu().numpy().view(np.uint32), bad_bits)          # payloads survive the upload
    seg_bad, s = _health(gcpx_lib, bad, chunks, seg0, summary=summary, gate=gate)
    m_bad, m_s = H.health_numpy(bad_bits.view(np.float32), chunks, seg0)
    print("planted:", s.tolist())
    assert np.array_equal(seg_bad, m_bad) and np.array_equal(s, m_s) and float(gate) == 1.0
    assert (seg_bad.sum(axis=1) > 0).all() and s[3] == len(names) and s[4] == 0 and s[6] == 1 and s[7] == 1
    assert min(s[0], s[1], s[2]) > 0 and s[:3].sum() == seg_bad.sum()
    # the same bits on a second call (and the count goes on); a clean call re-opens the gate and leaves the count
    seg_bad2, s2 = _health(gcpx_lib, bad, chunks, seg0, summary=summary, gate=gate)
    assert np.array_equal(seg_bad2, seg_bad) and s2[:7].tolist() == s[:7].tolist() and s2[7] == 2
    _, s3 = _health(gcpx_lib, clean, chunks, seg0, summary=summary, gate=gate)
    assert s3.tolist() == [0, 0, 0, 0, -1, 0, 0, 2] and float(gate) == 0.0
    # one bad element in one segment: first bad is that segment, the others stay clean
    one = clean.clone()
    o = poff["s1_16385.weight"][0]
    one[o + 16384] = float("-inf")
    seg_bad, s = _health(gcpx_lib, one, chunks, seg0)
    idx = names.index("s1_16385.weight")
    assert s.tolist() == [0, 0, 1, 1, idx, 0, 1, 1] and seg_bad[idx].tolist() == [0, 0, 1] and seg_bad.sum() == 1
    # a non-finite extra scalar alone sets the verdict; finite edge values do not
    for vals, n_bad in (([1.0, float("nan"), 2.0], 1), ([float("inf"), float("-inf")], 2), ([3.4028234663852886e38, -0.0, 1e-45], 0)):
        extra = torch.tensor(vals, device="cuda")
        seg_bad, s = _health(gcpx_lib, clean, chunks, seg0, extra=extra, gate=gate)
        m_bad, m_s = H.health_numpy(bits.view(np.float32), chunks, seg0, extra=np.float32(vals))
        assert not seg_bad.any() and s.tolist() == [0, 0, 0, 0, -1, n_bad, int(n_bad > 0), int(n_bad > 0)] and np.array_equal(s, m_s)
        assert float(gate) == float(n_bad > 0)
    # a chunk that leaves the vector is skipped, not read
    off_end = chunks.copy()
    off_end["first"][-1] = bad.numel() - 4
    seg_bad, _ = _health(gcpx_lib, bad, off_end, seg0)
    full = H.health_numpy(bad_bits.view(np.float32), chunks, seg0)[0]
    assert np.array_equal(seg_bad, H.health_numpy(bad_bits.view(np.float32), off_end, seg0)[0])
    assert np.array_equal(seg_bad[:-1], full[:-1]) and seg_bad[-1].sum() < full[-1].sum()
    # invalid arguments: -1, a text, no launch
    st = torch.cuda.current_stream().cuda_stream
    assert gcpx_lib.gcpx_grad_health(None, 0, None, 0, None, 0, None, 0, None, 0, None, None, None, st) == -1
    assert b"gcpx_grad_health" in gcpx_lib.gcpx_last_error()
    small = torch.zeros(3, dtype=torch.int32, device="cuda")
    ch, s0 = torch.from_numpy(chunks.view(np.uint8).copy()).cuda(), torch.from_numpy(seg0).cuda()
    assert gcpx_lib.gcpx_grad_health(bad.data_ptr(), bad.numel(), ch.data_ptr(), len(chunks), s0.data_ptr(), len(names), None, 0,
                                     small.data_ptr(), small.numel(), summary.data_ptr(), summary.data_ptr(), None, st) == -1


OPT_CALLS = [("radam_step", 0, 1), ("optim_step", 1, 1), ("optim_step", 2, 1), ("optim_step", 3, 1)] + \
            [("optim_range", kind, tick) for kind in range(4) for tick in (0, 1)]


@pytest.mark.parametrize("aligned", [True, False])
def test_closed_gate_stops_every_optimizer_entry_point(gcpx_lib, aligned):
    from video_gcp_amd import runtime as rt
    lib, st = gcpx_lib, torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(3)
    n, skip = (1027, 0) if aligned else (1026, 1)                  # 16-byte loads + a scalar tail / a slice one float off the boundary
    for what, kind, tick in OPT_CALLS:
        theta, grad = torch.randn(1027, generator=g).cuda(), (torch.randn(1027, generator=g) * 0.1).cuda()
        m, v = (torch.randn(1027, generator=g) * 0.01).cuda(), (torch.rand(1027, generator=g) * 0.01).cuda()
        p1, p2 = (0.9, 0.999) if kind <= 1 else ((0.9, 0.99) if kind == 2 else (0.9, 0.0))

        def call(state):
            ptrs = [t.data_ptr() + 4 * skip for t in (theta, grad, m, v)]
            if what == "radam_step":
                rt.check(lib.gcpx_radam_step(*ptrs, state.data_ptr(), n, 1e-2, p1, p2, 1e-8, 0.5, st), what)
            elif what == "optim_step":
                rt.check(lib.gcpx_optim_step(*ptrs, state.data_ptr(), n, kind, 1e-2, p1, p2, 1e-8, 0.5, st), what)
            else:
                rt.check(lib.gcpx_optim_range(*ptrs, state.data_ptr(), n, kind, 1e-2, p1, p2, 1e-8, 0.5, tick, 0, st), what)
            torch.cuda.synchronize()
        before = [t.clone() for t in (theta, m, v)]
        closed = torch.tensor([2.0, 0.0, 0.0, 1.0], device="cuda")
        call(closed)
        assert closed.tolist() == [2.0, 0.0, 0.0, 1.0], (what, kind, tick)
        for t, b, nm in zip((theta, m, v), before, ("theta", "m", "v")):
            assert torch.equal(t.view(torch.int32), b.view(torch.int32)), (what, kind, tick, nm)
        opened = torch.tensor([2.0, 0.0, 0.0, 0.0], device="cuda")
        call(opened)
        assert opened.tolist() == [3.0 if tick else 2.0, 0.0, 0.0, 0.0], (what, kind, tick)
        changed = theta[skip:skip + n] != before[0][skip:skip + n]
        # (an update of lr * 0.05 |N(0, 1)| stays below half an ulp of a weight of order 1 for |N| < ~1e-4: about one element in 10^4)
        assert float(changed.float().mean()) > 0.99, (what, kind, tick)
        if skip:
            assert torch.equal(theta[:skip], before[0][:skip])


def _tree_trainer(nan_guard, graph=True):
    import video_gcp_amd as V
    from video_gcp_amd.model import GCPTreeModel
    from video_gcp_amd.training import GCPTrainStep
    hp = V.config("c1")
    model = GCPTreeModel(hp, params=V.init_params(hp, seed=1, randomize_affine=True), device="cuda")
    model.use_graph = graph
    kw = {"nan_guard": nan_guard} if nan_guard else {}
    return hp, model, GCPTrainStep(model, lr=1e-3, **kw)


def _batch(hp, seed):
    inputs, noise, _ = make_inputs(hp, seed=seed, variant="B")
    return {k: v.cuda() for k, v in inputs.items()}, noise.cuda()


def _state(model, tr):
    torch.cuda.synchronize()
    return [t.clone() for t in (model.theta, tr.exp_avg, tr.exp_avg_sq, tr.opt_state, model._arena)]


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def test_clean_steps_under_a_guard_equal_the_unguarded_trainer():
    hp, m0, t0 = _tree_trainer(None)
    runs = [(m0, t0)] + [_tree_trainer(g)[1:] for g in ("raise", "skip")]
    for step in range(2):
        dev_in, noise = _batch(hp, 60 + step)
        for m, t in runs:
            t.step(dev_in, noise)
    ref = _state(m0, t0)
    assert float(t0.opt_state[0]) == 2.0
    for (m, t), g in zip(runs[1:], ("raise", "skip")):
        got = _state(m, t)
        for x, y, what in zip(ref, got, ("theta", "exp_avg", "exp_avg_sq", "opt_state", "packed weights")):
            assert torch.equal(x, y), (g, what)
        h = t.health()
        assert h.summary.tolist() == [0, 0, 0, 0, -1, 0, 0, 0] and not bool(h.seg_bad.any()) and len(h.names) == h.seg_bad.shape[0]
    with pytest.raises(ValueError):
        t0.health()
    with pytest.raises(ValueError):
        _tree_trainer("abort")


def _planted_parameter(model):
    names = [k for k, (o, shp) in model._poff.items() if k.endswith(".weight") and len(shp) >= 2]
    return names[len(names) // 2]


def test_planted_inf_raise_skip_and_no_guard():
    from video_gcp_amd.health import NonFiniteGradients
    from video_gcp_amd.scalar_log import BUFFER_SUFFIXES
    for guard in ("raise", "skip", None):
        hp, model, tr = _tree_trainer(guard)
        name = _planted_parameter(model)
        off, shp = model._poff[name]
        dev_in, noise = _batch(hp, 70)
        tr.step(dev_in, noise)                                       # a clean step first: the moments and the counter are not zero
        params0 = {k: v.clone() for k, v in model.state_dict().items() if not k.endswith(BUFFER_SUFFIXES)}
        dev_in, noise = _batch(hp, 71)
        out = tr.backward(dev_in, noise)
        tr.grad[off + 2] = float("inf")
        before = _state(model, tr)                                   # (behind the forward: it has updated the BatchNorm statistics)
        assert float(before[3][0]) == 1.0
        if guard == "raise":
            with pytest.raises(NonFiniteGradients) as ei:
                tr.optimizer_step(out)
            e = ei.value
            assert e.bad == [(name, 0, 1, 0)] and name not in e.ok and len(e.ok) == len(tr.health().names) - 1
            assert e.loss_nonfinite == 0 and e.outputs is out and str(e) == "there are NaN Gradients"
        else:
            tr.optimizer_step(out)
        after = _state(model, tr)
        if guard is None:
            # the test tells the cases apart: without a guard the +Inf goes through the optimizer into the weights
            assert not bool(torch.isfinite(model.theta[off:off + int(np.prod(shp))]).all())
            assert float(after[3][0]) == 2.0
            continue
        for x, y, what in zip(before[:3] + before[4:], after[:3] + after[4:], ("theta", "exp_avg", "exp_avg_sq", "packed weights")):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), (guard, what)
        assert after[3].tolist() == [1.0, 0.0, 0.0, 1.0], guard       # the counter has not ticked, the gate is closed
        for k, v in model.state_dict().items():
            if k in params0:
                assert torch.equal(v, params0[k]), (guard, k)
        h = tr.health()
        assert h.summary.tolist() == [0, 1, 0, 1, h.names.index(name), 0, 1, 1]
        assert h.seg_bad[h.names.index(name)].tolist() == [0, 1, 0] and int(h.seg_bad.sum()) == 1
        # the next clean step is applied and re-opens the gate
        dev_in, noise = _batch(hp, 72)
        tr.step(dev_in, noise)
        torch.cuda.synchronize()
        assert tr.opt_state.tolist() == [2.0, 0.0, 0.0, 0.0] and bool(torch.isfinite(model.theta).all())
        # applied: theta moves.  (How MANY elements move is not a property of the guard: an update below
        # half an ulp of its weight -- lr * m with a gradient under ~1e-6 -- leaves that weight's bits, and most of c1's are that small.)
        assert bool((model.theta != after[0]).any())
        assert tr.health().summary.tolist() == [0, 0, 0, 0, -1, 0, 0, 1]


def test_a_non_finite_loss_alone_closes_the_gate():
    hp, model, tr = _tree_trainer("skip")
    dev_in, noise = _batch(hp, 73)
    out = tr.backward(dev_in, noise)
    out.raw["losses"][5] = float("nan")                              # base_gcp.py:302-303: the total
    before = _state(model, tr)
    tr.optimizer_step(out)
    after = _state(model, tr)
    assert _same(before[:3], after[:3]) and after[3].tolist() == [0.0, 0.0, 0.0, 1.0]
    assert tr.health().summary.tolist() == [0, 0, 0, 0, -1, 1, 1, 1]


def test_the_gate_does_not_outlive_its_run():
    hp, model, tr = _tree_trainer("skip")
    dev_in, noise = _batch(hp, 74)
    out = tr.backward(dev_in, noise)
    tr.grad[model._poff[_planted_parameter(model)][0]] = float("nan")
    tr.optimizer_step(out)
    torch.cuda.synchronize()
    assert float(tr.opt_state[3]) == 1.0
    st = tr.optimizer_state()
    assert st["state"].tolist() == [0.0, 0.0, 0.0, 0.0] and float(tr.opt_state[3]) == 1.0      # stored open; the trainer's own is untouched
    st["state"][3] = 1.0                                             # ... and a checkpoint that does hold a closed gate
    _, m2, t2 = _tree_trainer(None)
    t2.load_optimizer_state(st)
    torch.cuda.synchronize()
    assert float(t2.opt_state[3]) == 0.0
    theta0 = m2.theta.clone()
    t2.step(dev_in, noise)
    torch.cuda.synchronize()
    assert float(t2.opt_state[0]) == 1.0 and bool((m2.theta != theta0).any())


def test_planted_fault_through_the_sequential_trainer():
    import video_gcp_amd as V
    from video_gcp_amd.health import NonFiniteGradients
    from video_gcp_amd.sequential import GCPSequentialModel
    from video_gcp_amd.training_sequential import SequentialTrainStep
    hp = V.config("c1", nz_mid_lstm=128, lstm_init="zero")
    model = GCPSequentialModel(hp, params=V.init_params_sequential(hp, seed=1, randomize_affine=True), device="cuda")
    tr = SequentialTrainStep(model, lr=1e-3, nan_guard="raise")
    inputs, noise, _ = make_inputs(hp, seed=7, variant="B")
    dev_in, noise = {k: v.cuda() for k, v in inputs.items()}, noise[:, :hp.max_seq_len - 1].contiguous().cuda()
    tr.step(dev_in, noise)
    torch.cuda.synchronize()
    assert tr.opt_state.tolist() == [1.0, 0.0, 0.0, 0.0]
    name = "dense_rec.lstm.cell.gen_lstm.out.weight"
    off, shp = model._poff[name]
    out = tr.backward(dev_in, noise)
    tr.grad[off + int(np.prod(shp)) - 1] = float("-inf")
    before = _state(model, tr)
    with pytest.raises(NonFiniteGradients) as ei:
        tr.optimizer_step(out)
    assert ei.value.bad == [(name, 0, 0, 1)]
    after = _state(model, tr)
    assert _same(before[:3] + before[4:], after[:3] + after[4:]) and after[3].tolist() == [1.0, 0.0, 0.0, 1.0]


def _model_trainer(tmp_path, monkeypatch, name, extra, plant_at=3, nan=float("nan")):
    from video_gcp_amd.model import GCPTreeModel
    from video_gcp_amd.train import ModelTrainer, get_cmd_args
    exp = tmp_path / name
    exp.mkdir()
    (exp / "conf.json").write_text(json.dumps({"config": "c1"}))
    argv = ["--path", str(exp), "--config", "c1", "--num_epochs", "1", "--batches_per_epoch", "5", "--log_outputs_interval", "2",
            "--deterministic", "1", "--skip_first_val", "1"] + extra
    monkeypatch.setattr(GCPTreeModel, "_n_models", 0)
    tr = ModelTrainer(get_cmd_args(argv))
    seen = {"name": _planted_parameter(tr.model)}
    backward = tr.trainer.backward

    def planting_backward(inputs, noise=None):
        if tr.global_step == plant_at:
            torch.cuda.synchronize()
            seen["params"] = {k: v.detach().cpu().clone() for k, v in tr.model.state_dict().items()}
            seen["inputs"] = {k: v.detach().cpu().clone() for k, v in inputs.items() if torch.is_tensor(v)}
        out = backward(inputs, noise)
        if tr.global_step == plant_at:
            tr.trainer.grad[tr.model._poff[seen["name"]][0] + 1] = nan
        return out
    tr.trainer.backward = planting_backward
    return tr, str(exp), seen


def test_trainer_raise_dumps_the_batch_and_an_untouched_checkpoint(tmp_path, monkeypatch):
    import video_gcp_amd as V
    from video_gcp_amd import checkpoint as CK
    from video_gcp_amd.health import NonFiniteGradients
    from video_gcp_amd.model import GCPTreeModel
    from video_gcp_amd.scalar_log import BUFFER_SUFFIXES
    tr, exp, seen = _model_trainer(tmp_path, monkeypatch, "raise", ["--nan_guard", "raise"])
    with pytest.raises(NonFiniteGradients) as ei:
        tr.run()
    assert tr.global_step == 3 and [b[0] for b in ei.value.bad] == [seen["name"]]
    d = np.load(os.path.join(exp, "nan_debug_info.npz"))
    assert d["bad_parameters"].tolist() == [seen["name"]] and d["bad_counts"].tolist() == [[1, 0, 0]]
    assert seen["name"] not in d["ok_parameters"].tolist() and len(d["ok_parameters"]) == len(tr.trainer.health().names) - 1
    assert int(d["global_step"]) == 3 and int(d["epoch"]) == 0
    for k, v in seen["inputs"].items():
        assert np.array_equal(d["inputs/" + k], v.numpy()), k
    assert np.array_equal(d["outputs/end_ind"], seen["inputs"]["end_ind"].numpy())
    assert np.isfinite(d["losses/total"]) and "losses/kl" in d.files and "losses/dense_img_rec" in d.files
    assert not os.path.exists(os.path.join(exp, "weights"))          # the run stopped before its epoch's checkpoint
    fresh = GCPTreeModel(tr.hp, params=V.init_params(tr.hp, seed=5), device="cuda")
    step, epoch, opt = CK.load_weights(os.path.join(exp, "nan_debug_ckpt.pth"), fresh)
    assert (step, epoch) == (3, 0) and opt["state"].tolist() == [3.0, 0.0, 0.0, 0.0]
    loaded = fresh.state_dict()
    n_par = 0
    for k, v in seen["params"].items():
        if not k.endswith(BUFFER_SUFFIXES):
            assert torch.equal(loaded[k].cpu(), v), k
            n_par += 1
    assert n_par > 100 and bool(torch.isfinite(fresh.theta).all()) and bool(torch.isfinite(opt["exp_avg_sq"]).all())
    # --dont_save: the same stop, no files
    tr2, exp2, _ = _model_trainer(tmp_path, monkeypatch, "raise_dont_save", ["--nan_guard", "raise", "--dont_save", "1"])
    with pytest.raises(NonFiniteGradients):
        tr2.run()
    assert os.listdir(exp2) == ["conf.json"]


def test_trainer_skip_goes_on_counts_and_guards_the_checkpoint(tmp_path, monkeypatch, capsys):
    from video_gcp_amd.health import NonFiniteWeights
    tr, exp, seen = _model_trainer(tmp_path, monkeypatch, "skip", ["--nan_guard", "skip", "--log_scalars", "1"], nan=float("inf"))
    tr.run()
    torch.cuda.synchronize()
    assert tr.global_step == 5 and bool(torch.isfinite(tr.model.theta).all())
    assert tr.trainer.opt_state.tolist() == [4.0, 0.0, 0.0, 0.0]       # five steps, four applied
    d = json.load(open(os.path.join(exp, "events", "scalar_data.json")))
    rows = d["gradients/skipped_steps_train"]
    assert [s for _, s, _ in rows] == [0, 2, 4] and [v for _, _, v in rows] == [0.0, 0.0, 1.0]
    assert os.listdir(os.path.join(exp, "weights")) == ["weights_ep0.pth"]
    assert "steps skipped for non-finite gradients: 1" in capsys.readouterr().out
    # non-finite running statistics in front of save_checkpoint: raises, and no new file
    name = [k for k in tr.model._poff if k.endswith(".running_var")][0]
    tr.model.theta[tr.model._poff[name][0]] = float("inf")
    with pytest.raises(NonFiniteWeights) as ei:
        tr.save_checkpoint(1)
    assert ei.value.bad == [(name, 0, 1, 0)] and os.listdir(os.path.join(exp, "weights")) == ["weights_ep0.pth"]
    # without the flag the trainer is built without a guard (what a planted value then does: test_planted_inf_raise_skip_and_no_guard)
    tr0, _, _ = _model_trainer(tmp_path, monkeypatch, "off", [])
    assert tr0.nan_guard is None and tr0.trainer.nan_guard is None and tr0.trainer._health is None
