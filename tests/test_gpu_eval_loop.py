"""-m gpu: prediction metrics in the trainer (gcp_builder.py:84-95, train.py:205-226, compute_metrics.py:89-226): the top-of-N
accumulation kernel against numpy, `--metric 1` on the fixture dataset against a direct Evaluator.eval and the oracle metrics, the
three pruning schemes, the flat model's binding (sequential.py:70-97) and `--skip_top100_val 0` during training."""
import json
import os

import numpy as np
import pytest
import torch

from helpers import make_inputs

pytestmark = pytest.mark.gpu


# ---- gcpx_topn_accumulate ----------------------------------------------------------------------------------------------------
def _run_accumulate(metrics, pools, maps, first, last, full_pools, full_map, comp, lower):
    """metrics [N, B, 3]; pools[n] [R, D]; maps[n] [B, T] -> (all [B, N, 3], best [B], best_frames [B, T, D], best_full [B, F, D])"""
    from video_gcp_amd import runtime as rt
    lib = rt.load_library()
    N, B, _ = metrics.shape
    T, D = maps[0].shape[1], pools[0].shape[1]
    F = full_map.shape[1]
    dev = torch.device("cuda")
    all_ = torch.full((B, N, 3), float("nan"), device=dev)
    best = torch.full((B,), -7, dtype=torch.int32, device=dev)
    frames = torch.full((B, T, D), float("nan"), device=dev)
    full = torch.full((B, F, D), float("nan"), device=dev)
    fmap = torch.from_numpy(full_map).to(dev)
    fi, la = torch.from_numpy(first).to(dev), torch.from_numpy(last).to(dev)
    st = torch.cuda.current_stream().cuda_stream
    keep = []
    for n in range(N):
        m = torch.from_numpy(metrics[n]).to(dev)
        p, mp, fp = torch.from_numpy(pools[n]).to(dev), torch.from_numpy(maps[n]).to(dev), torch.from_numpy(full_pools[n]).to(dev)
        keep += [m, p, mp, fp]
        rt.check(lib.gcpx_topn_accumulate(m.data_ptr(), B, n, N, comp, lower, all_.data_ptr(), best.data_ptr(), p.data_ptr(), p.shape[0],
                                          mp.data_ptr(), fi.data_ptr(), la.data_ptr(), T, frames.data_ptr(), fp.data_ptr(), fp.shape[0],
                                          fmap.data_ptr(), F, full.data_ptr(), D, st), "topn_accumulate")
    torch.cuda.synchronize()
    return all_.cpu().numpy(), best.cpu().numpy(), frames.cpu().numpy(), full.cpu().numpy()


@pytest.mark.parametrize("comp,lower", [(0, 1), (1, 0), (2, 0)])
def test_topn_accumulate_matches_numpy(comp, lower):
    """random metrics with planted ties (the first sample must win) and NaNs (np.argmin / np.argmax return the first NaN); the best
    frames must be bit-identical to the chosen sample's mapped frames, zero outside [first, last) and for rows < 0 or >= the pool"""
    rng = np.random.RandomState(comp)
    N, B, T, D, R, F = 7, 6, 5, 12, 9, 3
    metrics = rng.rand(N, B, 3).astype(np.float32)
    opt = (lambda v: v.min()) if lower else (lambda v: v.max())
    metrics[[2, 5], 0, comp] = opt(metrics[:, 0, comp]) + (-1.0 if lower else 1.0)    # tie at the optimum: sample 2 wins
    metrics[:, 1, comp] = 0.5                                                          # all equal: sample 0
    metrics[[3, 6], 2, comp] = np.nan                                                  # first NaN: sample 3
    metrics[0, 3, comp] = np.nan                                                       # NaN at sample 0 stays best
    metrics[[4, 6], 4, comp] = metrics[4, 4, comp] + (-2.0 if lower else 2.0)          # the later equal value does not replace
    pools = [rng.randn(R, D).astype(np.float32) for _ in range(N)]
    full_pools = [rng.randn(B * F, D).astype(np.float32) for _ in range(N)]
    maps = [rng.randint(-1, R + 2, size=(B, T)).astype(np.int32) for _ in range(N)]    # includes -1 and rows past the pool
    full_map = rng.permutation(B * F).reshape(B, F).astype(np.int32)
    first = rng.randint(0, 2, size=B).astype(np.int32)
    last = rng.randint(2, T + 1, size=B).astype(np.int32)
    all_, best, frames, full = _run_accumulate(metrics, pools, maps, first, last, full_pools, full_map, comp, lower)
    assert np.array_equal(all_, metrics.transpose(1, 0, 2), equal_nan=True)
    want = np.argmin(metrics[..., comp].T, 1) if lower else np.argmax(metrics[..., comp].T, 1)
    assert want.tolist()[:5] == [2, 0, 3, 0, 4]
    assert np.array_equal(best, want)
    for b in range(B):
        n = want[b]
        for t in range(T):
            r = maps[n][b, t]
            ok = first[b] <= t < last[b] and 0 <= r < R
            exp = pools[n][r] if ok else np.zeros(D, np.float32)
            assert np.array_equal(frames[b, t], exp), (b, t)
        assert np.array_equal(full[b], full_pools[n][full_map[b]])


# ---- the trainer ---------------------------------------------------------------------------------------------------------------
def _dataset(root):
    from dataset_fixture import write_random_dataset
    write_random_dataset(str(root), T=20, img=32, n_files=2, traj_per_file=3, seed=3, phases=("train", "val", "test"), min_len=6)
    return str(root)


def _experiment(path, **conf):
    os.makedirs(path, exist_ok=True)
    json.dump(dict(config="c1", **conf), open(os.path.join(path, "conf.json"), "w"))
    return str(path)


def _restart_noise(model):
    """the noise stream where ModelTrainer.__init__ starts it (seed 0, one rank: torch.cuda.manual_seed(1), then reseed())"""
    torch.cuda.manual_seed(1)
    model.reseed()


def _direct_evaluation(trainer, scheme, n):
    """what --metric 1 must compute: the trainer's validation loop with a plain Evaluator, from the same point of the noise stream"""
    from video_gcp_amd.evaluation import Evaluator
    m = trainer.model
    _restart_noise(m)
    ev = Evaluator(m, pruning_scheme=scheme, top_of_100=True, top_of=n)
    for inputs in trainer.val_loader:
        with m.val_mode(pred_length=False):
            out = m(inputs, "test")
            ev.eval(inputs, out, m)
        m(inputs)
    return ev


def _check_oracle(d, it):
    """the best sample's aligned frames, scored by the oracle, give the best sample's written metrics"""
    from oracle import metrics_oracle as MO
    z = np.load(os.path.join(d, f"results_{it}.npz"))
    gt = np.load(os.path.join(d, "gt_seq", f"it_{it}", "gt_seq_0.npy"))
    gen = np.load(os.path.join(d, "gen_images", f"it_{it}", "gen_images_0.npy"))
    S = z["mse"].shape[0]
    assert gt.shape == gen.shape and gt.shape[0] == S
    for s in range(S):
        k = int(np.count_nonzero(np.abs(gen[s]).reshape(gen.shape[1], -1).max(1) > 0))   # frames 1 .. end - 1, zeros after
        assert not np.any(gen[s, k:])
        b = int(z["best"][s])
        if k == 0:                                                   # nothing left after the crop
            assert np.isnan(z["mse"][s, b])
            continue
        mse, psnr, ssim = MO.sequence_metrics(gen[s, :k], gt[s, :k])
        assert abs(float(z["mse"][s, b]) - mse) <= 2e-4 * mse
        assert abs(float(z["psnr"][s, b]) - psnr) <= 2e-3
        assert abs(float(z["ssim"][s, b]) - ssim) <= 1e-4


@pytest.mark.parametrize("scheme", ["dtw", "pruned_dtw", "basic"])
def test_metric_pass_writes_the_evaluation_and_leaves_the_weights(tmp_path, scheme, capsys):
    from video_gcp_amd.train import ModelTrainer, get_cmd_args
    from video_gcp_amd.evaluation import summary_lines
    data = _dataset(tmp_path / "data")
    exp = _experiment(tmp_path / "exp", metric_pruning_scheme=scheme)
    n = 3
    argv = ["--path", exp, "--data_dir", data, "--metric", "1", "--top_of", str(n)]
    tr = ModelTrainer(get_cmd_args(argv))
    assert tr.val_loader.ds.phase == "test" and not tr.val_loader.shuffle
    before = {k: v.clone() for k, v in tr.model.sd.items()}
    tr.run()
    torch.cuda.synchronize()
    assert all(torch.equal(before[k], v) for k, v in tr.model.sd.items())      # no optimizer step
    assert tr.global_step == 0 and not os.path.exists(os.path.join(exp, "weights"))
    d = os.path.join(exp, "metrics")
    z = np.load(os.path.join(d, "results_0.npz"))
    S = len(tr.val_loader) * tr.model._hp.batch_size
    assert z["mse"].shape == z["psnr"].shape == z["ssim"].shape == (S, n) and z["best"].shape == (S,)
    assert np.array_equal(z["best"], np.argmin(z["mse"], 1))
    text = open(os.path.join(d, "results_0.txt")).read()
    lines, summary = summary_lines(dict(z), top_of_100=True)
    assert text == "".join(lines) and len(lines) == 3
    out = capsys.readouterr().out
    assert ",".join(str(v) for v in summary) in out and "Finished Evaluation" in out
    # the first call of a launch plan replays it a few times while it chooses between graph and eager launches, which draws noise: the
    # comparison runs the pass a second time from the start of the stream, with every plan built, next to the direct evaluation
    _restart_noise(tr.model)
    tr.run()
    z = np.load(os.path.join(d, "results_0.npz"))
    ev = _direct_evaluation(tr, scheme, n).collected()
    for k in ("mse", "psnr", "ssim"):
        np.testing.assert_allclose(z[k], ev[k], rtol=1e-6, atol=0)
    assert np.array_equal(z["best"], ev["best"])
    nodes = np.load(os.path.join(d, "full_gen_seq", "it_0", "full_gen_seq_0.npy"))
    assert nodes.shape == (S, tr.model._hp.n_nodes, 3, 32, 32)
    _check_oracle(d, 0)


def test_validation_with_top_of_n_writes_one_file_per_validation(tmp_path):
    from video_gcp_amd.train import ModelTrainer, get_cmd_args
    exp = _experiment(tmp_path / "exp")
    tr = ModelTrainer(get_cmd_args(["--path", exp, "--skip_top100_val", "0", "--top_of", "2", "--num_epochs", "1",
                                    "--batches_per_epoch", "2"]))
    tr.run()
    d = os.path.join(exp, "metrics")
    assert sorted(f for f in os.listdir(d) if f.startswith("results_")) == ["results_0.npz", "results_0.txt", "results_2.npz",
                                                                           "results_2.txt"]
    assert np.load(os.path.join(d, "results_2.npz"))["mse"].shape == (tr.model._hp.batch_size, 2)
    _check_oracle(d, 2)
    exp2 = _experiment(tmp_path / "exp2")
    tr2 = ModelTrainer(get_cmd_args(["--path", exp2, "--num_epochs", "1", "--batches_per_epoch", "2"]))
    assert tr2.evaluator is None
    tr2.run()
    assert not os.path.exists(os.path.join(exp2, "metrics"))


# ---- the flat model ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", ["basic", "dtw"])
def test_sequential_model_evaluation_matches_oracle(scheme):
    """SequentialRecModule.get_sample_with_len (sequential.py:70-97): 'basic' = images[:, :end + 1]; 'dtw' = images[1:end + 1] warped
    onto traj_seq[1:end + 1] with images[:, 1] in front; then the crop of the first and last frame and the metrics"""
    import video_gcp_amd as V
    from oracle import adaptive_oracle as A, metrics_oracle as MO
    from video_gcp_amd.evaluation import Evaluator
    from video_gcp_amd.sequential import GCPSequentialModel
    hp = V.config("c1", batch_size=3, nz_mid_lstm=128, lstm_init="zero")
    model = GCPSequentialModel(hp, params=V.init_params_sequential(hp, seed=1, randomize_affine=True), device="cuda")
    inputs, noise, _ = make_inputs(hp, seed=8, variant="B")
    inputs["end_ind"] = torch.tensor([hp.max_seq_len - 1, 6, 11])
    noise = noise[:, :hp.max_seq_len - 1].contiguous()
    dev_in = {k: v.cuda() for k, v in inputs.items()}
    ev = Evaluator(model, pruning_scheme=scheme, top_of_100=False)
    with model.val_mode(pred_length=False):
        out = model(dev_in, "train", noise=noise.cuda())
        images = out.dense_rec.images.cpu()
        res = ev.eval(dev_in, out, model)
    got = ev.collected()
    for b in range(hp.batch_size):
        end = int(inputs["end_ind"][b])
        tgt = inputs["traj_seq"][b, :end + 1]
        if scheme == "basic":
            gen = images[b, :end + 1]
        else:
            est, t1 = images[b, 1:end + 1], inputs["traj_seq"][b, 1:end + 1]
            cost = ((est[:, None] - t1[None]) ** 2).mean(dim=(2, 3, 4)).numpy()
            _, _, _, inds = A.dtw_matches(cost)
            gen = torch.cat([images[b, [1]], est[inds]], 0)          # the reference's prepend of frame 1
        assert gen.shape[0] == end + 1
        mse, psnr, ssim = MO.sequence_metrics(gen[1:-1].numpy(), tgt[1:-1].numpy())
        assert abs(float(res["mse"][b, 0]) - mse) <= 2e-4 * mse
        assert abs(float(res["psnr"][b, 0]) - psnr) <= 2e-3
        assert abs(float(res["ssim"][b, 0]) - ssim) <= 1e-4
        assert torch.equal(torch.from_numpy(got["gen_images"][b, :end - 1]), gen[1:-1])
        assert not np.any(got["gen_images"][b, end - 1:])
    assert got["full_gen_seq"].shape[1] == hp.max_seq_len - 2
    with pytest.raises(ValueError):
        Evaluator(model, pruning_scheme="pruned_dtw")
