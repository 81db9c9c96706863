"""CPU: the trainer's evaluation flags (gcp_builder.py:84-95,188-247), the results writer against the reference's lines
(compute_metrics.py:214-226,341-345) recomputed with numpy, and the data-parallel gather under a gloo world of two ranks."""
import os
import re
import sys
import types

import numpy as np
import pytest

from test_dist_cpu import _run_ranks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flags_and_defaults():
    from video_gcp_amd.train import get_cmd_args, val_phase
    a = get_cmd_args([])
    assert (a.metric, a.skip_top100_val, a.top_of) == (0, 1, 100)            # --skip_top100_val: 1 here, 0 in the reference
    assert val_phase(a) == "val"
    a = get_cmd_args(["--metric", "1", "--skip_top100_val", "0", "--top_of", "3"])
    assert (a.metric, a.skip_top100_val, a.top_of) == (1, 0, 3)
    assert val_phase(a) == "test"


def test_metric_reads_the_test_split_unshuffled(tmp_path):
    from dataset_fixture import write_random_dataset
    from video_gcp_amd.dataset import load_spec
    from video_gcp_amd.train import get_cmd_args, make_loader, val_phase
    write_random_dataset(str(tmp_path), T=8, img=8, n_files=3, traj_per_file=2, seed=1, phases=("train", "val", "test"))
    hp = types.SimpleNamespace(max_seq_len=8, img_sz=8, batch_size=2)
    model = types.SimpleNamespace(_hp=hp, device="cpu")
    spec = load_spec(str(tmp_path))
    ld = make_loader(str(tmp_path), spec, val_phase(get_cmd_args(["--metric", "1"])), hp, model, {}, n_repeat=1, seed=5)
    assert ld.ds.phase == "test" and not ld.shuffle
    assert all("/hdf5/test/" in f for f in ld.ds.filenames)
    order = [i for b in ld.schedule() for i, _, _ in b]
    assert order == list(range(len(ld.ds)))
    tr = make_loader(str(tmp_path), spec, "train", hp, model, {}, n_repeat=1, seed=5)
    assert tr.shuffle


def _fixed_evaluation(S=7, N=5, seed=0):
    rng = np.random.RandomState(seed)
    ev = {"mse": rng.rand(S, N).astype(np.float32) * 0.1, "psnr": 20 + rng.rand(S, N).astype(np.float32) * 10,
          "ssim": rng.rand(S, N).astype(np.float32)}
    ev["best"] = np.argmin(ev["mse"], 1)
    ev["gt_seq"] = rng.rand(S, 4, 3, 8, 8).astype(np.float32)
    ev["gen_images"] = rng.rand(S, 4, 3, 8, 8).astype(np.float32)
    ev["full_gen_seq"] = rng.rand(S, 7, 3, 8, 8).astype(np.float32)
    return ev


@pytest.mark.parametrize("top_of_100", [True, False])
def test_results_writer_writes_the_reference_lines(tmp_path, capsys, top_of_100):
    from video_gcp_amd.evaluation import write_results
    ev = _fixed_evaluation()
    path = write_results(str(tmp_path), 12, ev, top_of_100=top_of_100)
    assert path == os.path.join(str(tmp_path), "metrics", "results_12.txt")
    want, summary = [], []
    for name in ("mse", "psnr", "ssim"):
        v = ev[name].astype(np.float64)
        bv = np.array([v[s, ev["best"][s]] for s in range(v.shape[0])])
        m, sem, spread = np.mean(bv), np.std(bv), np.mean(np.std(v, axis=1))
        line = f"mean {name} {m}, standard error of the mean (SEM) {sem}"
        line += f", mean std of 100 samples {spread}\n" if top_of_100 else "\n"
        want.append(line)
        summary += [m, sem, spread]
    assert open(path).read() == "".join(want)
    out = capsys.readouterr().out
    assert ",".join(str(x) for x in summary) + "\n" in out
    assert re.search(r"^mean mse [0-9.e-]+, standard error of the mean \(SEM\) ", out, re.M)
    z = np.load(os.path.join(str(tmp_path), "metrics", "results_12.npz"))
    assert sorted(z.files) == ["best", "mse", "psnr", "ssim"]
    for k in z.files:
        assert np.array_equal(z[k], ev[k])
    for k in ("gt_seq", "gen_images", "full_gen_seq"):
        assert np.array_equal(np.load(os.path.join(str(tmp_path), "metrics", k, "it_12", f"{k}_0.npy")), ev[k])


def _rank_evaluation(rank, n_batches, B, flat):
    ev = _fixed_evaluation(S=n_batches * B, N=4, seed=10 + rank)
    if flat:                                   # the flat model's full_gen_seq: as long as the longest prediction of the rank
        ev["full_gen_seq"] = ev["full_gen_seq"][:, :5 + rank]
    return ev


def _gather_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch
    from video_gcp_amd import dist as D
    from video_gcp_amd.evaluation import gather_evaluation, summary_lines
    D.init_from_env("gloo")
    res = []
    for flat in (False, True):
        got = gather_evaluation(_rank_evaluation(rank, 3, 2, flat), 2)
        res.append(None if got is None else (got, summary_lines(got)))
    q.put((rank, res))
    torch.distributed.destroy_process_group()


def test_two_rank_gather_equals_one_process():
    from video_gcp_amd.evaluation import summary_lines
    out = dict(_run_ranks(_gather_worker))
    assert out[1] == [None, None]                                  # only rank 0 holds the gathered arrays
    for flat, (got, (lines, summary)) in zip((False, True), out[0]):
        parts = [_rank_evaluation(r, 3, 2, flat) for r in range(2)]
        # one process with batch 4 over the same sequences: global batch g = rank 0's 2 sequences of it, then rank 1's
        want = {}
        for k in parts[0]:
            L = max(p[k].shape[1] for p in parts) if k == "full_gen_seq" else None
            blocks = []
            for g in range(3):
                for p in parts:
                    x = p[k][2 * g:2 * g + 2]
                    if L is not None and x.shape[1] < L:
                        x = np.concatenate((x, np.zeros((2, L - x.shape[1]) + x.shape[2:], x.dtype)), 1)
                    blocks.append(x)
            want[k] = np.concatenate(blocks, 0)
        assert sorted(got) == sorted(want)
        for k in want:
            assert np.array_equal(got[k], want[k]), k
        assert (lines, summary) == summary_lines(want)
