"""The dataset reader (video-gcp_amd/dataset.py) against the reference's own data loader executed on the fixture
(tests/golden/make_ref_dataset_goldens.py): draws, padding, chopping, conversion, splits and shuffles; the spec file; the loader's
schedule across ranks and resumes.  No GPU."""
import os
import socket
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import video_gcp_amd  # noqa: E402,F401
from video_gcp_amd import dataset as DS  # noqa: E402
import dataset_fixture as FX  # noqa: E402


@pytest.fixture(scope="module")
def golden_dir(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("ref_dataset"))
    return root, FX.write_golden_dataset(root)


def _case_dataset(root, g, case):
    is_train, rl, rs, std, seed = (int(x) for x in g[f"{case}:cfg"])
    spec = dict(max_seq_len=8)
    if std:
        spec.update(states_mean=FX.STATES_MEAN, states_std=FX.STATES_STD)
    ds = DS.VideoDataset(root, spec, "train" if is_train else "val", 8, randomize_length=rl, randomize_start=rs)
    return ds, seed


@pytest.mark.parametrize("case", FX.CASES)
def test_items_reproduce_the_reference_draws_exactly(golden_dir, case):
    root, g = golden_dir
    ds, seed = _case_dataset(root, g, case)
    assert [os.path.relpath(f, root) for f in ds.filenames] == list(g[f"{case}:files"])
    rs = np.random.RandomState(seed)            # the reference: np.random.seed(seed), then the items in index order
    for i in range(len(ds)):
        got = DS.assemble_numpy([ds.item(i, rs)], ds.T, ds.states_mean, ds.states_den)
        for k in ("traj_seq", "I_0", "I_g", "pad_mask", "traj_seq_states", "actions"):
            ref = g[f"{case}:{i}:{k}"]
            assert got[k][0].dtype == ref.dtype and np.array_equal(got[k][0], ref), (case, i, k)
        assert int(got["end_ind"][0]) == int(g[f"{case}:{i}:end_ind"]) and int(g[f"{case}:{i}:start_ind"]) == 0


def test_golden_covers_the_edges(golden_dir):
    """the fixture holds what the kernel tests lean on: padded frames (-1.0), end_ind at T-1 and short, chopped sequences"""
    _, g = golden_dir
    ends = [int(g[f"{c}:{i}:end_ind"]) for c in FX.CASES for i in range(4)]
    assert 7 in ends and min(ends) <= 2
    assert any((g[f"val:{i}:traj_seq"] == -1.0).all(axis=(1, 2, 3)).any() for i in range(4))


def test_global_split_and_shuffle(tmp_path, golden_dir):
    _, g = golden_dir
    tiny = {k.split(":", 2)[2]: g[k] for k in g.files if k.startswith("data:hdf5/val/file_0:")}
    for name in g["global:names"]:
        FX.write_npz(str(tmp_path / (name + ".npz")), tiny)
    FX.write_npz(str(tmp_path / "dataset_info.npz"), tiny)
    split = {"train": 0.5, "val": 0.25, "test": 0.25}
    for phase in ("train", "val", "test"):
        ds = DS.VideoDataset(str(tmp_path), dict(max_seq_len=8, split=split, dataset_class="GlobalSplitVarLenVideoDataset"), phase, 8)
        assert [os.path.relpath(f, tmp_path)[:-4] for f in ds.filenames] == list(g[f"global:{phase}:files"]), phase


def test_dataset_spec_through_the_placeholder_executor(tmp_path):
    FX.write_spec(str(tmp_path), max_seq_len=12, img_sz=32, dataset_class="FolderSplitVarLenVideoDataset",
                  states_mean="np.array([0.5, 1.0], dtype=np.float32)", states_std="np.ones(2, dtype=np.float32)",
                  split="dict(train=0.9, val=0.1)", n_rooms=25, crop="[1, 2]")
    spec = DS.load_spec(str(tmp_path))
    assert spec["max_seq_len"] == 12 and DS.dataset_class_name(spec) == "FolderSplitVarLenVideoDataset"
    over = DS.spec_overrides(spec, {"max_seq_len", "img_sz", "crop"})
    assert over == {"max_seq_len": 12, "img_sz": 32}                 # lists never override (gcp_builder.py:68)


def test_trainer_conf_takes_max_seq_len_from_the_spec(tmp_path):
    from video_gcp_amd.train import load_conf_with_data
    data = tmp_path / "data"
    FX.write_random_dataset(str(data), T=12, img=32, n_files=1, traj_per_file=2)
    exp = tmp_path / "exp"
    exp.mkdir()
    (exp / "conf.py").write_text("from blox import AttrDict\nconfiguration = {'batch_size': 2, 'data_dir': %r}\n"
                                 "model_config = {'img_sz': 32, 'hierarchy_levels': 4}\n" % str(data))
    hp, conf, ignored, data_dir, spec, extra = load_conf_with_data(str(exp), None, None)
    assert data_dir == str(data) and hp.max_seq_len == 12 and spec["max_seq_len"] == 12
    assert "defaulted:max_seq_len" not in ignored
    # without a dataset the conf reports the default, as before
    hp2, _, ignored2, d2, _, _ = load_conf_with_data(str(exp), None, None, use_data=False)
    assert d2 is None and "defaulted:max_seq_len" in ignored2


def test_wrong_resolution_raises(tmp_path):
    FX.write_random_dataset(str(tmp_path), T=8, img=16, n_files=1, traj_per_file=2, phases=("train",))
    ds = DS.VideoDataset(str(tmp_path), DS.load_spec(str(tmp_path)), "train", 32)
    with pytest.raises(ValueError, match="resize_video"):
        ds.read(0)


def test_unknown_dataset_class_raises(tmp_path):
    with open(tmp_path / "dataset_spec.py", "w") as f:
        f.write("from gcp.datasets.data_loader import MazeTopRenderedGlobalSplitVarLenVideoDataset\n"
                "dataset_spec = dict(max_seq_len=8, dataset_class=MazeTopRenderedGlobalSplitVarLenVideoDataset)\n")
    spec = DS.load_spec(str(tmp_path))
    with pytest.raises(ValueError, match="MiniWorld"):
        DS.dataset_class_name(spec)
    with pytest.raises(ValueError, match="MazeTopRendered"):
        DS.VideoDataset(str(tmp_path), spec, "train", 8)


def test_schedule_is_keyed_and_resumes(tmp_path):
    FX.write_random_dataset(str(tmp_path), T=8, img=8, n_files=3, traj_per_file=4, phases=("train",))
    ds = DS.VideoDataset(str(tmp_path), DS.load_spec(str(tmp_path)), "train", 8)
    s1 = DS.epoch_schedule(len(ds), 4, 2, seed=7, epoch=1, shuffle=True)
    assert len(s1) == 2 * (12 // 4)
    a = [DS.numpy_batch(ds, b, 7) for b in s1]
    # a fresh reader and a "resumed" run at epoch 1 draw the same batches
    ds2 = DS.VideoDataset(str(tmp_path), DS.load_spec(str(tmp_path)), "train", 8)
    b = [DS.numpy_batch(ds2, bb, 7) for bb in DS.epoch_schedule(len(ds2), 4, 2, seed=7, epoch=1, shuffle=True)]
    assert all(np.array_equal(x[k], y[k]) for x, y in zip(a, b) for k in x)
    s0 = DS.epoch_schedule(len(ds), 4, 2, seed=7, epoch=0, shuffle=True)
    assert s0 != s1
    # val: no shuffle, every index once per pass
    v = DS.epoch_schedule(len(ds), 4, 1, seed=7, epoch=0, shuffle=False)
    assert [i for bb in v for i, _, _ in bb] == list(range(12))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_worker(rank, world, port, root, q):
    sys.path.insert(0, ROOT)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import video_gcp_amd  # noqa: F401
    from video_gcp_amd import dataset as D
    torch.distributed.init_process_group("gloo", rank=rank, world_size=world)
    ds = D.VideoDataset(root, D.load_spec(root), "train", 8)
    sched = D.epoch_schedule(len(ds), 2, 1, seed=3, epoch=0, shuffle=True, rank=torch.distributed.get_rank(),
                             world=torch.distributed.get_world_size())
    batches = [D.numpy_batch(ds, b, 3)["traj_seq"] for b in sched]
    q.put((rank, [[i for i, _, _ in b] for b in sched], batches))
    torch.distributed.destroy_process_group()


def test_two_gloo_ranks_split_the_single_process_batch(tmp_path):
    import torch.multiprocessing as mp
    FX.write_random_dataset(str(tmp_path), T=8, img=8, n_files=3, traj_per_file=4, phases=("train",))
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, str(tmp_path), q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=180) for _ in procs], key=lambda r: r[0])
    for p in procs:
        p.join(60)
    assert all(p.exitcode == 0 for p in procs)
    ds = DS.VideoDataset(str(tmp_path), DS.load_spec(str(tmp_path)), "train", 8)
    single = DS.epoch_schedule(len(ds), 4, 1, seed=3, epoch=0, shuffle=True)
    ref = [DS.numpy_batch(ds, b, 3)["traj_seq"] for b in single]
    (_, i0, b0), (_, i1, b1) = res
    assert len(i0) == len(i1) == len(single) == 3
    for g in range(3):
        assert not set(i0[g]) & set(i1[g])
        assert i0[g] + i1[g] == [i for i, _, _ in single[g]]
        assert np.array_equal(np.concatenate([b0[g], b1[g]]), ref[g])
