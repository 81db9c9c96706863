"""The device-resident data path on the host (video-gcp_amd/dataset_resident.py): the store's layout and tables, its numpy mirror
against the host-fed path's numpy assembly on every branch of the draws, the reference's own items (tests/golden/ref_dataset.npz)
through the mirror, draws without files, the capacity and top-down errors, and the loader's schedule.  No GPU: the store is built on
the CPU device."""
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import video_gcp_amd  # noqa: E402,F401
from video_gcp_amd import dataset as DS  # noqa: E402
from video_gcp_amd import dataset_resident as DR  # noqa: E402
import dataset_fixture as FX  # noqa: E402
import topdown_fixture as TF  # noqa: E402

T, IMG = 8, 8
CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def random_dir(tmp_path_factory):
    """3 files x 3 trajectories of 8 x 8 frames, ragged lengths in [4, 12]: some shorter than T = 8"""
    root = str(tmp_path_factory.mktemp("resident"))
    FX.write_random_dataset(root, T=T, img=IMG, n_files=3, traj_per_file=3, min_len=4)
    return root


def _mirror_batch(store, batch, seed):
    ds = store.ds
    info, pad = DR.resident_batch_info(store, batch, seed)
    return DR.resident_batch_numpy(store.host_arrays(), info, pad, ds.T, ds.states_mean, ds.states_den,
                                   img_sz=ds.img_sz if ds.resize else None), info


def _assert_mirror_equals_host_path(ds, seed=5, batch_size=3, epochs=2):
    store = DR.ResidentStore(ds, CPU)
    n = 0
    for epoch in range(epochs):
        for batch in DS.epoch_schedule(len(ds), batch_size, 2, seed, epoch, shuffle=ds.phase == "train"):
            ref = DS.numpy_batch(ds, batch, seed)
            got, _ = _mirror_batch(store, batch, seed)
            assert set(got) == set(ref)
            for k in ref:
                assert got[k].dtype == ref[k].dtype and np.array_equal(got[k], ref[k]), (epoch, n, k)
            n += 1
    assert n
    return store


def test_store_layout_and_tables(random_dir):
    ds = DS.VideoDataset(random_dir, DS.load_spec(random_dir), "train", IMG)
    store = DR.ResidentStore(ds, CPU, n_workers=3)
    raws = [ds.read(i) for i in range(len(ds))]
    n = np.array([r["images"].shape[0] for r in raws])
    assert len(store) == 9 and n.min() < T < n.max()
    assert np.array_equal(store.n, n) and store.first_frame.dtype == np.int64
    assert np.array_equal(store.first_frame, np.cumsum(n) - n) and np.array_equal(store.first_state, store.first_frame)
    assert np.array_equal(store.first_action, np.cumsum(n - 1) - (n - 1))
    assert (store.Hs, store.Ws, store.S, store.A) == (IMG, IMG, 2, 2)
    frames, states, actions = store.host_arrays()
    assert store.frames.dtype == torch.uint8 and store.frames.numel() == n.sum() * IMG * IMG * 3 == store.frames_bytes
    assert store.frames.data_ptr() % 16 == 0
    assert store.nbytes == store.frames_bytes + 4 * (n.sum() * 2 + (n - 1).sum() * 2)
    # back to back in dataset index order, nothing between the trajectories
    assert np.array_equal(frames, np.concatenate([r["images"] for r in raws]))
    assert states.dtype == np.float32 and np.array_equal(states, np.concatenate([r["states"] for r in raws]))
    assert actions.shape == ((n - 1).sum(), 2) and np.array_equal(actions, np.concatenate([r["actions"] for r in raws]))
    for i, r in enumerate(raws):
        assert np.array_equal(store.pad_masks[i], r["pad_mask"])


@pytest.mark.parametrize("phase,rl,rs,std", [("train", False, False, False), ("val", False, False, False), ("train", True, False, False),
                                             ("val", True, False, False), ("train", False, True, False), ("train", True, False, True)])
def test_mirror_equals_the_host_assembly(random_dir, phase, rl, rs, std):
    spec = DS.load_spec(random_dir)
    if std:
        spec.update(states_mean=FX.STATES_MEAN, states_std=FX.STATES_STD)
    ds = DS.VideoDataset(random_dir, spec, phase, IMG, randomize_length=rl, randomize_start=rs)
    store = _assert_mirror_equals_host_path(ds)
    if phase == "val" and not rl:               # a window that runs past a short trajectory: its frames are padding, -1.0
        got, info = _mirror_batch(store, DS.epoch_schedule(len(ds), 9, 1, 5, 0, False)[0], 5)
        assert (info[:, 1] < T).any() and (got["traj_seq"] == -1.0).all(axis=(2, 3, 4)).any()


def test_mirror_resizes_like_the_host_assembly(tmp_path):
    FX.write_random_dataset(str(tmp_path), T=T, img=12, n_files=2, traj_per_file=3, phases=("train",), min_len=4)
    ds = DS.VideoDataset(str(tmp_path), DS.load_spec(str(tmp_path)), "train", IMG, randomize_length=True, resize=True)
    store = _assert_mirror_equals_host_path(ds)
    assert (store.Hs, store.Ws) == (12, 12)


def test_dataset_without_states_and_actions_and_with_cameras(tmp_path):
    """files that hold images and pad masks only, the images as [n, n_cam, H, W, 3]: camera 0 is stored"""
    rng = np.random.RandomState(3)
    for f in range(2):
        d = {"traj_per_file": np.array(3)}
        for i in range(3):
            n = int(rng.randint(4, 13))
            d[f"traj{i}/images"] = rng.randint(0, 256, size=(n, 2, IMG, IMG, 3)).astype(np.uint8)
            d[f"traj{i}/pad_mask"] = np.ones(n, dtype=np.float32)
        FX.write_npz(str(tmp_path / "hdf5" / "train" / f"file_{f}.npz"), d)
    FX.write_spec(str(tmp_path), max_seq_len=T)
    ds = DS.VideoDataset(str(tmp_path), DS.load_spec(str(tmp_path)), "train", IMG)
    store = _assert_mirror_equals_host_path(ds, batch_size=2)
    assert (store.S, store.A) == (0, 0) and store.states.shape[1] == 0 and store.nbytes == store.frames_bytes
    cam0 = np.concatenate([np.load(f)[f"traj{i}/images"][:, 0] for f in ds.filenames for i in range(3)])
    assert np.array_equal(store.host_arrays()[0], cam0)
    got, _ = _mirror_batch(store, DS.epoch_schedule(len(ds), 2, 1, 5, 0, True)[0], 5)
    assert "traj_seq_states" not in got and "actions" not in got


@pytest.mark.parametrize("case", FX.CASES)
def test_mirror_reproduces_the_reference_items(tmp_path, case):
    g = FX.write_golden_dataset(str(tmp_path))
    is_train, rl, rs, std, seed = (int(x) for x in g[f"{case}:cfg"])
    spec = dict(max_seq_len=8)
    if std:
        spec.update(states_mean=FX.STATES_MEAN, states_std=FX.STATES_STD)
    ds = DS.VideoDataset(str(tmp_path), spec, "train" if is_train else "val", 8, randomize_length=rl, randomize_start=rs)
    store = DR.ResidentStore(ds, CPU)
    arrays = store.host_arrays()
    r = np.random.RandomState(seed)             # the reference: np.random.seed(seed), then the items in index order
    for i in range(len(ds)):
        plan = store.draw(i, r)
        got = DR.resident_batch_numpy(arrays, DR.resident_info(store, i, plan)[None], plan["pad_mask"][None], ds.T, ds.states_mean,
                                      ds.states_den)
        for k in ("traj_seq", "I_0", "I_g", "pad_mask", "traj_seq_states", "actions"):
            ref = g[f"{case}:{i}:{k}"]
            assert got[k][0].dtype == ref.dtype and np.array_equal(got[k][0], ref), (case, i, k)
        assert int(got["end_ind"][0]) == int(g[f"{case}:{i}:end_ind"]) and int(got["start_ind"][0]) == 0


def test_draws_touch_no_file_once_the_store_is_built(tmp_path):
    data = tmp_path / "data"
    FX.write_random_dataset(str(data), T=T, img=IMG, n_files=2, traj_per_file=3, phases=("train",), min_len=4)
    ds = DS.VideoDataset(str(data), DS.load_spec(str(data)), "train", IMG, randomize_length=True)
    batches = DS.epoch_schedule(len(ds), 3, 1, 7, 0, True)
    ref = [DS.numpy_batch(ds, b, 7) for b in batches]
    store = DR.ResidentStore(ds, CPU)
    os.rename(str(data), str(tmp_path / "gone"))
    ds._cache = DS._FileCache()                 # and no handle that was open before: a read would have to open a file again
    with pytest.raises(FileNotFoundError):
        ds.read(0)
    for b, want in zip(batches, ref):
        got, _ = _mirror_batch(store, b, 7)
        for k in want:
            assert np.array_equal(got[k], want[k]), k


def test_info_that_points_outside_the_store_is_padding(random_dir):
    """the mirror's (and the kernels') answer to integers that do not belong to the store: a padded frame, nothing read"""
    ds = DS.VideoDataset(random_dir, DS.load_spec(random_dir), "val", IMG)
    store = DR.ResidentStore(ds, CPU)
    arrays = store.host_arrays()
    N = arrays[0].shape[0]
    info = np.array([[N - 2, T, 0, 0, 0, 0, 0, T | (T - 1) << 32], [-1, T, -1, T, -1, T, 0, T | 0 << 32]], dtype=np.int64)
    got = DR.resident_batch_numpy(arrays, info, np.ones((2, T), dtype=np.float32), T)
    assert np.array_equal(got["traj_seq"][0, :2], DS.LUT[np.transpose(arrays[0][N - 2:], (0, 3, 1, 2))])
    assert (got["traj_seq"][0, 2:] == -1.0).all() and (got["traj_seq"][1] == -1.0).all()
    assert (got["traj_seq_states"] == 0).all() and (got["actions"] == 0).all()


def test_a_split_over_the_budget_raises_and_names_the_bytes(random_dir):
    ds = DS.VideoDataset(random_dir, DS.load_spec(random_dir), "train", IMG)
    need = DR.ResidentStore(ds, CPU).nbytes
    with pytest.raises(ValueError, match=rf"needs {need} bytes.*has {need - 1} bytes available"):
        DR.ResidentStore(ds, CPU, budget_bytes=need - 1)
    assert DR.ResidentStore(ds, CPU, budget_bytes=need).nbytes == need


def test_a_top_rendered_dataset_raises(tmp_path):
    TF.write_topdown_dataset(str(tmp_path), T=T, n_files=4, traj_per_file=3, seed=2, min_len=5, scale=24, cw=6, k=7)
    ds = DS.VideoDataset(str(tmp_path), DS.load_spec(str(tmp_path)), "train", IMG)
    assert ds.topdown is not None
    with pytest.raises(ValueError, match="top-rendered"):
        DR.ResidentStore(ds, CPU)
    model = types.SimpleNamespace(_hp=types.SimpleNamespace(max_seq_len=T, img_sz=IMG, batch_size=3), device=CPU)
    with pytest.raises(ValueError, match="top-rendered"):
        DR.ResidentLoader(ds, model, 3)


def test_a_trajectory_whose_arrays_disagree_with_its_pad_mask_raises(tmp_path):
    rng = np.random.RandomState(0)
    d = {"traj_per_file": np.array(1), "traj0/images": rng.randint(0, 256, size=(6, IMG, IMG, 3)).astype(np.uint8),
         "traj0/states": rng.randn(5, 2).astype(np.float32), "traj0/actions": rng.randn(5, 2).astype(np.float32),
         "traj0/pad_mask": np.ones(6, dtype=np.float32)}
    FX.write_npz(str(tmp_path / "hdf5" / "train" / "file_0.npz"), d)
    FX.write_spec(str(tmp_path), max_seq_len=T)
    ds = DS.VideoDataset(str(tmp_path), DS.load_spec(str(tmp_path)), "train", IMG)
    with pytest.raises(ValueError, match="states has 5 rows"):
        DR.ResidentStore(ds, CPU)


@pytest.mark.parametrize("phase", ["train", "val"])
def test_loader_schedule_equals_the_host_fed_loader(random_dir, phase):
    ds = DS.VideoDataset(random_dir, DS.load_spec(random_dir), phase, IMG)
    model = types.SimpleNamespace(_hp=types.SimpleNamespace(max_seq_len=T, img_sz=IMG, batch_size=2), device=CPU)
    for rank, world in ((0, 1), (1, 2)):
        host = DS.HostFedLoader(ds, model, 2, n_repeat=2, seed=3, rank=rank, world=world)
        res = DR.ResidentLoader(ds, model, 2, n_repeat=2, seed=3, rank=rank, world=world)
        assert res.shuffle == host.shuffle == (phase == "train") and len(res) == len(host)
        for epoch in (0, 3):
            host.set_epoch(epoch)
            res.set_epoch(epoch)
            assert res.schedule() == host.schedule() and len(res.schedule()) == len(res)
    with pytest.raises(ValueError, match="batch"):
        DR.ResidentLoader(ds, model, 3)
