"""The host-fed data path on the device: gcpx_assemble_batch bit-exact against the reference's own loader (golden) and against
the numpy assembly at the c1 / c2 shapes; trainers fed by HostFedLoader (2-slot ring: every slot reused) end bit-identical to the
same trainers fed the numpy-assembled batches as ordinary device tensors; ModelTrainer with --data_dir."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import video_gcp_amd as V  # noqa: E402
from video_gcp_amd import dataset as DS  # noqa: E402
from video_gcp_amd import runtime as rt  # noqa: E402
import dataset_fixture as FX  # noqa: E402

pytestmark = pytest.mark.gpu
KEYS = ("traj_seq", "I_0", "I_g", "pad_mask", "end_ind", "start_ind", "traj_seq_states", "actions")


def _assemble_on_device(items, T, img, S, A, mean=None, den=None):
    """pack on the host, upload, gcpx_assemble_batch into fresh device tensors (stale bytes in the staging slot on purpose)"""
    B = len(items)
    frames = np.full((B, T, img, img, 3), 77, dtype=np.uint8)
    aux = np.full(B * T + B * T * S + B * (T - 1) * A, 5.0, dtype=np.float32)
    info = np.zeros((B, DS.N_INFO), dtype=np.int32)
    for j, it in enumerate(items):
        DS.pack_item(it, j, frames, aux, info, B, T, S, A)
    dev = torch.device("cuda")
    out = dict(traj_seq=torch.full((B, T, 3, img, img), 9.0, device=dev), I_0=torch.full((B, 3, img, img), 9.0, device=dev),
               I_g=torch.full((B, 3, img, img), 9.0, device=dev), pad_mask=torch.full((B, T), 9.0, device=dev),
               end_ind=torch.full((B,), 99, dtype=torch.int64, device=dev), start_ind=torch.full((B,), 99, dtype=torch.int64, device=dev),
               traj_seq_states=torch.full((B, T, S), 9.0, device=dev), actions=torch.full((B, T - 1, A), 9.0, device=dev))
    t = lambda a: torch.from_numpy(a).to(dev)
    md = (t(mean), t(den)) if mean is not None else (None, None)
    DS.assemble_into(rt.load_library(), t(frames), t(aux), t(info), t(DS.LUT), md[0], md[1], out, S, A,
                     torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


@pytest.mark.parametrize("case", FX.CASES)
def test_assembly_is_bit_exact_against_the_reference_loader(tmp_path, case):
    g = FX.write_golden_dataset(str(tmp_path))
    is_train, rl, rs, std, seed = (int(x) for x in g[f"{case}:cfg"])
    spec = dict(max_seq_len=8)
    if std:
        spec.update(states_mean=FX.STATES_MEAN, states_std=FX.STATES_STD)
    ds = DS.VideoDataset(str(tmp_path), spec, "train" if is_train else "val", 8, randomize_length=rl, randomize_start=rs)
    r = np.random.RandomState(seed)
    items = [ds.item(i, r) for i in range(len(ds))]
    got = _assemble_on_device(items, 8, 8, 2, 2, ds.states_mean, ds.states_den)
    for i in range(len(ds)):
        for k in ("traj_seq", "I_0", "I_g", "pad_mask", "traj_seq_states", "actions"):
            assert torch.equal(got[k][i], torch.from_numpy(g[f"{case}:{i}:{k}"])), (case, i, k)
        assert int(got["end_ind"][i]) == int(g[f"{case}:{i}:end_ind"]) and int(got["start_ind"][i]) == 0
    if case == "val":                           # frames padded past the recording are -1.0, not 0.0
        assert any(bool((got["traj_seq"][i] == -1.0).all(dim=(1, 2, 3)).any()) for i in range(len(ds)))


@pytest.mark.parametrize("name,rl", [("c1", True), ("c2", True), ("c2", False)])
def test_assembly_matches_numpy_at_model_shapes(tmp_path, name, rl):
    hp = V.config(name)
    T, img, B = hp.max_seq_len, hp.img_sz, hp.batch_size
    FX.write_random_dataset(str(tmp_path), T=T, img=img, n_files=1, traj_per_file=B, phases=("train",), min_len=4)
    ds = DS.VideoDataset(str(tmp_path), DS.load_spec(str(tmp_path)), "train", img, randomize_length=rl)
    batch = DS.epoch_schedule(len(ds), B, 1, seed=4, epoch=0, shuffle=True)[0]
    ref = DS.numpy_batch(ds, batch, 4)
    got = _assemble_on_device([ds.item(i, DS.item_rng(4, c, p)) for i, p, c in batch], T, img, 2, 2)
    ends = ref["end_ind"].tolist()
    assert len(set(ends)) > 1
    for k in KEYS:
        assert torch.equal(got[k], torch.from_numpy(ref[k])), k


def _trainer(name, seq=False, graph=True):
    if seq:
        from video_gcp_amd.sequential import GCPSequentialModel
        from video_gcp_amd.training_sequential import SequentialTrainStep
        hp = V.config(name, nz_mid_lstm=128, lstm_init="zero")
        model = GCPSequentialModel(hp, params=V.init_params_sequential(hp, seed=1), device="cuda")
        step = SequentialTrainStep
    else:
        from video_gcp_amd.model import GCPTreeModel
        from video_gcp_amd.training import GCPTrainStep
        hp = V.config(name)
        model = GCPTreeModel(hp, params=V.init_params(hp, seed=1, randomize_affine=True), device="cuda")
        step = GCPTrainStep
    model.use_graph = graph
    model._rng_stream_id = 0                    # the two trainers of a test draw the same in-plan noise after reseed()
    return hp, model, step(model, lr=1e-3)


def _run(model, tr, batches):
    torch.cuda.manual_seed(11)
    model.reseed(11)
    n = 0
    for inputs in batches:
        tr.step(inputs)
        model.step()
        n += 1
    torch.cuda.synchronize()
    return n


def _host_fed_vs_device_fed(tmp_path, name, seq, graph, steps):
    hp0 = V.config(name)
    T, img, B = hp0.max_seq_len, hp0.img_sz, hp0.batch_size
    FX.write_random_dataset(str(tmp_path), T=T, img=img, n_files=2, traj_per_file=3, phases=("train",), min_len=5)
    spec = DS.load_spec(str(tmp_path))
    reps = -(-steps // (6 // B))
    hp, m1, t1 = _trainer(name, seq, graph)
    ds = DS.VideoDataset(str(tmp_path), spec, "train", img, randomize_length=True)
    loader = DS.HostFedLoader(ds, m1, B, n_repeat=reps, seed=3, n_slots=2, n_workers=3)
    loader.set_epoch(1)
    assert len(loader) >= steps
    n1 = _run(m1, t1, loader)
    _, m2, t2 = _trainer(name, seq, graph)
    dev = [{k: torch.from_numpy(v).cuda() for k, v in b.items()} for b in loader.numpy_batches()]
    n2 = _run(m2, t2, dev)
    assert n1 == n2 >= steps
    assert torch.isfinite(m1.theta).all()
    assert torch.equal(m1.theta, m2.theta) and torch.equal(t1.exp_avg, t2.exp_avg) and torch.equal(t1.exp_avg_sq, t2.exp_avg_sq)


@pytest.mark.parametrize("graph", [True, False])
def test_host_fed_tree_trainer_matches_device_fed(tmp_path, graph):
    _host_fed_vs_device_fed(tmp_path, "c1", False, graph, 20)


def test_host_fed_sequential_trainer_matches_device_fed(tmp_path):
    _host_fed_vs_device_fed(tmp_path, "c1", True, "auto", 8)


def test_model_trainer_with_data_dir_trains_validates_and_resumes(tmp_path):
    from video_gcp_amd.train import ModelTrainer, get_cmd_args
    data, exp = tmp_path / "data", tmp_path / "exp"
    FX.write_random_dataset(str(data), T=20, img=32, n_files=2, traj_per_file=3, min_len=5)
    exp.mkdir()
    (exp / "conf.json").write_text('{"config": "c1", "num_epochs": 1, "epoch_cycles_train": 2}')
    argv = ["--path", str(exp), "--data_dir", str(data), "--log_outputs_interval", "1"]
    mt = ModelTrainer(get_cmd_args(argv))
    assert isinstance(mt.train_loader, DS.HostFedLoader) and mt.val_loader.ds.phase == "val"
    assert len(mt.train_loader) == 2 * (6 // 2)
    mt.run()
    torch.cuda.synchronize()
    assert mt.global_step == 6 and np.isfinite(mt.last_val) and all(np.isfinite(v) for _, v in mt.log)
    theta = mt.model.theta.clone()
    mt2 = ModelTrainer(get_cmd_args(argv + ["--resume", "latest", "--num_epochs", "2", "--skip_first_val", "1"]))
    start = mt2.resume("latest")
    assert start == 1 and mt2.global_step == 6 and torch.equal(mt2.model.theta, theta)
    mt2.train(start)
    torch.cuda.synchronize()
    assert mt2.global_step == 12 and torch.isfinite(mt2.model.theta).all()
