"""Resizing in the device-side batch assembly: gcpx_resize_assemble_batch, called directly, equal to the numpy assembly with resizing
(itself bit-identical to Pillow, tests/test_dataset_resize_cpu.py) for every size pair of tests/golden/pil_resize.npz under every branch
of the time map and at the c2 batch shape; its argument checks; HostFedLoader over a dataset stored at twice the model's size;
ModelTrainer with --resize_frames 1 (train, validate, resume, --metric) and without it."""
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
SIZES = sorted({tuple(int(x) for x in c[:3]) for c in np.load(os.path.join(ROOT, "tests", "golden", "pil_resize.npz"))["cases"]})


def _device_args(items, T, Hs, Ws, img, S, A):
    """pack on the host and upload (stale bytes in the staging slot and in the outputs on purpose): everything the export reads"""
    B = len(items)
    frames = np.full((B, T, Hs, Ws, 3), 77, dtype=np.uint8)
    aux = np.full(B * T + B * T * S + B * (T - 1) * A, 5.0, dtype=np.float32)
    info = np.zeros((B, DS.N_INFO), dtype=np.int32)
    for j, it in enumerate(items):
        DS.pack_item(it, j, frames, aux, info, B, T, S, A)
    dev = torch.device("cuda")
    t = lambda a: torch.from_numpy(a).to(dev)
    out = dict(traj_seq=torch.full((B, T, 3, img, img), 9.0, device=dev), I_0=torch.full((B, 3, img, img), 9.0, device=dev),
               I_g=torch.full((B, 3, img, img), 9.0, device=dev), pad_mask=torch.full((B, T), 9.0, device=dev),
               end_ind=torch.full((B,), 99, dtype=torch.int64, device=dev), start_ind=torch.full((B,), 99, dtype=torch.int64, device=dev),
               traj_seq_states=torch.full((B, T, S), 9.0, device=dev), actions=torch.full((B, T - 1, A), 9.0, device=dev))
    return dict(frames=t(frames), aux=t(aux), info=t(info), lut=t(DS.LUT), tables=[t(x) for x in DS.resize_tables(Hs, Ws, img)], out=out)


def _call(d, B, T, src, img, S, A, **over):
    """the export with the arguments of `d`, any of them replaced by `over`"""
    lib = rt.load_library()
    kx, bx, ky, by = d["tables"]
    a, o = d["aux"].data_ptr(), d["out"]
    v = dict(frames=d["frames"].data_ptr(), info=d["info"].data_ptr(), lut=d["lut"].data_ptr(), kx=kx.data_ptr(), bx=bx.data_ptr(),
             ky=ky.data_ptr(), by=by.data_ptr(), Hs=src[0], Ws=src[1], H=img, W=img, ksx=kx.shape[1], ksy=ky.shape[1],
             traj_seq=o["traj_seq"].data_ptr())
    v.update(over)
    return lib.gcpx_resize_assemble_batch(v["frames"], v["info"], v["lut"], v["kx"], v["bx"], v["ky"], v["by"], a, a + 4 * B * T if S else None,
                                          a + 4 * B * T * (1 + S) if A else None, None, None, B, T, v["Hs"], v["Ws"], v["H"], v["W"],
                                          v["ksx"], v["ksy"], S, A, v["traj_seq"], o["I_0"].data_ptr(), o["I_g"].data_ptr(),
                                          o["pad_mask"].data_ptr(), o["end_ind"].data_ptr(), o["start_ind"].data_ptr(),
                                          o["traj_seq_states"].data_ptr() if S else None, o["actions"].data_ptr() if A else None,
                                          torch.cuda.current_stream().cuda_stream)


def _assemble_on_device(items, T, Hs, Ws, img, S, A):
    d = _device_args(items, T, Hs, Ws, img, S, A)
    rt.check(_call(d, len(items), T, (Hs, Ws), img, S, A), "resize_assemble_batch")
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in d["out"].items()}


def _item(rng, n, Hs, Ws, offset, chop, zero_from, end_ind, T, saturated=False):
    im = (rng.randint(0, 2, size=(n, Hs, Ws, 3)) * 255 if saturated else rng.randint(0, 256, size=(n, Hs, Ws, 3))).astype(np.uint8)
    raw = dict(images=im, states=rng.randn(n, 2).astype(np.float32), actions=rng.randn(n - 1, 2).astype(np.float32))
    return raw, dict(offset=offset, chop=chop, zero_from=zero_from, end_ind=end_ind, pad_mask=(np.arange(T) <= end_ind).astype(np.float32))


def _time_map_items(case, rng, Hs, Ws, T):
    """B = 3 sequences per branch of the time map"""
    if case == "full":                  # the window lies inside the recording, every frame valid, I_g is the last frame
        return [_item(rng, T + 3, Hs, Ws, o, 0, T, T - 1, T, saturated=o == 2) for o in (0, 2, 3)]
    if case == "short":                 # n_frames < T: frames past the recording are padding (-1.0)
        return [_item(rng, n, Hs, Ws, o, 0, T, n - o - 1, T) for n, o in ((4, 0), (5, 2), (T - 1, 0))]
    if case == "chop":                  # randomize_length: chop > 0, frames from zero_from on are zero, the last frame repeats
        return [_item(rng, n, Hs, Ws, 0, c, z, z - 1, T) for n, c, z in ((T, 2, 4), (T + 2, 3, 3), (5, 1, 6))]
    assert case == "ends"               # end_ind == 0 (I_g is I_0) and == T - 1, with and without a chop
    return [_item(rng, T, Hs, Ws, 0, 0, 1, 0, T), _item(rng, T, Hs, Ws, 0, 0, T, T - 1, T), _item(rng, T, Hs, Ws, 0, 2, T, T - 1, T)]


@pytest.mark.parametrize("case", ["full", "short", "chop", "ends"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}to{s[2]}")
def test_export_equals_the_numpy_assembly(size, case):
    Hs, Ws, img = size
    T = 7
    items = _time_map_items(case, np.random.RandomState(Hs * 1000 + Ws + img), Hs, Ws, T)
    ref = DS.assemble_numpy(items, T, img_sz=img)
    assert ref["traj_seq"].shape == (3, T, 3, img, img)
    got = _assemble_on_device(items, T, Hs, Ws, img, 2, 2)
    for k in KEYS:
        assert torch.equal(got[k], torch.from_numpy(ref[k])), (size, case, k)
    if case in ("short", "chop"):
        assert bool((got["traj_seq"] == -1.0).all(dim=(2, 3, 4)).any())
    if case == "ends":
        assert torch.equal(got["I_g"][0], got["I_0"][0]) and torch.equal(got["I_g"][1], got["traj_seq"][1, T - 1])


@pytest.mark.parametrize("rl", [True, False])
def test_export_equals_the_numpy_assembly_at_the_c2_batch_shape(tmp_path, rl):
    hp = V.config("c2")
    T, img, B = hp.max_seq_len, hp.img_sz, hp.batch_size
    assert (T, img, B) == (80, 64, 16)
    FX.write_random_dataset(str(tmp_path), T=T, img=128, n_files=1, traj_per_file=B, phases=("train",), min_len=4)
    ds = DS.VideoDataset(str(tmp_path), DS.load_spec(str(tmp_path)), "train", img, randomize_length=rl, resize=True)
    assert ds.src_size == (128, 128)
    batch = DS.epoch_schedule(len(ds), B, 1, seed=4, epoch=0, shuffle=True)[0]
    ref = DS.numpy_batch(ds, batch, 4)
    got = _assemble_on_device([ds.item(i, DS.item_rng(4, c, p)) for i, p, c in batch], T, 128, 128, img, 2, 2)
    assert len(set(ref["end_ind"].tolist())) > 1
    for k in KEYS:
        assert torch.equal(got[k], torch.from_numpy(ref[k])), k


def test_argument_checks_launch_nothing():
    T, Hs, Ws, img = 7, 32, 32, 16
    items = _time_map_items("full", np.random.RandomState(0), Hs, Ws, T)
    d = _device_args(items, T, Hs, Ws, img, 2, 2)
    lib = rt.load_library()
    for over, text in ((dict(kx=None), b"table"), (dict(ky=None), b"table"), (dict(bx=None), b"table"), (dict(by=None), b"table"),
                       (dict(Hs=513), b"512"), (dict(Ws=520), b"512"), (dict(H=516, W=516), b"512"),
                       (dict(Hs=16 * 9, ksy=2 * 9 + 1), b"more than 8"), (dict(W=18), b"multiple of 4"), (dict(ksx=7), b"tap counts"),
                       (dict(frames=d["frames"].data_ptr() + 1), b"aligned"), (dict(traj_seq=d["out"]["traj_seq"].data_ptr() + 4), b"aligned")):
        status = _call(d, 3, T, (Hs, Ws), img, 2, 2, **over)
        err = lib.gcpx_last_error()
        assert status < 0 and b"gcpx_resize_assemble_batch" in err and text in err, (over, status, err)
    torch.cuda.synchronize()
    for k, v in d["out"].items():                                           # nothing was launched: the outputs keep their fill
        assert bool((v == (99 if v.dtype == torch.int64 else 9.0)).all()), k
    rt.check(_call(d, 3, T, (Hs, Ws), img, 2, 2), "resize_assemble_batch")    # and the same arguments, unchanged, run
    torch.cuda.synchronize()
    ref = DS.assemble_numpy(items, T, img_sz=img)
    assert torch.equal(d["out"]["traj_seq"].cpu(), torch.from_numpy(ref["traj_seq"]))


def _tree_model(name):
    from video_gcp_amd.model import GCPTreeModel
    hp = V.config(name)
    return hp, GCPTreeModel(hp, params=V.init_params(hp, seed=1, randomize_affine=True), device="cuda")


@pytest.mark.parametrize("name", ["c1", "c2"])
def test_host_fed_loader_resizes_into_the_input_buffers(tmp_path, name):
    hp, model = _tree_model(name)
    T, img, B = hp.max_seq_len, hp.img_sz, hp.batch_size
    FX.write_random_dataset(str(tmp_path), T=T, img=2 * img, n_files=2, traj_per_file=B + B // 2, phases=("train",), min_len=5)
    ds = DS.VideoDataset(str(tmp_path), DS.load_spec(str(tmp_path)), "train", img, randomize_length=True, resize=True)
    assert ds.src_size == (2 * img, 2 * img)
    loader = DS.HostFedLoader(ds, model, B, n_repeat=1, seed=3, n_slots=2, n_workers=3)
    assert loader.shuffle and len(loader) == 3
    orders = []
    for epoch in range(2):
        loader.set_epoch(epoch)
        orders.append([i for b in loader.schedule() for i, _, _ in b])
        n = 0
        for got, ref in zip(loader, loader.numpy_batches()):
            torch.cuda.synchronize()
            for k in KEYS:
                assert got[k].data_ptr() == model.input_buffer(k, tuple(got[k].shape), got[k].dtype).data_ptr(), k   # no staging copy
                assert torch.equal(got[k].cpu(), torch.from_numpy(ref[k])), (epoch, n, k)
            n += 1
        assert n == 3
    assert orders[0] != orders[1]
    assert loader.dev["frames"][0].shape == (B, T, 2 * img, 2 * img, 3)        # uploaded at the stored size


def _trainer(name):
    from video_gcp_amd.training import GCPTrainStep
    hp, model = _tree_model(name)
    model.use_graph = True
    model._rng_stream_id = 0                    # the two trainers draw the same in-plan noise after reseed()
    return hp, model, GCPTrainStep(model, lr=1e-3)


def _run(model, tr, batches, steps):
    torch.cuda.manual_seed(11)
    model.reseed(11)
    losses = []
    for inputs in batches:
        out = tr.step(inputs)
        losses.append(out.raw["losses"].clone())
        model.step()
        if len(losses) == steps:
            break
    torch.cuda.synchronize()
    return [x.cpu() for x in losses]


def test_model_trainer_resizes_with_the_flag_and_raises_without(tmp_path):
    from video_gcp_amd.train import ModelTrainer, get_cmd_args
    data, exp = tmp_path / "data", tmp_path / "exp"
    FX.write_random_dataset(str(data), T=20, img=64, n_files=2, traj_per_file=3, phases=("train", "val", "test"), min_len=5)
    exp.mkdir()
    (exp / "conf.json").write_text('{"config": "c1", "num_epochs": 1, "epoch_cycles_train": 2}')
    argv = ["--path", str(exp), "--data_dir", str(data), "--log_outputs_interval", "1"]
    with pytest.raises(ValueError, match="resize_video"):
        ModelTrainer(get_cmd_args(argv))
    argv += ["--resize_frames", "1"]
    mt = ModelTrainer(get_cmd_args(argv))
    assert isinstance(mt.train_loader, DS.HostFedLoader) and mt.train_loader.ds.resize and mt.val_loader.ds.resize
    assert mt.train_loader.ds.src_size == (64, 64) and mt.model._hp.img_sz == 32 and mt.val_loader.ds.phase == "val"
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
    # two host-fed steps against the same batches resized and assembled by numpy and fed from the device: only the feeding differs
    ds = mt.train_loader.ds
    _, m1, t1 = _trainer("c1")
    loader = DS.HostFedLoader(ds, m1, 2, n_repeat=1, seed=3, n_slots=2, n_workers=3)
    l1 = _run(m1, t1, loader, 2)
    _, m2, t2 = _trainer("c1")
    l2 = _run(m2, t2, [{k: torch.from_numpy(v).cuda() for k, v in b.items()} for b in loader.numpy_batches()], 2)
    assert len(l1) == len(l2) == 2 and all(torch.isfinite(x).all() for x in l1)
    assert all(torch.equal(a, b) for a, b in zip(l1, l2))
    assert torch.equal(m1.theta, m2.theta) and torch.equal(t1.exp_avg, t2.exp_avg) and torch.equal(t1.exp_avg_sq, t2.exp_avg_sq)


def test_metric_pass_on_a_resized_dataset_writes_its_results(tmp_path):
    from video_gcp_amd.train import ModelTrainer, get_cmd_args
    data, exp = tmp_path / "data", tmp_path / "exp"
    FX.write_random_dataset(str(data), T=20, img=64, n_files=2, traj_per_file=3, seed=3, phases=("train", "val", "test"), min_len=6)
    exp.mkdir()
    (exp / "conf.json").write_text('{"config": "c1"}')
    argv = ["--path", str(exp), "--data_dir", str(data), "--metric", "1", "--top_of", "3"]
    with pytest.raises(ValueError, match="resize_video"):
        ModelTrainer(get_cmd_args(argv))
    tr = ModelTrainer(get_cmd_args(argv + ["--resize_frames", "1"]))
    assert tr.val_loader.ds.phase == "test" and tr.val_loader.ds.resize and not tr.val_loader.shuffle
    tr.run()
    torch.cuda.synchronize()
    z = np.load(os.path.join(str(exp), "metrics", "results_0.npz"))
    S = len(tr.val_loader) * tr.model._hp.batch_size
    assert z["mse"].shape == (S, 3) and np.isfinite(z["mse"]).all() and os.path.exists(os.path.join(str(exp), "metrics", "results_0.txt"))
    gt = np.load(os.path.join(str(exp), "metrics", "gt_seq", "it_0", "gt_seq_0.npy"))
    assert gt.shape[-3:] == (3, 32, 32)
