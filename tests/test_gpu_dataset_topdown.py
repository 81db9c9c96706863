"""The nav datasets' top-down frames on the device: gcpx_topdown_assemble_batch, called directly, equal to the numpy assembly (itself pinned
to a literal restatement of the reference's renderer, tests/test_dataset_topdown_cpu.py) under every branch of the time map, with dots at
the picture's border, clamped crops, overlapping and far-away goals, and at the c2 batch shape; its argument checks; HostFedLoader over the
image-less fixture dataset; ModelTrainer on it (train, validate, resume, --metric)."""
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
import topdown_fixture as TF  # noqa: E402

pytestmark = pytest.mark.gpu
KEYS = ("traj_seq", "I_0", "I_g", "pad_mask", "end_ind", "start_ind", "traj_seq_states", "actions")


def _assets(arrays):
    a = dict(background=arrays["background"], cw=int(arrays["crop_window"]), n_rooms=int(arrays["n_rooms"]),
             scale=int(arrays["render_scale"]), agent_stamp=arrays["agent_stamp"], goal_stamp=arrays["goal_stamp"],
             agent_color=arrays["agent_color"], goal_color=arrays["goal_color"])
    a["S"] = int(DS.topdown_table_size(a["n_rooms"]) * a["scale"])
    return a


def _device_args(items, T, a, img, S, A):
    """pack on the host and upload (stale values in the staging slot and in the outputs on purpose): everything the export reads"""
    B = len(items)
    coords = np.full(B * T * 2 + B * 2, 2 ** 30, dtype=np.int32)
    aux = np.full(B * T + B * T * S + B * (T - 1) * A, 5.0, dtype=np.float32)
    info = np.zeros((B, DS.N_INFO), dtype=np.int32)
    for j, it in enumerate(items):
        DS.pack_item(it, j, coords, aux, info, B, T, S, A, topdown=a)
    dev = torch.device("cuda")
    t = lambda x: torch.from_numpy(x).to(dev)
    out = dict(traj_seq=torch.full((B, T, 3, img, img), 9.0, device=dev), I_0=torch.full((B, 3, img, img), 9.0, device=dev),
               I_g=torch.full((B, 3, img, img), 9.0, device=dev), pad_mask=torch.full((B, T), 9.0, device=dev),
               end_ind=torch.full((B,), 99, dtype=torch.int64, device=dev), start_ind=torch.full((B,), 99, dtype=torch.int64, device=dev),
               traj_seq_states=torch.full((B, T, S), 9.0, device=dev), actions=torch.full((B, T - 1, A), 9.0, device=dev))
    return dict(assets=DS.topdown_device_assets(a, img, dev), coords=t(coords), aux=t(aux), info=t(info), lut=t(DS.LUT), out=out)


def _call(d, B, T, img, S, A, **over):
    """the export with the arguments of `d`, any of them replaced by `over`"""
    lib = rt.load_library()
    da = d["assets"]
    kx, bx, ky, by = da["tables"]
    a, c, o = d["aux"].data_ptr(), d["coords"].data_ptr(), d["out"]
    v = dict(background=da["background"].data_ptr(), side=da["background"].shape[0], cw=da["cw"], agent_stamp=da["agent_stamp"].data_ptr(),
             goal_stamp=da["goal_stamp"].data_ptr(), k=da["k"], coords=c, goal=c + 4 * B * T * 2, kx=kx.data_ptr(), bx=bx.data_ptr(),
             ky=ky.data_ptr(), by=by.data_ptr(), H=img, W=img, ksx=kx.shape[1], ksy=ky.shape[1], traj_seq=o["traj_seq"].data_ptr(),
             I_g=o["I_g"].data_ptr())
    v.update(over)
    return lib.gcpx_topdown_assemble_batch(v["background"], v["side"], v["cw"], v["agent_stamp"], v["goal_stamp"], v["k"], da["agent_rgb"],
                                           da["goal_rgb"], v["coords"], v["goal"], d["info"].data_ptr(), d["lut"].data_ptr(), v["kx"],
                                           v["bx"], v["ky"], v["by"], a, a + 4 * B * T if S else None,
                                           a + 4 * B * T * (1 + S) if A else None, None, None, B, T, v["H"], v["W"], v["ksx"], v["ksy"], S,
                                           A, v["traj_seq"], o["I_0"].data_ptr(), v["I_g"], o["pad_mask"].data_ptr(),
                                           o["end_ind"].data_ptr(), o["start_ind"].data_ptr(),
                                           o["traj_seq_states"].data_ptr() if S else None, o["actions"].data_ptr() if A else None,
                                           torch.cuda.current_stream().cuda_stream)


def _assemble_on_device(items, T, a, img, S, A):
    d = _device_args(items, T, a, img, S, A)
    rt.check(_call(d, len(items), T, img, S, A), "topdown_assemble_batch")
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in d["out"].items()}


def _walk(rng, a, n, start, k):
    """n picture pixels: a walk of small steps from `start`, kept where every crop fits ([-k, S + cw] on both axes)"""
    steps = rng.randint(-2, 3, size=(n, 2))
    steps[0] = 0
    return np.clip(np.asarray(start) + np.cumsum(steps, axis=0), -(k // 2), a["S"] + a["cw"])


def _item(rng, a, n, start, offset, chop, zero_from, end_ind, T):
    k = a["agent_stamp"].shape[0]
    pix = _walk(rng, a, n, start, k)
    st = TF.states_for_pixels(pix, a["n_rooms"], a["scale"], a["S"], a["cw"])
    assert np.array_equal(DS.topdown_pixels(st, a["n_rooms"], a["scale"], a["S"], a["cw"]), pix)
    raw = dict(states=st, actions=rng.randn(n - 1, 2).astype(np.float32), name=f"item@{start}")
    return raw, dict(offset=offset, chop=chop, zero_from=zero_from, end_ind=end_ind, pad_mask=(np.arange(T) <= end_ind).astype(np.float32))


def _time_map_items(case, rng, a, T):
    """B = 3 sequences per branch of the time map; one starts in the picture's corner (stamps cut by the border, clamped crops), one at
    the far corner, one inside; the walks are short, so late frames have the goal's dot on the agent's"""
    S, cw = a["S"], a["cw"]
    starts = ((0, 1), (S + cw - 1, S + cw), (cw + S // 2, cw + S // 3))
    if case == "full":                  # the window lies inside the recording, every frame rendered, I_g is the last frame
        return [_item(rng, a, T + 3, s, o, 0, T, T - 1, T) for s, o in zip(starts, (0, 2, 3))]
    if case == "short":                 # fewer states than T: frames past them are zero (-1.0)
        return [_item(rng, a, n, s, o, 0, T, n - o - 1, T) for s, (n, o) in zip(starts, ((4, 0), (5, 2), (T - 1, 0)))]
    if case == "chop":                  # randomize_length: chop > 0, frames from zero_from on are zero
        return [_item(rng, a, n, s, 0, c, z, z - 1, T) for s, (n, c, z) in zip(starts, ((T, 2, 4), (T + 2, 3, 3), (5, 1, 3)))]
    assert case == "ends"               # end_ind == 0 (I_g is I_0); end_ind < T - 1 with states behind it (kept; their frames are not
    return [_item(rng, a, T, starts[0], 0, 0, 1, 0, T), _item(rng, a, T, starts[1], 0, 0, T, 2, T),     # rendered); end_ind == T - 1
            _item(rng, a, T, starts[2], 0, 2, T, T - 1, T)]


# (cw, img): 2cw = 12 -> 8 with an odd cw and rows of 36 bytes; 32 -> 32, both passes identities; 40 -> 32; the nav datasets' 80 -> 64
SIZES = [(6, 8), (16, 32), (20, 32), (40, 64)]


@pytest.mark.parametrize("case", ["full", "short", "chop", "ends"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"cw{s[0]}to{s[1]}")
def test_export_equals_the_numpy_assembly(size, case):
    cw, img = size
    T = 7
    a = _assets(TF.make_assets(seed=cw, scale=3 * cw + 1, cw=cw, k=7 if cw < 40 else 11))
    items = _time_map_items(case, np.random.RandomState(cw * 100 + img), a, T)
    ref = DS.assemble_numpy(items, T, img_sz=img, topdown=a)
    assert ref["traj_seq"].shape == (3, T, 3, img, img)
    got = _assemble_on_device(items, T, a, img, 2, 2)
    for k in KEYS:
        assert torch.equal(got[k], torch.from_numpy(ref[k])), (size, case, k)
    if case != "full":
        assert bool((got["traj_seq"] == -1.0).all(dim=(2, 3, 4)).any())
    if case == "ends":
        assert torch.equal(got["I_g"][0], got["I_0"][0]) and torch.equal(got["I_g"][2], got["traj_seq"][2, T - 1])
        assert bool((got["traj_seq_states"][1, 3:] != 0).any()) and bool((got["traj_seq"][1, 3:] == -1.0).all())


def test_export_equals_the_numpy_assembly_at_the_c2_batch_shape(tmp_path):
    hp = V.config("c2")
    T, img, B = hp.max_seq_len, hp.img_sz, hp.batch_size
    assert (T, img, B) == (80, 64, 16)
    TF.write_topdown_dataset(str(tmp_path), T=T, n_files=2, traj_per_file=B, seed=8, min_len=6, split=(1.0, 0.0, 0.0), n_rooms=25, cw=40)
    ds = DS.VideoDataset(str(tmp_path), DS.load_spec(str(tmp_path)), "train", img, randomize_length=True)
    assert ds.topdown["S"] == 426 and ds.topdown["background"].shape == (506, 506, 3) and ds.src_size == (80, 80)
    batch = DS.epoch_schedule(len(ds), B, 1, seed=4, epoch=0, shuffle=True)[0]
    ref = DS.numpy_batch(ds, batch, 4)
    got = _assemble_on_device([ds.item(i, DS.item_rng(4, c, p)) for i, p, c in batch], T, ds.topdown, img, 2, 2)
    assert len(set(ref["end_ind"].tolist())) > 1
    for k in KEYS:
        assert torch.equal(got[k], torch.from_numpy(ref[k])), k


def test_argument_checks_launch_nothing():
    T, cw, img = 7, 20, 32
    a = _assets(TF.make_assets(seed=1, scale=64, cw=cw, k=7))
    items = _time_map_items("full", np.random.RandomState(0), a, T)
    d = _device_args(items, T, a, img, 2, 2)
    lib = rt.load_library()
    k5 = DS.resize_ksize(40, 32)
    for over, text in ((dict(kx=None), b"table"), (dict(ky=None), b"table"), (dict(bx=None), b"table"), (dict(by=None), b"table"),
                       (dict(background=None), b"background"), (dict(agent_stamp=None), b"stamp"), (dict(coords=None), b"coordinate"),
                       (dict(cw=1), b"[4, 128]"), (dict(cw=65, side=400), b"[4, 128]"), (dict(W=30), b"multiple of 4"),
                       (dict(k=8), b"odd"), (dict(k=33), b"at most 31"), (dict(ksx=k5 + 2), b"tap counts"), (dict(ksy=k5 - 2), b"tap counts"),
                       (dict(traj_seq=d["out"]["traj_seq"].data_ptr() + 4), b"aligned"), (dict(I_g=d["out"]["I_g"].data_ptr() + 8), b"aligned"),
                       (dict(background=d["assets"]["background"].data_ptr() + 1), b"aligned"), (dict(side=2 * cw - 1), b"side"),
                       (dict(H=516, W=516), b"512")):
        status = _call(d, 3, T, img, 2, 2, **over)
        err = lib.gcpx_last_error()
        assert status < 0 and b"gcpx_topdown_assemble_batch" in err and text in err, (over, status, err)
    torch.cuda.synchronize()
    for k, v in d["out"].items():                                           # nothing was launched: the outputs keep their fill
        assert bool((v == (99 if v.dtype == torch.int64 else 9.0)).all()), k
    rt.check(_call(d, 3, T, img, 2, 2), "topdown_assemble_batch")             # and the same arguments, unchanged, run
    torch.cuda.synchronize()
    ref = DS.assemble_numpy(items, T, img_sz=img, topdown=a)
    for k in KEYS:
        assert torch.equal(d["out"][k].cpu(), torch.from_numpy(ref[k])), k


def _tree_model(name):
    from video_gcp_amd.model import GCPTreeModel
    hp = V.config(name)
    return hp, GCPTreeModel(hp, params=V.init_params(hp, seed=1, randomize_affine=True), device="cuda")


def test_host_fed_loader_renders_into_the_input_buffers(tmp_path):
    hp, model = _tree_model("c1")
    T, img, B = hp.max_seq_len, hp.img_sz, hp.batch_size
    TF.write_topdown_dataset(str(tmp_path), T=T, n_files=2, traj_per_file=B + B // 2, seed=5, min_len=5, split=(1.0, 0.0, 0.0), scale=64,
                             cw=20, k=7)
    ds = DS.VideoDataset(str(tmp_path), DS.load_spec(str(tmp_path)), "train", img, randomize_length=True)
    loader = DS.HostFedLoader(ds, model, B, n_repeat=1, seed=3, n_slots=2, n_workers=3)
    assert loader.shuffle and len(loader) == 3 and loader.S == 2
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
    pin, devs = loader.pin, loader.dev
    assert "frames" not in pin and "frames" not in devs                       # no frame buffer: a slot holds coordinates
    assert devs["coords"][0].shape == (B * T * 2 + B * 2,) and devs["coords"][0].dtype == torch.int32
    assert not any(v.dtype == torch.uint8 and v.numel() >= B * T * 3 * img * img for vs in list(pin.values()) + list(devs.values()) for v in vs)


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


def test_model_trainer_on_a_top_rendered_dataset(tmp_path):
    from video_gcp_amd.train import ModelTrainer, get_cmd_args
    data, exp = tmp_path / "data", tmp_path / "exp"
    TF.write_topdown_dataset(str(data), T=20, n_files=4, traj_per_file=3, seed=6, min_len=5, scale=64, cw=20, k=7)
    exp.mkdir()
    (exp / "conf.json").write_text('{"config": "c1", "num_epochs": 1, "epoch_cycles_train": 2}')
    argv = ["--path", str(exp), "--data_dir", str(data), "--log_outputs_interval", "1"]
    mt = ModelTrainer(get_cmd_args(argv))                                    # no flag: the dataset_spec.py names Nav9Rooms
    assert isinstance(mt.train_loader, DS.HostFedLoader) and mt.train_loader.ds.topdown is not None and mt.val_loader.ds.phase == "val"
    assert mt.train_loader.ds.src_size == (40, 40) and mt.model._hp.img_sz == 32 and len(mt.train_loader.ds) == 6
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
    # two host-fed steps against the same batches rendered and assembled by numpy and fed from the device: only the feeding differs
    ds = mt.train_loader.ds
    _, m1, t1 = _trainer("c1")
    loader = DS.HostFedLoader(ds, m1, 2, n_repeat=1, seed=3, n_slots=2, n_workers=3)
    l1 = _run(m1, t1, loader, 2)
    _, m2, t2 = _trainer("c1")
    l2 = _run(m2, t2, [{k: torch.from_numpy(v).cuda() for k, v in b.items()} for b in loader.numpy_batches()], 2)
    assert len(l1) == len(l2) == 2 and all(torch.isfinite(x).all() for x in l1)
    assert all(torch.equal(a, b) for a, b in zip(l1, l2))
    assert torch.equal(m1.theta, m2.theta) and torch.equal(t1.exp_avg, t2.exp_avg) and torch.equal(t1.exp_avg_sq, t2.exp_avg_sq)


def test_metric_pass_on_a_top_rendered_dataset_writes_its_results(tmp_path):
    from video_gcp_amd.train import ModelTrainer, get_cmd_args
    data, exp = tmp_path / "data", tmp_path / "exp"
    TF.write_topdown_dataset(str(data), T=20, n_files=4, traj_per_file=3, seed=7, min_len=6, scale=64, cw=20, k=7)
    exp.mkdir()
    (exp / "conf.json").write_text('{"config": "c1"}')
    tr = ModelTrainer(get_cmd_args(["--path", str(exp), "--data_dir", str(data), "--metric", "1", "--top_of", "3"]))
    assert tr.val_loader.ds.phase == "test" and tr.val_loader.ds.topdown is not None and not tr.val_loader.shuffle
    tr.run()
    torch.cuda.synchronize()
    z = np.load(os.path.join(str(exp), "metrics", "results_0.npz"))
    S = len(tr.val_loader) * tr.model._hp.batch_size
    assert S > 0 and z["mse"].shape == (S, 3) and np.isfinite(z["mse"]).all()
    assert os.path.exists(os.path.join(str(exp), "metrics", "results_0.txt"))
    gt = np.load(os.path.join(str(exp), "metrics", "gt_seq", "it_0", "gt_seq_0.npy"))
    assert gt.shape[-3:] == (3, 32, 32)
