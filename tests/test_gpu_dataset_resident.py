"""The device-resident data path on the device: gcpx_assemble_batch_resident / gcpx_resize_assemble_batch_resident called directly,
torch.equal to the numpy assembly of the host-fed path (dataset.assemble_numpy); ResidentLoader against numpy_batches() and against
HostFedLoader; ModelTrainer with --device_dataset 1 against the same run without it; the argument checks.

Bounds are tested without ever faulting: the store handed to the kernels is a view inside a larger allocation whose bytes before and
after the view are 255, and store_bytes is the view's size.  A read outside the store, or of a neighbouring trajectory in place of
padding, then shows as a wrong value (+1.0 where -1.0 belongs)."""
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import video_gcp_amd as V  # noqa: E402
from video_gcp_amd import dataset as DS  # noqa: E402
from video_gcp_amd import dataset_resident as DR  # noqa: E402
from video_gcp_amd import runtime as rt  # noqa: E402
import dataset_fixture as FX  # noqa: E402

pytestmark = pytest.mark.gpu
KEYS = ("traj_seq", "I_0", "I_g", "pad_mask", "end_ind", "start_ind", "traj_seq_states", "actions")
GUARD = 4096
S = A = 2


def _trajectory(rng, n, Hs, Ws, fill=None):
    im = rng.randint(0, 256, size=(n, Hs, Ws, 3)).astype(np.uint8) if fill is None else np.full((n, Hs, Ws, 3), fill, dtype=np.uint8)
    return dict(images=im, states=rng.randn(n, S).astype(np.float32), actions=rng.randn(n - 1, A).astype(np.float32))


def _tables(trajs):
    """the host tables of a ResidentStore over `trajs` (what resident_info reads)"""
    n = np.array([r["images"].shape[0] for r in trajs], dtype=np.int64)
    return types.SimpleNamespace(n=n, first_frame=np.cumsum(n) - n, first_state=np.cumsum(n) - n, first_action=np.cumsum(n - 1) - (n - 1),
                                 S=S, A=A)


def _guarded(nbytes):
    """a 16-byte aligned view of nbytes inside a larger allocation, 255 before and after it; the view itself is left as allocated"""
    big = torch.empty(GUARD + nbytes + GUARD, dtype=torch.uint8, device="cuda")
    big[:GUARD] = 255
    big[GUARD + nbytes:] = 255
    view = big[GUARD:GUARD + nbytes]
    assert view.data_ptr() % 16 == 0
    return big, view


def _plan(T, offset, chop, zero_from, end_ind):
    return dict(offset=offset, chop=chop, zero_from=zero_from, end_ind=end_ind, pad_mask=(np.arange(T) <= end_ind).astype(np.float32))


def _device_args(trajs, picks, T, img):
    """the store of `trajs` inside its guards, the info and pad masks of `picks` = [(trajectory, plan)], fresh outputs"""
    dev = torch.device("cuda")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    frames = np.concatenate([r["images"] for r in trajs]).reshape(-1)
    big, view = _guarded(frames.size)
    view.copy_(t(frames))
    tab = _tables(trajs)
    B = len(picks)
    info = np.stack([DR.resident_info(tab, i, p) for i, p in picks])
    pad = np.stack([p["pad_mask"] for _, p in picks])
    Hs, Ws = trajs[0]["images"].shape[1:3]
    out = dict(traj_seq=torch.full((B, T, 3, img, img), 9.0, device=dev), I_0=torch.full((B, 3, img, img), 9.0, device=dev),
               I_g=torch.full((B, 3, img, img), 9.0, device=dev), pad_mask=torch.full((B, T), 9.0, device=dev),
               end_ind=torch.full((B,), 99, dtype=torch.int64, device=dev), start_ind=torch.full((B,), 99, dtype=torch.int64, device=dev),
               traj_seq_states=torch.full((B, T, S), 9.0, device=dev), actions=torch.full((B, T - 1, A), 9.0, device=dev))
    return dict(big=big, store=view, info=t(info), pad=t(pad), states=t(np.concatenate([r["states"] for r in trajs])),
                actions=t(np.concatenate([r["actions"] for r in trajs])), lut=t(DS.LUT), src=(Hs, Ws),
                tables=[t(x) for x in DS.resize_tables(Hs, Ws, img)], out=out, info_np=info)


def _call(d, B, T, img, resize, **over):
    """the export with the arguments of `d`, any of them replaced by `over`"""
    lib = rt.load_library()
    kx, bx, ky, by = d["tables"]
    o = d["out"]
    v = dict(store=d["store"].data_ptr(), store_bytes=d["store"].numel(), info=d["info"].data_ptr(), kx=kx.data_ptr(), ky=ky.data_ptr(),
             Hs=d["src"][0], Ws=d["src"][1], H=img, W=img, ksx=kx.shape[1], ksy=ky.shape[1])
    v.update(over)
    head = (v["store"], v["store_bytes"], v["info"], d["lut"].data_ptr())
    mid = (d["pad"].data_ptr(), d["states"].data_ptr(), d["actions"].data_ptr(), None, None, B, T)
    tail = (S, A, o["traj_seq"].data_ptr(), o["I_0"].data_ptr(), o["I_g"].data_ptr(), o["pad_mask"].data_ptr(), o["end_ind"].data_ptr(),
            o["start_ind"].data_ptr(), o["traj_seq_states"].data_ptr(), o["actions"].data_ptr(), torch.cuda.current_stream().cuda_stream)
    if resize:
        return lib.gcpx_resize_assemble_batch_resident(*head, v["kx"], bx.data_ptr(), v["ky"], by.data_ptr(), *mid, v["Hs"], v["Ws"],
                                                       v["H"], v["W"], v["ksx"], v["ksy"], *tail)
    return lib.gcpx_assemble_batch_resident(*head, *mid, v["H"], v["W"], *tail)


def _check(trajs, picks, T, img, resize):
    d = _device_args(trajs, picks, T, img)
    rt.check(_call(d, len(picks), T, img, resize), "assemble_batch_resident")
    torch.cuda.synchronize()
    ref = DS.assemble_numpy([(trajs[i], p) for i, p in picks], T, img_sz=img if resize else None)
    got = {k: v.cpu() for k, v in d["out"].items()}
    for k in KEYS:
        assert torch.equal(got[k], torch.from_numpy(ref[k])), k
    assert bool((d["big"][:GUARD] == 255).all()) and bool((d["big"][-GUARD:] == 255).all())
    return got, d


@pytest.mark.parametrize("img", [8, 5], ids=["8x8_dwords", "5x5_bytes"])
def test_plain_form_equals_the_numpy_assembly(img):
    """trajectories of 3, 6 and 9 frames back to back, the middle one all 255: the padded frames of the short one are -1.0, not the
    +1.0 of the frames behind it.  5 x 5 frames are 75 bytes: every odd frame starts off a dword."""
    T = 6
    rng = np.random.RandomState(img)
    trajs = [_trajectory(rng, 3, img, img), _trajectory(rng, 6, img, img, fill=255), _trajectory(rng, 9, img, img)]
    # offset 0 and the largest offset that still fills the window; end_ind short and at T - 1
    got, d = _check(trajs, [(0, _plan(T, 0, 0, T, 2)), (1, _plan(T, 0, 0, T, T - 1)), (2, _plan(T, 3, 0, T, T - 1))], T, img, False)
    assert bool((got["traj_seq"][0, 3:] == -1.0).all()) and bool((got["traj_seq"][1] == 1.0).all())
    assert d["info_np"][2, 0] + T == 18                                  # the window ends on the last frame of the store
    # the largest valid offset of all (one frame left, end_ind 0: I_g is I_0); chop > 0 with zero_from < T; end_ind next to 0
    got, _ = _check(trajs, [(0, _plan(T, 2, 0, T, 0)), (2, _plan(T, 0, 2, 4, 3)), (2, _plan(T, 3, 1, 2, 1))], T, img, False)
    assert bool((got["traj_seq"][0, 1:] == -1.0).all()) and torch.equal(got["I_g"][0], got["I_0"][0])
    assert bool((got["traj_seq"][1, 4:] == -1.0).all()) and bool((got["actions"][0] == 0).all())


@pytest.mark.parametrize("size", [(12, 12, 8), (8, 8, 16), (20, 12, 8), (128, 128, 64), (10, 10, 8)], ids=lambda s: f"{s[0]}x{s[1]}to{s[2]}")
def test_resize_form_equals_the_numpy_assembly(size):
    """every size: a window whose last frame is the last frame of the store (the 16-byte staging loads end on store_bytes), a chopped
    window with padding behind it, and the short trajectory in front of an all-255 one.  The frames of the first four sizes are
    multiples of 16 bytes, so there a staging load starts off a 16-byte boundary only in bands below the first (128 -> 64 has them);
    10 x 10 frames are 300 bytes and every window that starts on an odd frame has shift != 0."""
    Hs, Ws, img = size
    T = 4
    rng = np.random.RandomState(Hs * 1000 + Ws + img)
    trajs = [_trajectory(rng, 5, Hs, Ws), _trajectory(rng, 3, Hs, Ws), _trajectory(rng, 4, Hs, Ws, fill=255), _trajectory(rng, 7, Hs, Ws)]
    got, d = _check(trajs, [(0, _plan(T, 1, 1, 3, 2)), (3, _plan(T, 3, 0, T, T - 1))], T, img, True)
    assert d["info_np"][1, 0] + T == 19 and bool((got["traj_seq"][0, 3] == -1.0).all())
    if (Hs, Ws) == (10, 10):
        assert all(int(f) * Hs * Ws * 3 % 16 != 0 for f in d["info_np"][:, 0])
    got, _ = _check(trajs, [(1, _plan(T, 0, 0, T, 2)), (3, _plan(T, 0, 0, T, T - 1))], T, img, True)
    assert bool((got["traj_seq"][0, 3] == -1.0).all())                   # not the all-255 frame that follows the short trajectory


def test_addressing_past_4_gib():
    """a store of just over 4 GiB, untouched except for its first and its last trajectory; one batch takes a sequence from each end"""
    free = torch.cuda.mem_get_info()[0]
    if free < 16 * 2 ** 30:
        print(f"skipped: {free} bytes free on the device, the test wants 16 GiB")
        pytest.skip("less than 16 GiB free on the device")
    dev, T = torch.device("cuda"), 4
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    nbytes = 768 * (2 ** 32 // 768 + 16)                                 # whole 16 x 16 frames (and whole 8 x 8 ones): 4 GiB + 12 KB,
    assert nbytes > 2 ** 32                                              # the last trajectory starts past 2^32 at either frame size
    big, view = _guarded(nbytes)
    rng = np.random.RandomState(0)
    for side, img, resize in ((8, 8, False), (16, 8, True)):
        fb = side * side * 3
        N = nbytes // fb
        ends = [_trajectory(rng, 5, side, side), _trajectory(rng, 6, side, side)]
        view[:5 * fb] = t(ends[0]["images"].reshape(-1))
        view[nbytes - 6 * fb:] = t(ends[1]["images"].reshape(-1))
        picks = [(0, _plan(T, 1, 0, T, 2)), (1, _plan(T, 2, 0, T, T - 1))]
        tab = _tables(ends)
        info = np.stack([DR.resident_info(tab, i, p) for i, p in picks])
        info[1, 0] = N - 6 + 2                                           # the last trajectory lies at the end of the store
        assert info[1, 0] * fb > 2 ** 32 and (info[1, 0] + T) * fb == nbytes
        d = _device_args(ends, picks, T, img)
        d.update(big=big, store=view, info=t(info))
        rt.check(_call(d, 2, T, img, resize), "assemble_batch_resident")
        torch.cuda.synchronize()
        ref = DS.assemble_numpy([(ends[i], p) for i, p in picks], T, img_sz=img if resize else None)
        for k in KEYS:
            assert torch.equal(d["out"][k].cpu(), torch.from_numpy(ref[k])), (side, k)


def test_argument_checks_launch_nothing():
    T, img = 4, 8
    rng = np.random.RandomState(0)
    trajs = [_trajectory(rng, 6, 12, 12)]
    picks = [(0, _plan(T, 0, 0, T, T - 1)), (0, _plan(T, 2, 0, T, T - 1))]
    d = _device_args(trajs, picks, T, img)
    lib = rt.load_library()
    for resize, name in ((True, b"gcpx_resize_assemble_batch_resident"), (False, b"gcpx_assemble_batch_resident")):
        cases = [(dict(store=None), b"null"), (dict(info=None), b"null"), (dict(store_bytes=0), b"less than one frame")]
        if resize:
            cases += [(dict(W=6), b"multiple of 4"), (dict(ksx=7), b"tap counts"), (dict(ksy=3), b"tap counts"), (dict(kx=None), b"table"),
                      (dict(Hs=513), b"512"), (dict(store=d["store"].data_ptr() + 4), b"aligned")]
        for over, text in cases:
            status = _call(d, 2, T, img, resize, **over)
            err = lib.gcpx_last_error()
            assert status < 0 and name in err and text in err, (over, status, err)
    torch.cuda.synchronize()
    for k, v in d["out"].items():                                        # nothing was launched: the outputs keep their fill
        assert bool((v == (99 if v.dtype == torch.int64 else 9.0)).all()), k
    rt.check(_call(d, 2, T, img, True), "resize_assemble_batch_resident")  # and the same arguments, unchanged, run
    torch.cuda.synchronize()
    ref = DS.assemble_numpy([(trajs[i], p) for i, p in picks], T, img_sz=img)
    assert torch.equal(d["out"]["traj_seq"].cpu(), torch.from_numpy(ref["traj_seq"]))


@pytest.fixture(scope="module")
def c1_model():
    from video_gcp_amd.model import GCPTreeModel
    hp = V.config("c1")
    return hp, GCPTreeModel(hp, params=V.init_params(hp, seed=1, randomize_affine=True), device="cuda")


def _collect(loader):
    out = []
    for got in loader:
        torch.cuda.synchronize()
        out.append({k: v.cpu().clone() for k, v in got.items()})
    return out


def test_ring_reuse_five_batches_equal_the_numpy_batches(tmp_path, c1_model):
    hp, model = c1_model
    Tm, img, B = hp.max_seq_len, hp.img_sz, hp.batch_size
    FX.write_random_dataset(str(tmp_path), T=Tm, img=img, n_files=2, traj_per_file=3 * B // 2, phases=("train",), min_len=5)
    ds = DS.VideoDataset(str(tmp_path), DS.load_spec(str(tmp_path)), "train", img, randomize_length=True)
    loader = DR.ResidentLoader(ds, model, B, n_repeat=2, seed=3, n_slots=2)
    loader.set_epoch(1)
    assert len(loader) >= 5
    n = 0
    for got, ref in zip(loader, loader.numpy_batches()):
        torch.cuda.synchronize()
        for k in KEYS:
            assert got[k].data_ptr() == model.input_buffer(k, tuple(got[k].shape), got[k].dtype).data_ptr(), k   # no staging copy
            assert torch.equal(got[k].cpu(), torch.from_numpy(ref[k])), (n, k)
        n += 1
    assert n == len(loader) >= 5


def test_three_slot_ring_of_both_loaders_equals_the_numpy_batches(tmp_path, c1_model):
    """n_slots = 3 with fewer batches than slots (2) and with a slot reused (4), through the one ring of dataset.RingLoader"""
    hp, model = c1_model
    Tm, img, B = hp.max_seq_len, hp.img_sz, hp.batch_size
    FX.write_random_dataset(str(tmp_path), T=Tm, img=img, n_files=2, traj_per_file=B, phases=("train",), min_len=5)
    ds = DS.VideoDataset(str(tmp_path), DS.load_spec(str(tmp_path)), "train", img, randomize_length=True)
    for n_repeat in (1, 2):
        for loader in (DS.HostFedLoader(ds, model, B, n_repeat=n_repeat, seed=5, n_slots=3, n_workers=3),
                       DR.ResidentLoader(ds, model, B, n_repeat=n_repeat, seed=5, n_slots=3)):
            assert len(loader) == 2 * n_repeat
            n = 0
            for got, ref in zip(loader, loader.numpy_batches()):
                torch.cuda.synchronize()
                assert set(got) == set(KEYS)
                for k in KEYS:
                    assert got[k].data_ptr() == model.input_buffer(k, tuple(got[k].shape), got[k].dtype).data_ptr(), k
                    assert torch.equal(got[k].cpu(), torch.from_numpy(ref[k])), (type(loader).__name__, n_repeat, n, k)
                n += 1
            assert n == len(loader)


@pytest.mark.parametrize("resize,rl,rs,std", [(False, True, False, True), (False, False, True, False), (True, True, False, False)],
                         ids=["length_std", "start", "resize_length"])
def test_loader_equals_the_host_fed_loader(tmp_path, c1_model, resize, rl, rs, std):
    hp, model = c1_model
    Tm, img, B = hp.max_seq_len, hp.img_sz, hp.batch_size
    FX.write_random_dataset(str(tmp_path), T=Tm, img=2 * img if resize else img, n_files=2, traj_per_file=3 * B // 2, min_len=5)
    spec = DS.load_spec(str(tmp_path))
    if std:
        spec.update(states_mean=FX.STATES_MEAN, states_std=FX.STATES_STD)
    for phase in ("train", "val"):
        ds = DS.VideoDataset(str(tmp_path), spec, phase, img, randomize_length=rl, randomize_start=rs, resize=resize)
        host = DS.HostFedLoader(ds, model, B, n_repeat=2, seed=3, n_slots=2, n_workers=3)
        res = DR.ResidentLoader(ds, model, B, n_repeat=2, seed=3, n_slots=2)
        assert res.shuffle == (phase == "train") and (res.store.Hs == 2 * img) == resize
        host.set_epoch(1)
        res.set_epoch(1)
        want, got = _collect(host), _collect(res)
        assert len(want) == len(got) == len(res) > 1
        for n, (w, g) in enumerate(zip(want, got)):
            assert set(w) == set(g) == set(KEYS)
            for k in KEYS:
                assert torch.equal(w[k], g[k]), (phase, n, k)


def test_model_trainer_with_device_dataset_logs_the_same_losses(tmp_path):
    from video_gcp_amd.train import ModelTrainer, get_cmd_args
    data = tmp_path / "data"
    FX.write_random_dataset(str(data), T=20, img=32, n_files=2, traj_per_file=3, min_len=5)
    runs = []
    for flag in ("0", "1"):
        exp = tmp_path / f"exp{flag}"
        exp.mkdir()
        (exp / "conf.json").write_text('{"config": "c1", "num_epochs": 1}')
        mt = ModelTrainer(get_cmd_args(["--path", str(exp), "--data_dir", str(data), "--log_outputs_interval", "1", "--dont_save", "1",
                                        "--device_dataset", flag]))
        assert isinstance(mt.train_loader, DR.ResidentLoader if flag == "1" else DS.HostFedLoader)
        assert type(mt.val_loader) is type(mt.train_loader) and mt.val_loader.ds.phase == "val"
        mt.model._rng_stream_id = 0             # the two trainers draw the same in-plan noise
        torch.cuda.manual_seed(11)
        mt.model.reseed(11)
        mt.run()
        torch.cuda.synchronize()
        runs.append((list(mt.log), mt.last_val, mt.model.theta.clone()))
    (log0, val0, th0), (log1, val1, th1) = runs
    assert len(log0) == 3 and all(np.isfinite(v) for _, v in log0)
    assert log0 == log1 and val0 == val1 and torch.equal(th0, th1)
    exp = tmp_path / "exp_small"
    exp.mkdir()
    (exp / "conf.json").write_text('{"config": "c1"}')
    with pytest.raises(ValueError, match="needs [0-9]+ bytes"):
        ModelTrainer(get_cmd_args(["--path", str(exp), "--data_dir", str(data), "--device_dataset", "1", "--device_dataset_gb", "0.0001"]))
