"""-m gpu: picture logs composed on the device (csrc/panel.hip, video-gcp_amd/image_log.py).

  * gcpx_panel_compose called directly on the inputs of tests/golden/ref_image_log.npz equals the canvases the reference's own logger
    computed, exactly, as f32 and as uint8 -- with two nodes of one level on the same time step and a masked tail among them;
  * every panel of a c1-sized balanced model, a c5s adaptive + attentive model and a small sequential model, composed on the device,
    equals the numpy restatement (visualization.compose) of the same outputs copied to the host, f32 and uint8 exactly;
  * a three-step ModelTrainer run with --log_images 1 writes the expected files, which decode to the composed canvases; the same run
    without the flag writes no images/ directory, and the losses of the two runs are bit-equal."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from video_gcp_amd import image_log as IL  # noqa: E402
from video_gcp_amd import runtime as rt  # noqa: E402
from video_gcp_amd import visualization as V  # noqa: E402
import image_log_fixture as FX  # noqa: E402
from helpers import make_inputs  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = FX.golden_cases()


def _device_compose(lib, panel, tensors):
    """(f32 canvas, uint8 canvas of the same launch, uint8 canvas of a uint8-only launch) through a direct call of the export"""
    tab, names = IL.tile_table(panel)
    table = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).cuda()
    ptrs, elems = (C.c_void_p * rt.PANEL_MAX_SRCS)(), (C.c_int64 * rt.PANEL_MAX_SRCS)()
    for i, name in enumerate(names):
        ptrs[i], elems[i] = tensors[name].data_ptr(), tensors[name].numel()
    shape = (panel.n, panel.H, panel.W, 3)
    f32 = torch.full(shape, float("nan"), device="cuda")
    u8, u8_only = torch.full(shape, 77, dtype=torch.uint8, device="cuda"), torch.full(shape, 77, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    args = (table.data_ptr(), len(panel.tiles), ptrs, elems, len(names), panel.n, panel.H, panel.W, C.c_float(panel.background),
            int(panel.post_rescale))
    rt.check(lib.gcpx_panel_compose(*args, f32.data_ptr(), u8.data_ptr(), stream), "panel_compose")
    rt.check(lib.gcpx_panel_compose(*args, None, u8_only.data_ptr(), stream), "panel_compose")
    torch.cuda.synchronize()
    return f32.cpu().numpy(), u8.cpu().numpy(), u8_only.cpu().numpy()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_export_equals_the_reference_canvases_exactly(case, gcpx_lib):
    name, panel, src, want, keep = case
    tensors = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in src.items()}
    f32, u8, u8_only = _device_compose(gcpx_lib, panel, tensors)
    bad = f32[:keep] != want
    print(f"{name}: {int(bad.sum())} of {want.size} f32 elements differ")
    assert f32.dtype == np.float32 and np.array_equal(f32[:keep], want), (name, int(bad.sum()))
    assert np.array_equal(u8[:keep], V.to_uint8(want)) and np.array_equal(u8_only, u8)


def test_wide_and_odd_canvases_cross_segment_and_packing_boundaries(gcpx_lib):
    """a canvas wider than one workgroup's segment (1024 pixels) whose width is not a multiple of 4 (byte stores), tiles that straddle
    the segment boundary and the canvas edge, and an index out of its range (tile skipped)"""
    rng = np.random.RandomState(3)
    res, F, nb = 10, 107, 2
    frames = rng.uniform(-1.3, 1.3, size=(nb, F, 3, res, res)).astype(np.float32)
    idx = np.array([3, 200], np.int32)
    for W in (F * res + 3, F * res):                       # 1073 (odd: byte stores), 1070 (not a multiple of 4 either), then 1072 below
        p = V.Panel("wide", nb, res + 5, W, 1.0)
        p.add(**V._frames("frames", res, F, nb=nb, nf=F, n_b=1, c_f=res, c0=-4, r0=-2, flags=V.RESCALE))
        p.add(**V._frames("frames", res, F, nb=nb, n_b=1, r0=3, index="idx", index_stride=1, index_count=F))
        src = dict(frames=frames, idx=idx)
        want = V.compose(p, src)
        f32, u8, u8_only = _device_compose(gcpx_lib, p, {k: torch.from_numpy(v).cuda() for k, v in src.items()})
        assert np.array_equal(f32, want) and np.array_equal(u8, V.to_uint8(want)) and np.array_equal(u8_only, u8)
    p = V.Panel("wide4", nb, res, 1072, 0.0, post_rescale=True)
    p.add(**V._frames("frames", res, F, nb=nb, nf=F, n_b=1, c_f=res))
    want = V.compose(p, dict(frames=frames))
    f32, u8, u8_only = _device_compose(gcpx_lib, p, dict(frames=torch.from_numpy(frames).cuda()))
    assert np.array_equal(f32, want) and np.array_equal(u8, V.to_uint8(want)) and np.array_equal(u8_only, u8)


def _check_panels(model, panels, expect):
    lib = model.lib
    names = []
    for key, build, tensors, trim in panels:
        panel = build()
        names.append(panel.name)
        want = V.compose(panel, IL.numpy_sources({k: tensors[k] for k in panel.sources}))
        f32, u8, u8_only = _device_compose(lib, panel, tensors)
        assert np.array_equal(f32, want), panel.name
        assert np.array_equal(u8, V.to_uint8(want)) and np.array_equal(u8_only, u8), panel.name
        assert len(np.unique(u8)) > 16, panel.name                   # a picture, not a flat canvas
    assert names == expect, names


def _tree(cfg, batch):
    import video_gcp_amd as VG
    from video_gcp_amd.model import GCPTreeModel
    hp = VG.config(cfg, batch_size=batch)
    sd = VG.init_params(hp, seed=1, randomize_affine=True)
    if hp.adaptive:
        sd["decoder.log_sigma"].fill_(0.2)
        sd["tree_module.tree_modules.0.binding.temp"].fill_(0.05)
    model = GCPTreeModel(hp, params=sd, device="cuda")
    inputs, noise, _ = make_inputs(hp, seed=5, variant="B")
    return hp, model, {k: v.cuda() for k, v in inputs.items()}, noise.cuda()


def test_panels_of_a_balanced_model_equal_the_numpy_restatement():
    hp, model, dev_in, noise = _tree("c1", 5)
    out = model(dev_in, "train", noise=noise)
    _check_panels(model, IL.tree_panels(model, out, dev_in, "train"), ["hierarchical_splits", "pruned_seq_gif"])
    with model.val_mode(pred_length=False):
        out = model(dev_in, "test")
        _check_panels(model, IL.tree_panels(model, out, dev_in, "val"), ["hierarchical_splits", "pruned_seq_gif", "output_tree"])
        assert IL.tree_panels(model, out, dev_in, "val")[0][2]["node_t"] is out.raw["node_t"]      # balanced binding: match_timesteps


def test_panels_of_an_adaptive_attentive_model_equal_the_numpy_restatement():
    hp, model, dev_in, noise = _tree("c5s", 5)
    assert hp.adaptive and hp.attentive_inference
    out = model(dev_in, "train", noise=noise)
    _check_panels(model, IL.tree_panels(model, out, dev_in, "train"),
                  ["hierarchical_splits", "pruned_seq_gif", "match_overview", "gt_target_gif", "attention_masks"])
    # the node tiles sit where node_t says: sample 0, root (depth-first index N // 2), on the device canvas of the first panel
    key, build, tensors, _ = IL.tree_panels(model, out, dev_in, "train")[0]
    panel = build()
    _, u8, _ = _device_compose(model.lib, panel, tensors)
    res, N = hp.img_sz, hp.n_nodes
    assert tensors["node_t"] is out.raw["best_t"]                    # adaptive binding: the argmax of the matching distribution
    t = int(tensors["node_t"][0, N // 2])
    assert 0 <= t < hp.max_seq_len
    root = V.to_uint8((out.raw["images_df"][0, N // 2].cpu().numpy().transpose(1, 2, 0) + np.float32(1)) / np.float32(2))
    r0 = res + V.GAMMA_WIDTH
    assert np.array_equal(u8[0, r0:r0 + res, t * res:(t + 1) * res], root)
    # a prior-sampled prediction has no matching: the nodes sit on the midpoints of tree_module.py:113, the root on end_ind / 2
    with model.val_mode(pred_length=False):
        out = model(dev_in, "test")
        panels = IL.tree_panels(model, out, dev_in, "val")
        _check_panels(model, panels, ["hierarchical_splits", "pruned_seq_gif", "output_tree"])
        steps = panels[0][2]["node_t"].cpu()
        assert steps.dtype == torch.int32 and torch.equal(steps[:, N // 2].long(), out.end_ind.cpu() // 2)
        assert torch.equal(steps[:, N // 4].long(), out.end_ind.cpu() // 4) and int(steps.min()) >= 0 and int(steps.max()) < hp.max_seq_len


def test_panels_of_a_sequential_model_equal_the_numpy_restatement():
    import video_gcp_amd as VG
    from video_gcp_amd.sequential import GCPSequentialModel
    hp = VG.config("c1", batch_size=5, nz_mid_lstm=128, lstm_init="zero")
    model = GCPSequentialModel(hp, params=VG.init_params_sequential(hp, seed=1, randomize_affine=True), device="cuda")
    inputs, noise, _ = make_inputs(hp, seed=3, variant="B")
    dev_in = {k: v.cuda() for k, v in inputs.items()}
    out = model(dev_in, "train", noise=noise[:, :hp.max_seq_len - 1].contiguous().cuda())       # one latent per predicted step
    _check_panels(model, IL.sequential_panels(model, out, dev_in, "train"), ["dense_rec"])
    _check_panels(model, IL.sequential_panels(model, out, dev_in, "val"), ["dense_rec"])


def _run_trainer(tmp_path, monkeypatch, name, extra, conf=None):
    import json
    from video_gcp_amd.model import GCPTreeModel
    from video_gcp_amd.train import ModelTrainer, get_cmd_args
    exp = tmp_path / name
    exp.mkdir()
    (exp / "conf.json").write_text(json.dumps(conf or {"config": "c5s", "overrides": {"batch_size": 5}}))
    argv = ["--path", str(exp), "--num_epochs", "1", "--batches_per_epoch", "3", "--log_outputs_interval", "1", "--imepoch", "3",
            "--deterministic", "1"] + extra
    # every model of a process draws its latent noise from a stream of its own, numbered by this counter (model.py): the runs that are
    # compared start from the same number, as two processes would
    monkeypatch.setattr(GCPTreeModel, "_n_models", 0)
    tr = ModelTrainer(get_cmd_args(argv))
    tr.run()
    return tr, str(exp)


def test_trainer_writes_pictures_only_when_asked_and_logging_does_not_disturb_the_run(tmp_path, monkeypatch):
    tr, exp = _run_trainer(tmp_path, monkeypatch, "with", ["--log_images", "1"])
    panels = ["hierarchical_splits", "pruned_seq_gif", "match_overview", "gt_target_gif", "attention_masks"]
    ext = lambda p: "apng" if p.endswith("gif") else "png"
    want = {f"{p}_train_{s}.{ext(p)}" for p in panels for s in (0, 1, 2)}
    # validation runs before the epoch (step 0) and after it (step 3); its prior-sampled prediction has no matching and no attention
    want |= {f"{p}_val_{s}.{ext(p)}" for p in ("hierarchical_splits", "pruned_seq_gif", "output_tree") for s in (0, 3)}
    assert set(os.listdir(os.path.join(exp, "images"))) == want
    assert sorted(os.path.basename(f) for f in tr.image_files) == sorted(want)
    # the files of the last logging call decode to the canvases it composed
    assert set(tr.model.last_panels) == {"hierarchical_splits", "pruned_seq_gif", "output_tree"}
    for p, canvas in tr.model.last_panels.items():
        frames, delays = FX.decode_png(open(os.path.join(exp, "images", f"{p}_val_3.{ext(p)}"), "rb").read())
        if p.endswith("gif"):
            assert np.array_equal(frames, canvas) and (len(frames) == 1 or delays == [0.25] * len(frames))
        else:
            assert frames.shape[0] == 1 and np.array_equal(frames[0].reshape(canvas.shape), canvas)
        assert len(np.unique(canvas)) > 16
    tr0, exp0 = _run_trainer(tmp_path, monkeypatch, "without", [])
    assert not os.path.exists(os.path.join(exp0, "images")) and tr0.image_files == []
    assert tr.global_step == tr0.global_step == 3 and len(tr.log) == 3
    assert tr.log == tr0.log and tr.last_val == tr0.last_val          # bit-equal losses: logging only reads
    assert torch.equal(tr.model.theta, tr0.model.theta)


def test_trainer_writes_the_dense_rec_video_of_the_sequential_model_and_nothing_with_dont_save(tmp_path, monkeypatch):
    conf = {"config": "c1", "model": "SequentialModel", "lr": 1e-3, "overrides": {"nz_mid_lstm": 128, "lstm_init": "zero", "batch_size": 5}}
    tr, exp = _run_trainer(tmp_path, monkeypatch, "seq", ["--log_images", "1"], conf)
    want = {f"dense_rec_train_{s}.apng" for s in (0, 1, 2)} | {f"dense_rec_val_{s}.apng" for s in (0, 3)}
    assert set(os.listdir(os.path.join(exp, "images"))) == want
    frames, delays = FX.decode_png(open(os.path.join(exp, "images", "dense_rec_train_2.apng"), "rb").read())
    hp = tr.model._hp
    assert frames.shape == (hp.max_seq_len, 2 * hp.img_sz + 2, 5 * hp.img_sz, 3) and delays == [0.25] * hp.max_seq_len
    assert not frames[:, hp.img_sz:hp.img_sz + 2].any()               # the 2-pixel gap of zeros between the rows
    tr1, exp1 = _run_trainer(tmp_path, monkeypatch, "dont", ["--log_images", "1", "--dont_save", "1"], conf)
    assert not os.path.exists(os.path.join(exp1, "images")) and tr1.image_files == []
