"""State trajectories on the top-down map, on the device: gcpx_topdown_trajectories, called directly, bit for bit equal to its numpy
mirror (visualization.render_trajectories_numpy, itself pinned in tests/test_topdown_traj_cpu.py) at pictures that are and are not a
multiple of the tile, with strided states, at the nav datasets' real size, with more layers than one launch takes, and on NaN / Inf /
huge states; its argument checks; gcpx_topdown_bottlenecks against numpy.argmax; model.log_outputs end to end on tiny models.
Every comparison is exact: the spec is integer arithmetic after an exactly specified float32 conversion."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import video_gcp_amd as VG  # noqa: E402
from video_gcp_amd import dataset as DS  # noqa: E402
from video_gcp_amd import image_log as IL  # noqa: E402
from video_gcp_amd import runtime as rt  # noqa: E402
from video_gcp_amd import visualization as V  # noqa: E402
from helpers import make_inputs  # noqa: E402
import topdown_fixture as TF  # noqa: E402

pytestmark = pytest.mark.gpu
RED, GREEN = (1.0, 0.0, 0.0), (0.0, 1.0, 0.0)


def _assets(**kw):
    arrays = TF.make_assets(**kw)
    a = dict(background=arrays["background"], cw=int(arrays["crop_window"]), n_rooms=int(arrays["n_rooms"]),
             scale=int(arrays["render_scale"]), agent_stamp=arrays["agent_stamp"], goal_stamp=arrays["goal_stamp"],
             agent_color=arrays["agent_color"], goal_color=arrays["goal_color"])
    a["S"] = int(DS.topdown_table_size(a["n_rooms"]) * a["scale"])
    return a


def _call(a, layers, n, **over):
    """the export on device layers [dict(states, length, color, dim_t)]; `over` replaces arguments.  Returns (status, canvas)"""
    lib = rt.load_library()
    dev = torch.device("cuda")
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    bg, ast, gst = t(a["background"]), t(a["agent_stamp"].astype(np.uint8)), t(a["goal_stamp"].astype(np.uint8))
    rgb = lambda c: int(c[0]) | int(c[1]) << 8 | int(c[2]) << 16
    S = over.get("S", a["S"])
    out = torch.full((n, min(S, 4096), min(S, 4096), 3), 77, dtype=torch.uint8, device=dev)
    tab = (rt.TrajLayer * max(len(layers), 1))()
    for d, L in zip(tab, layers):
        st = L["states"]
        d.states, (d.s_n, d.s_p, d.s_d), d.P = st.data_ptr(), st.stride(), over.get("P", st.shape[1])
        d.len, d.len_i64 = L["length"].data_ptr(), int(L["length"].dtype == torch.int64)
        d.color = (C.c_float * 3)(*L["color"])
        if L.get("dim_t") is not None:
            d.dim_t, d.K = L["dim_t"].data_ptr(), over.get("K", L["dim_t"].shape[1])
    status = lib.gcpx_topdown_trajectories(bg.data_ptr(), S, a["cw"], ast.data_ptr(), gst.data_ptr(), over.get("k", ast.shape[0]),
                                           rgb(a["agent_color"]), rgb(a["goal_color"]), tab, over.get("n_layers", len(layers)), n,
                                           over.get("state_dim", 2), a["n_rooms"], a["scale"], out.data_ptr(),
                                           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return status, out.cpu().numpy()


def _check(a, layers, n):
    """device canvases == mirror of the host copies of the same layers"""
    status, got = _call(a, layers, n)
    assert status == 0, rt.load_library().gcpx_last_error()
    want = V.render_trajectories_numpy(a, IL.numpy_layers(layers))[:n]
    assert got.shape == want.shape and np.array_equal(got, want), np.argwhere((got != want).any(-1))[:8]
    return got


def _walks(rng, a, n, P, step=1.5):
    """states [n, P, 2]: random walks that start inside the maze and may leave the picture"""
    lim = 4.5 * int(np.sqrt(a["n_rooms"]))
    return (rng.uniform(-lim, lim, size=(n, 1, 2)) + np.cumsum(rng.randn(n, P, 2) * step, axis=1)).astype(np.float32)


def _dev(x, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(x)).to(device="cuda", dtype=dtype)


@pytest.mark.parametrize("scale", [48, 50])
def test_two_layers_lengths_and_dim_t(scale):
    """S = 48 (tiles of 32: one whole and one half per axis) and S = 50; lengths 1, 2 and all 12 points; dim_t on the second layer with
    a duplicate, a value beyond the length and 0"""
    a = _assets(seed=scale, n_rooms=9, scale=scale, cw=8, k=11)
    assert a["S"] == scale
    rng = np.random.RandomState(scale)
    n, P = 3, 12
    ln64, ln32 = _dev(np.array([1, 2, 12]), torch.int64), _dev(np.array([12, 1, 2]), torch.int32)
    dim_t = _dev(np.array([[0, 3, 3, 4, 30, 7, 11], [1, 1, 0, 0, 5, 5, 5], [2, 10, 11, 6, 7, 0, 0]]), torch.int32)
    for ln in (ln64, ln32):
        layers = [dict(states=_dev(_walks(rng, a, n, P)), length=ln, color=GREEN),
                  dict(states=_dev(_walks(rng, a, n, P)), length=ln, color=RED, dim_t=dim_t)]
        got = _check(a, layers, n)
        assert len(np.unique(got.reshape(-1, 3), axis=0)) > 50           # the random picture shows through
    # the dimmed reds are there: 127 and 63
    reds = {tuple(c) for c in got.reshape(-1, 3).tolist() if c[1] == 0 and c[2] == 0}
    assert (127, 0, 0) in reds or (63, 0, 0) in reds


def test_strided_states_25_rooms():
    """S = 51 at 25 rooms; the states are slices of larger buffers: a [B, W, 2] window with a row pitch of 6, and every second column"""
    a = _assets(seed=2, n_rooms=25, scale=31, cw=5, k=7)
    assert a["S"] == 51
    rng = np.random.RandomState(9)
    n, P = 3, 12
    big = torch.full((5, 20, 6), 1e9, device="cuda")
    big[1:4, 3:15, 2:4] = _dev(_walks(rng, a, n, P, 3.0))
    wide = torch.full((4, 12, 5), -1e9, device="cuda")
    wide[:3, :, 1:5:2] = _dev(_walks(rng, a, n, P, 3.0))
    s1, s2 = big[1:4, 3:15, 2:4], wide[:3, :, 1:5:2]
    assert s1.stride() == (120, 6, 1) and s2.stride() == (60, 5, 2)
    ln = _dev(np.array([12, 7, 30]), torch.int64)                        # 30 > P: all 12 points, as numpy truncates the slice
    dim_t = _dev(np.array([[5, 6], [6, 6], [29, 0]]), torch.int32)
    _check(a, [dict(states=s1, length=ln, color=GREEN), dict(states=s2, length=ln, color=RED, dim_t=dim_t)], n)


def test_more_layers_than_one_launch_takes():
    """11 layers (a launch takes GCPX_TRAJ_LAYERS_PER_LAUNCH = 8): the later launches continue on the canvas, the paint order holds"""
    a = _assets(seed=4, n_rooms=9, scale=48, cw=8, k=5)
    rng = np.random.RandomState(4)
    n, P = 2, 6
    ln = _dev(np.array([6, 4]), torch.int64)
    cols = [(c, 1.0 - c, 0.25 * (i % 5)) for i, c in enumerate(np.linspace(0, 1, 11))]
    _check(a, [dict(states=_dev(_walks(rng, a, n, P, 4.0)), length=ln, color=tuple(float(v) for v in c)) for c in cols], n)
    status, got = _call(a, [], n)                                       # no layer: the unpadded picture
    assert status == 0 and np.array_equal(got, np.repeat(a["background"][None, 8:56, 8:56], n, axis=0))


def test_real_size():
    """the nav datasets' own size: 25 rooms at scale 256 with crop_window 40 (S = 426, 14 x 14 tiles), 100 points, 3 canvases"""
    a = _assets(seed=6, n_rooms=25, scale=256, cw=40, k=11)
    assert a["S"] == 426
    rng = np.random.RandomState(6)
    n, P = 3, 100
    ln = _dev(np.array([100, 57, 81]), torch.int64)
    dim_t = _dev(rng.randint(0, 100, size=(n, 7)), torch.int32)
    layers = [dict(states=_dev(_walks(rng, a, n, P, 0.6)), length=ln, color=GREEN),
              dict(states=_dev(_walks(rng, a, n, P, 0.6)), length=ln, color=RED, dim_t=dim_t)]
    _check(a, layers, n)


def test_non_finite_and_huge_states():
    """the cases of the CPU test on the device: a NaN (no division for its trajectory, its segments skipped), +-Inf at the first, the last
    and a middle point (no stamp there), 1e30 (clamped), 3e38 (overflows to Inf at this scale), all-NaN, a length of 0 and below"""
    a = _assets(seed=7, n_rooms=9, scale=256, cw=8, k=9)
    rng = np.random.RandomState(7)
    n, P = 10, 5
    st = _walks(rng, a, n, P, 3.0)
    st[0, 2, 0] = np.nan
    st[1, 0, 1] = np.inf
    st[2, 4, 1] = -np.inf
    st[3, 2, 1] = np.inf
    st[4, 2] = (1e30, 1e30)
    st[5, 2] = (-1e30, 1e30)
    st[6, 2] = (3e38, 0)
    st[7] = np.nan
    st[8, 1] = (-np.inf, np.nan)
    ln = np.array([5, 5, 5, 5, 5, 5, 5, 5, 5, 0])
    got = _check(a, [dict(states=_dev(st), length=_dev(ln, torch.int64), color=RED)], n)
    S, cw = a["S"], a["cw"]
    bg = a["background"][cw:cw + S, cw:cw + S]
    assert np.array_equal(got[7], bg) and np.array_equal(got[9], bg)
    ln[9] = -3
    _check(a, [dict(states=_dev(st), length=_dev(ln, torch.int32), color=RED)], n)
    # small states around a NaN stay undivided: render units, as in numpy
    st = rng.uniform(-0.8, 0.8, size=(2, 6, 2)).astype(np.float32)
    st[0, 3, 1] = np.nan
    _check(a, [dict(states=_dev(st), length=_dev(np.array([6, 6]), torch.int64), color=GREEN)], 2)


def test_limits_are_checked_before_any_launch():
    a = _assets(seed=1, n_rooms=9, scale=48, cw=8, k=5)
    lib = rt.load_library()
    st, ln = torch.zeros(2, 4, 2, device="cuda"), _dev(np.array([4, 4]), torch.int64)
    dim_t = torch.zeros(2, 3, dtype=torch.int32, device="cuda")
    layer = dict(states=st, length=ln, color=RED, dim_t=dim_t)
    assert _call(a, [layer], 2)[0] == 0
    for over, word in ((dict(S=2049), b"2048"), (dict(P=1025), b"1024"), (dict(n_layers=65), b"64"), (dict(K=17), b"16"), (dict(k=4), b"odd"),
                       (dict(k=33), b"31"), (dict(state_dim=3), b"state_dim"), (dict(P=0), b"1024")):
        assert _call(a, [layer], 2, **over)[0] < 0, over
        assert word in lib.gcpx_last_error(), (over, lib.gcpx_last_error())


# ---- the argmax helper ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,T,K", [(4, 9, 7), (3, 70, 7), (2, 5, 3)])
def test_bottleneck_frames_equal_numpy_argmax(L, T, K):
    from video_gcp_amd.model import TreeView
    lib = rt.load_library()
    rng = np.random.RandomState(L)
    B, N, n = 4, 2 ** L - 1, 3
    w = rng.rand(B, N, T).astype(np.float32)
    w[0, :, :] = np.round(w[0] * 3) / 3                                 # ties: the first maximum
    w[1, 0] = 0                                                         # an all-zero row: 0
    w[1, N // 2] = 0
    w[2, N // 2, T // 2] = np.nan                                       # a NaN counts as the maximum
    w[2, 0, -1] = w[2, 0].max()                                         # the maximum again at the end
    bf2df = TreeView.bf2df_index(L, torch.device("cuda")).cpu().numpy()
    want = np.argmax(w[:, bf2df], axis=2)[:n, :K]
    out = torch.full((n, K), -5, dtype=torch.int32, device="cuda")
    rt.check(lib.gcpx_topdown_bottlenecks(_dev(w).data_ptr(), B, N, T, L, n, K, out.data_ptr(), torch.cuda.current_stream().cuda_stream))
    assert np.array_equal(out.cpu().numpy(), want)
    assert lib.gcpx_topdown_bottlenecks(_dev(w).data_ptr(), B, N + 1, T, L, n, K, out.data_ptr(), None) < 0
    assert lib.gcpx_topdown_bottlenecks(_dev(w).data_ptr(), B, N, T, L, n, N + 1, out.data_ptr(), None) < 0


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
def _model(cfg, **over):
    from video_gcp_amd.model import GCPTreeModel
    hp = VG.config(cfg, batch_size=3, **over)
    sd = VG.init_params(hp, seed=1, randomize_affine=True)
    if hp.adaptive:
        sd["decoder.log_sigma"].fill_(0.2)
        sd["tree_module.tree_modules.0.binding.temp"].fill_(0.05)
    model = GCPTreeModel(hp, params=sd, device="cuda")
    inputs, noise, _ = make_inputs(hp, seed=5, variant="B")
    return hp, model, {k: v.cuda() for k, v in inputs.items()}, noise.cuda()


def test_log_outputs_of_an_adaptive_nav_model(tmp_path):
    """regressed_state_topdown: ground truth green, regressed states red, dimmed around the argmax of the matching of the breadth-first
    nodes 0..6; no full-sequence actions on a training step, so no action_traj_topdown (the reference would re-run the inverse model)"""
    from video_gcp_amd.model import TreeView
    hp, model, dev_in, noise = _model("c5s")
    a = _assets(seed=3, n_rooms=9, scale=48, cw=8, k=7)
    model.log_dir, model.topdown_assets = str(tmp_path), a
    out = model(dev_in, "train", noise=noise)
    files = model.log_outputs(out, dev_in, None, 7, True, "train")
    path = os.path.join(str(tmp_path), "regressed_state_topdown_train_7.png")
    assert path in files and os.path.getsize(path) > 100
    assert not any("action_traj_topdown" in f for f in files) and "action_traj_topdown" not in model.last_panels
    md = out.raw["match_dist_df"].cpu().numpy()
    bf2df = TreeView.bf2df_index(hp.hierarchy_levels, model.device).cpu().numpy()
    length = dev_in["end_ind"].cpu().numpy() + 1
    layers = [dict(states=dev_in["traj_seq_states"].cpu().numpy(), length=length, color=GREEN, dim_t=None),
              dict(states=out.raw["regressed_state_padded"].cpu().numpy(), length=length, color=RED,
                   dim_t=np.argmax(md[:, bf2df], axis=2)[:, :7])]
    want = V.render_trajectories_numpy(a, layers)[:V.N_LOGGED_SAMPLES]
    got = model.last_panels["regressed_state_topdown"]
    assert got.shape == (3, 48, 48, 3) and np.array_equal(got, want)
    assert (got != a["background"][None, 8:56, 8:56]).any()
    # a second logging step reuses the cached canvas and the renderer
    cache = dict(model._image_log_panels)
    model.log_outputs(out, dev_in, None, 8, True, "train")
    assert all(model._image_log_panels[k] is v for k, v in cache.items()) and len(model._image_log_panels) == len(cache)
    assert np.array_equal(model.last_panels["regressed_state_topdown"], want)
    # log_images false: nothing new
    before = sorted(os.listdir(str(tmp_path)))
    assert model.log_outputs(out, dev_in, None, 9, False, "train") == [] and sorted(os.listdir(str(tmp_path))) == before


def test_log_outputs_with_full_sequence_actions_and_without_assets(tmp_path):
    """a forward that produced outputs.actions [B, len, 2] also gives action_traj_topdown; a model without assets writes neither"""
    hp, model, dev_in, noise = _model("c1")
    a = _assets(seed=5, n_rooms=9, scale=50, cw=6, k=5)
    model.log_dir = str(tmp_path)
    with model.val_mode(pred_length=False):                              # val_mode runs the inverse model over the full sequence
        plan_in = {k: dev_in[k] for k in ("I_0", "I_g", "end_ind", "start_ind")}
        out = model(plan_in, "train", noise=noise)
        assert out.raw["actions_padded"].shape == (3, hp.max_seq_len - 1, 2)
        files = model.log_outputs(out, dev_in, None, 1, True, "val")
        assert files and not any("topdown" in f for f in files) and not any("topdown" in k for k in model.last_panels)
        model.topdown_assets = a
        files = model.log_outputs(out, dev_in, None, 2, True, "val")
    for name in ("regressed_state_topdown", "action_traj_topdown"):
        assert os.path.join(str(tmp_path), f"{name}_val_2.png") in files
    # the expected layers by hand: ground truth green first, the prediction red on top, both cut at end_ind + 1, no dim_t (a balanced
    # tree has no matching distribution); the cumulated actions start at the first regressed state
    rs, act = out.raw["regressed_state_padded"], out.raw["actions_padded"]
    length = dev_in["end_ind"].cpu().numpy() + 1
    truth = dict(states=dev_in["traj_seq_states"].cpu().numpy(), length=length, color=GREEN, dim_t=None)
    cum = torch.cat((rs[:, :1], act), dim=1).cumsum(1)                  # (the device's own cumsum: its summation order is torch's)
    assert cum.shape == (3, hp.max_seq_len, 2) and torch.equal(cum[:, 0], rs[:, 0])
    for name, pred in (("regressed_state_topdown", rs), ("action_traj_topdown", cum)):
        want = V.render_trajectories_numpy(a, [truth, dict(states=pred.cpu().numpy(), length=length, color=RED, dim_t=None)])[:3]
        assert model.last_panels[name].shape == (3, 50, 50, 3) and np.array_equal(model.last_panels[name], want), name
    assert list(model.last_panels)[:2] == ["regressed_state_topdown", "action_traj_topdown"]
    assert not np.array_equal(model.last_panels["action_traj_topdown"], model.last_panels["regressed_state_topdown"])
    # a batch smaller than N_LOGGED_SAMPLES: the samples there are
    small = IL.trajectory_layers(model, out, dev_in, torch.cuda.current_stream().cuda_stream, n=7)
    assert list(small) == ["regressed_state_topdown", "action_traj_topdown"]


# ---- --metric and the planner's picture ---------------------------------------------------------------------------------------------------
def _read_png(path):
    """uint8 [H, W, 3] of a PNG written by image_log.write_png (8-bit RGB, filter type 0 on every row)"""
    import struct
    import zlib
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, size = 8, b"", None
    while pos < len(data):
        n, tag = struct.unpack(">I", data[pos:pos + 4])[0], data[pos + 4:pos + 8]
        if tag == b"IHDR":
            size = struct.unpack(">II", data[pos + 8:pos + 16])
        if tag == b"IDAT":
            idat += data[pos + 8:pos + 8 + n]
        pos += 12 + n
    W, H = size
    rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(H, 1 + 3 * W)
    assert (rows[:, 0] == 0).all()
    return rows[:, 1:].reshape(H, W, 3)


def test_metric_pass_and_planner_write_the_trajectory_pictures(tmp_path):
    """`--metric 1` on a nav dataset: metrics/trajectories/it_<step>/trajectories_<b>.png, one red polyline of traj_seq_states[b, :end_ind + 1]
    of the first batch (states with a third column, so the layer is a strided view); write_trajectory_png: the planner's inferStateTraj"""
    from video_gcp_amd.train import ModelTrainer, get_cmd_args
    data, exp = tmp_path / "data", tmp_path / "exp"
    TF.write_topdown_dataset(str(data), T=20, n_files=4, traj_per_file=3, seed=7, min_len=6, scale=64, cw=20, k=7)
    exp.mkdir()
    (exp / "conf.json").write_text('{"config": "c1"}')
    tr = ModelTrainer(get_cmd_args(["--path", str(exp), "--data_dir", str(data), "--metric", "1", "--top_of", "2"]))
    a = tr.model.topdown_assets                                          # handed over by the trainer: the dataset class is top-rendered
    assert a is not None and a["S"] == 64 and np.array_equal(a["background"], tr.val_loader.ds.topdown["background"])
    tr.run()
    torch.cuda.synchronize()
    first = next(iter(tr.val_loader.numpy_batches()))
    B = first["traj_seq_states"].shape[0]
    want = V.render_trajectories_numpy(a, [dict(states=first["traj_seq_states"][..., :2], length=first["end_ind"] + 1, color=RED, dim_t=None)])
    folder = os.path.join(str(exp), "metrics", "trajectories", "it_0")
    assert sorted(os.listdir(folder)) == [f"trajectories_{b}.png" for b in range(min(B, V.N_PLOTTED_ELEMENTS))]
    for b in range(min(B, V.N_PLOTTED_ELEMENTS)):
        assert np.array_equal(_read_png(os.path.join(folder, f"trajectories_{b}.png")), want[b]), b
    assert not os.path.exists(os.path.join(str(exp), "images"))          # no --log_images: no picture log
    # the planner's picture: one red polyline of the plan's regressed states
    states = first["traj_seq_states"][0, :int(first["end_ind"][0]) + 1, :2]
    path = IL.write_trajectory_png(str(tmp_path / "plan_0_inferStateTraj.png"), a, states, torch.device("cuda"))
    assert np.array_equal(_read_png(path), want[0])


def test_plan_entry_point_writes_the_state_trajectory_only_with_the_flag(tmp_path):
    """plan.py --topdown_assets FILE: plan_<i>_inferStateTraj.png next to plan_<i>.npz, one red polyline of the plan's regressed states
    (kept in the .npz as `states`); without the flag the same run writes plan_<i>.npz alone, with the keys it always had"""
    from video_gcp_amd.plan import main
    arrays = TF.make_assets(seed=9, n_rooms=9, scale=48, cw=8, k=7)
    TF.write_assets(str(tmp_path), arrays)
    a = DS.load_topdown_assets(os.path.join(str(tmp_path), "topdown_assets.npz"))        # the file's own path
    assert a["S"] == 48 and np.array_equal(a["background"], arrays["background"])
    argv = ["--config", "c1", "--nstart_goal_pairs", "1", "--candidates", "16", "--iters", "1"]
    plain, drawn = str(tmp_path / "plain"), str(tmp_path / "drawn")
    main(argv + ["--out", plain])
    assert os.listdir(plain) == ["plan_0.npz"]
    assert sorted(np.load(os.path.join(plain, "plan_0.npz")).files) == ["actions", "cost", "image_plan", "latents"]
    res = main(argv + ["--out", drawn, "--topdown_assets", os.path.join(str(tmp_path), "topdown_assets.npz")])
    assert sorted(os.listdir(drawn)) == ["plan_0.npz", "plan_0_inferStateTraj.png"]
    z = np.load(os.path.join(drawn, "plan_0.npz"))
    states = z["states"]
    assert states.shape == (res[0]["plan_len"], 2) and np.isfinite(states).all()
    assert sorted(z.files) == ["actions", "cost", "image_plan", "latents", "states"] and z["image_plan"].shape[0] == states.shape[0]
    want = V.render_trajectories_numpy(a, [dict(states=states[None], length=np.array([states.shape[0]]), color=RED, dim_t=None)])[0]
    assert np.array_equal(_read_png(os.path.join(drawn, "plan_0_inferStateTraj.png")), want)
