"""The nav datasets' top-down frames on the host (video-gcp_amd/dataset.py): the state -> pixel arithmetic against values worked by hand,
the renderer against a literal restatement of the reference's steps (copy the whole padded picture, paint agent then goal, clamp the
centre, slice) and against a typed-out window, and the numpy assembly over the image-less fixture dataset."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import video_gcp_amd  # noqa: E402,F401
from video_gcp_amd import dataset as DS  # noqa: E402
import topdown_fixture as TF  # noqa: E402


def _assets(arrays):
    """the arrays of an assets file as load_topdown_assets returns them"""
    a = dict(background=arrays["background"], cw=int(arrays["crop_window"]), n_rooms=int(arrays["n_rooms"]),
             scale=int(arrays["render_scale"]), agent_stamp=arrays["agent_stamp"], goal_stamp=arrays["goal_stamp"],
             agent_color=arrays["agent_color"], goal_color=arrays["goal_color"])
    a["S"] = int(DS.topdown_table_size(a["n_rooms"]) * a["scale"])
    return a


@pytest.mark.parametrize("cw", [3, 40])
def test_pixel_positions_of_hand_worked_states(cw):
    px = lambda s, n=9, S=256: DS.topdown_pixels(np.array([s], dtype=np.float32), n, 256, S, cw)[0].tolist()
    assert px((0, 0)) == [128 + cw, 128 + cw]
    assert px((13.5, -13.5)) == [256 + cw, cw]
    assert px((-13.5, 13.5)) == [cw, 256 + cw]
    # 25 rooms: table_size = 5 / 3, S = int(426.67) = 426; x: 13.5 / 27 + 0.8333 = 1.3333 -> int(341.33) = 341;
    # y: 6.75 / 27 + 0.8333 = 1.0833 -> int(277.33) = 277 -> 426 + cw - 277
    assert int(DS.topdown_table_size(25) * 256) == 426
    assert px((13.5, -6.75), 25, 426) == [341 + cw, 149 + cw]
    # q = -13.6 / 27 + 0.5 = -0.0037 -> int(-0.948) = 0, not -1 (x); the same through the mirrored y
    assert px((-13.6, 13.6)) == [cw, 256 + cw]
    assert px((-13.7, 0)) == [cw - 1, 128 + cw]                       # int(-1.896) = -1
    out = DS.topdown_pixels(np.zeros((4, 3), dtype=np.float32), 9, 256, 256, cw)      # a third state column is ignored
    assert out.dtype == np.int32 and out.shape == (4, 2)


def test_fixture_states_round_trip():
    pix = np.array([[-2, 5], [0, 0], [7, 31], [30, 30], [6, 30], [18, 3]])
    st = TF.states_for_pixels(pix, 9, 24, 24, 6)
    assert np.array_equal(DS.topdown_pixels(st, 9, 24, 24, 6), pix)


def _restate(a, x, y, gx, gy):
    """render_pos_top_down (multiroom3d_env.py:185-219) step by step on a copy of the whole padded picture"""
    img = a["background"].copy()
    side, cw, k = img.shape[0], a["cw"], a["agent_stamp"].shape[0]
    for stamp, color, (px, py) in ((a["agent_stamp"], a["agent_color"], (x, y)), (a["goal_stamp"], a["goal_color"], (gx, gy))):
        for dy in range(k):
            for dx in range(k):
                yy, xx = py + dy - k // 2, px + dx - k // 2
                if stamp[dy, dx] and 0 <= yy < side and 0 <= xx < side:
                    img[yy, xx] = color
    cx, cy = max(cw, x), max(cw, y)
    return img[cy - cw:cy + cw, cx - cw:cx + cw]


def _mask(a, stamp, px, py, x, y):
    """where `stamp` centred on (px, py) lands inside the crop around agent pixel (x, y)"""
    side, cw, k = a["background"].shape[0], a["cw"], stamp.shape[0]
    m = np.zeros((side + 2 * k, side + 2 * k), dtype=bool)
    m[py + k - k // 2:py + 2 * k - k // 2, px + k - k // 2:px + 2 * k - k // 2] = stamp
    m = m[k:-k, k:-k]
    cx, cy = max(cw, x), max(cw, y)
    return m[cy - cw:cy + cw, cx - cw:cx + cw]


def test_renderer_equals_the_literal_restatement():
    a = _assets(TF.make_assets(seed=5, scale=24, cw=6, k=7))
    cw, k = a["cw"], 7
    assert a["background"].shape == (36, 36, 3)
    goal = (16, 15)
    xy = np.array([(0, 0), (1, 20), (20, 2), (-1, 10), (3, 3), (cw, cw), (15, 15), (16, 14), (18, 16), (30, 30), (30, 8), (5, 30), (25, 9)])
    got = DS.render_topdown_numpy(a, xy, goal)
    assert got.dtype == np.uint8 and got.shape == (len(xy), 2 * cw, 2 * cw, 3)
    seen = dict(border=0, clamped=0, overlap=0, outside=0)
    for i, (x, y) in enumerate(xy.tolist()):
        want = _restate(a, x, y, *goal)
        assert want.shape == (2 * cw, 2 * cw, 3) and np.array_equal(got[i], want), (x, y)
        am, gm = _mask(a, a["agent_stamp"], x, y, x, y), _mask(a, a["goal_stamp"], goal[0], goal[1], x, y)
        if (x < k // 2 or y < k // 2) and am.any():                  # the padded picture's border cut the agent's stamp
            assert am.sum() < a["agent_stamp"].sum()
            seen["border"] += 1
        if x < cw or y < cw:                                          # clamped centre: the dot is not in the middle of the crop
            assert (max(cw, x), max(cw, y)) != (x, y) and (got[i][am & ~gm] == a["agent_color"]).all()
            seen["clamped"] += 1
        if (am & gm).any():                                           # the goal is painted last
            assert (got[i][am & gm] == a["goal_color"]).all() and (got[i][am & ~gm] == a["agent_color"]).all()
            seen["overlap"] += 1
        if not gm.any():
            seen["outside"] += 1
    assert all(v > 0 for v in seen.values()), seen
    with pytest.raises(ValueError):
        DS.render_topdown_numpy(a, [(31, 10)], goal)                  # max(cw, 31) + cw > 36: the reference's slice comes out short


def test_typed_out_window():
    yy, xx = np.mgrid[0:12, 0:12]
    bg = np.stack([10 * yy + xx, yy, xx], axis=-1).astype(np.uint8)
    a = dict(background=bg, cw=2, n_rooms=9, scale=8, S=8, agent_stamp=np.array([[1, 1, 0], [0, 1, 0], [0, 0, 0]], dtype=bool),
             goal_stamp=np.array([[0, 0, 0], [0, 1, 1], [0, 0, 1]], dtype=bool), agent_color=np.array([0, 0, 255], dtype=np.uint8),
             goal_color=np.array([0, 255, 0], dtype=np.uint8))
    got = DS.render_topdown_numpy(a, [(5, 6)], (5, 5))[0]             # rows 4..7, columns 3..6 of the picture
    A, G = (0, 0, 255), (0, 255, 0)
    want = np.array([[(43, 4, 3), (44, 4, 4), (45, 4, 5), (46, 4, 6)],
                     [(53, 5, 3), A, G, G],                           # agent (5, 4) and (5, 5); the goal's (5, 5) wins, (5, 6) is new
                     [(63, 6, 3), (64, 6, 4), A, G],                  # agent centre (6, 5), goal (6, 6)
                     [(73, 7, 3), (74, 7, 4), (75, 7, 5), (76, 7, 6)]], dtype=np.uint8)
    assert np.array_equal(got, want)
    # the clamp moves the crop, not the dot: agent at (1, 0) -> crop at columns 0..3, rows 0..3, stamp cut by the picture's border
    got = DS.render_topdown_numpy(a, [(1, 0)], (9, 9))[0]
    want = bg[0:4, 0:4].copy()
    want[0, 1] = A                                                    # of the stamp's (y, x) = (-1, 0), (-1, 1), (0, 1) only the last is inside
    assert np.array_equal(got, want)


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("nav"))
    arrays = TF.write_topdown_dataset(root, T=8, n_files=4, traj_per_file=3, seed=2, min_len=5, scale=24, cw=6, k=7,
                                      spec_extra="    states_mean=np.array([0.5, -1.0], dtype=np.float32),\n"
                                                 "    states_std=np.array([6.0, 7.0], dtype=np.float32),\n")
    return root, _assets(arrays)


@pytest.mark.parametrize("rl", [False, True])
def test_numpy_assembly_on_the_fixture(tree, rl):
    root, a = tree
    T, img = 8, 8
    spec = DS.load_spec(root)
    ds = DS.VideoDataset(root, spec, "train", img, randomize_length=rl)
    assert ds.kind == "GlobalSplitVarLenVideoDataset" and ds.topdown is not None and ds.resize and ds.src_size == (12, 12)
    assert len(ds.filenames) == 2 and len(ds) == 6
    files = [f for ph in ("train", "val", "test") for f in DS.VideoDataset(root, spec, ph, img).filenames]
    assert len(files) == 4 and not any(f.endswith(DS.TOPDOWN_ASSETS) for f in files)      # the assets file is no trajectory file
    assert np.array_equal(ds.topdown["background"], a["background"]) and ds.topdown["S"] == 24
    raw = ds.read(0)                                                  # files hold no images at all
    assert "images" not in raw and raw["states"].shape[1] == 2 and "traj0" in raw["name"]
    batch = DS.epoch_schedule(len(ds), 3, 1, seed=1, epoch=0, shuffle=True)[0]
    items = [ds.item(i, DS.item_rng(1, c, p)) for i, p, c in batch]
    out = DS.numpy_batch(ds, batch, 1)
    assert out["traj_seq"].shape == (3, T, 3, img, img) and out["traj_seq"].dtype == np.float32
    assert out["traj_seq_states"].shape == (3, T, 2)
    short = 0
    for j, (raw, p) in enumerate(items):
        e = p["end_ind"]
        assert out["end_ind"][j] == e
        assert (out["traj_seq"][j, e + 1:] == -1.0).all()             # frames past end_ind are uint8 zeros
        short += e + 1 < T
        assert np.array_equal(out["I_g"][j], out["traj_seq"][j, e]) and np.array_equal(out["I_0"][j], out["traj_seq"][j, 0])
        win = raw["states"][p["offset"]:p["offset"] + T]
        shown = np.minimum(np.arange(e + 1) + p["chop"], T - 1)
        pix = DS.topdown_pixels(win, 9, 24, 24, 6)
        # frame end_ind: agent and goal coincide
        fr = DS.render_topdown_numpy(a, pix[shown[-1:]], pix[shown[-1]])
        want = np.transpose(DS.resize_frames_numpy(fr, img), (0, 3, 1, 2)).astype(np.float32) / 255 * 2 - 1
        assert np.array_equal(out["I_g"][j], want[0])
        # every rendered frame, by the restatement
        for t in range(e + 1):
            w = _restate(a, *pix[shown[t]].tolist(), *pix[shown[-1]].tolist())
            w = np.transpose(DS.resize_frames_numpy(w, img), (2, 0, 1)).astype(np.float32) / 255 * 2 - 1
            assert np.array_equal(out["traj_seq"][j, t], w), (j, t)
        # states: x, y only, time-mapped, standardised as the spec says
        s = np.zeros((T, 2), dtype=np.float32)
        s[:e + 1] = win[shown]
        if not rl:                                                    # without randomize_length nothing is zeroed: the padded window
            s[:win.shape[0]] = win
        mean, den = np.array([0.5, -1.0], dtype=np.float32), (1e-6 + np.array([6.0, 7.0])).astype(np.float32)
        assert np.array_equal(out["traj_seq_states"][j], (s - mean) / den)
    assert not rl or short > 0


@pytest.mark.parametrize("rl", [False, True])
def test_packed_coordinates_describe_the_same_frames(tree, rl):
    """what pack_item hands to the device (coordinates of the window, the goal, the time-map integers), taken through the time map
    the kernel applies, gives the frames of assemble_numpy"""
    root, a = tree
    T, img, B = 8, 8, 3
    ds = DS.VideoDataset(root, DS.load_spec(root), "train", img, randomize_length=rl)
    batch = DS.epoch_schedule(len(ds), B, 1, seed=6, epoch=0, shuffle=True)[1]
    items = [ds.item(i, DS.item_rng(6, c, p)) for i, p, c in batch]
    coords = np.full(B * T * 2 + B * 2, 12345, dtype=np.int32)
    aux = np.full(B * T + B * T * 2 + B * (T - 1) * 2, 5.0, dtype=np.float32)
    info = np.zeros((B, DS.N_INFO), dtype=np.int32)
    for j, it in enumerate(items):
        DS.pack_item(it, j, coords, aux, info, B, T, 2, 2, topdown=ds.topdown)
    ref = DS.numpy_batch(ds, batch, 6)
    xy, goal = coords[:B * T * 2].reshape(B, T, 2), coords[B * T * 2:].reshape(B, 2)
    for j in range(B):
        n, chop, zero_from, end_ind = info[j, 0], info[j, 3], info[j, 4], info[j, 5]
        for t in range(T):
            s = min(t + chop, T - 1)
            if t <= end_ind and t < zero_from and s < n:
                fr = DS.resize_frames_numpy(DS.render_topdown_numpy(a, xy[j, s][None], goal[j]), img)[0]
            else:
                fr = np.zeros((img, img, 3), dtype=np.uint8)
            assert np.array_equal(ref["traj_seq"][j, t], np.transpose(fr, (2, 0, 1)).astype(np.float32) / 255 * 2 - 1), (j, t)


def test_a_crop_that_does_not_fit_names_the_trajectory(tmp_path):
    root = str(tmp_path)
    TF.write_topdown_dataset(root, T=8, n_files=2, traj_per_file=2, seed=4, min_len=8, scale=24, cw=6, k=7, split=(1.0, 0.0, 0.0))
    spec = DS.load_spec(root)
    path = DS.VideoDataset(root, spec, "train", 8).filenames[0]
    with np.load(path) as z:
        d = {k: z[k] for k in z.files}
    d["traj1/states"][2, 0] = 30.0                                    # q = 1.61: right of the maze, the crop leaves the padded picture
    TF.write_npz(path, d)
    ds = DS.VideoDataset(root, spec, "train", 8)
    plan = dict(offset=0, chop=0, zero_from=8, end_ind=7, pad_mask=np.ones(8, dtype=np.float32))
    DS.assemble_numpy([(ds.read(0), plan)], 8, img_sz=8, topdown=ds.topdown)
    bad = (ds.read(1), plan)
    with pytest.raises(ValueError, match=r"file_\d\.npz:traj1.*frame 2"):
        DS.assemble_numpy([bad], 8, img_sz=8, topdown=ds.topdown)
    with pytest.raises(ValueError, match=r"file_\d\.npz:traj1"):
        DS.pack_item(bad, 0, np.zeros(8 * 2 + 2, dtype=np.int32), np.zeros(8 + 16 + 14, dtype=np.float32),
                     np.zeros((1, DS.N_INFO), dtype=np.int32), 1, 8, 2, 2, topdown=ds.topdown)
    # a frame past end_ind is not rendered, so a state out there does not matter
    DS.assemble_numpy([(bad[0], dict(plan, end_ind=1, zero_from=2))], 8, img_sz=8, topdown=ds.topdown)


def test_missing_or_malformed_assets_raise(tree, tmp_path):
    root, _ = tree
    import shutil
    data = str(tmp_path / "data")
    shutil.copytree(root, data)
    spec = DS.load_spec(data)
    arrays = dict(np.load(os.path.join(data, DS.TOPDOWN_ASSETS)))
    os.remove(os.path.join(data, DS.TOPDOWN_ASSETS))
    with pytest.raises(ValueError, match="MazeTopRendered.*INTEGRATION.md"):
        DS.VideoDataset(data, spec, "train", 8)
    for name in ("Nav25Rooms", "MazeTopRenderedGlobalSplitVarLenVideoDataset", "gcp.datasets.configs.nav_9rooms.Nav9Rooms"):
        with pytest.raises(ValueError, match="MazeTopRendered"):
            DS.VideoDataset(data, dict(spec, dataset_class=name), "train", 8)
    TF.write_assets(data, dict(arrays, background=arrays["background"][1:]))
    with pytest.raises(ValueError, match="background"):
        DS.VideoDataset(data, spec, "train", 8)
    TF.write_assets(data, dict(arrays, agent_stamp=np.ones((4, 4), dtype=bool)))
    with pytest.raises(ValueError, match="stamps"):
        DS.VideoDataset(data, spec, "train", 8)
    TF.write_assets(data, arrays)
    assert DS.VideoDataset(data, spec, "train", 8).topdown["cw"] == 6
