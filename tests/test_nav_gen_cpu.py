"""Nav data generator, host side (no GPU): nav_layout and the numpy restatements of nav_gen against tests/golden/ref_prm.npz, which
tests/golden/make_ref_prm_goldens.py recorded by EXECUTING the reference's prm.py, multiroom2d_layout.py, sampling_fcns.py and
prm_policy.py.

Exactness.  The PRM cases keep only seeds whose decisions all lie further than 1e-9 from their thresholds in the reference's own run
(|dist - rr|, |d - max_edge_len|, round's half-way point of d / rr, gaps between sorted neighbour distances, best against second-best
path cost; `case_*/margins`).  Float64 arithmetic in another order moves a distance by a few 1e-17, so every decision -- and with it
every integer of the kept mask, the road map and the path -- must come out equal.

Spline bound.  scipy reaches the interpolating spline by two routes, splprep / splev and make_interp_spline; their difference on each
case's path is recorded (`spline_route_diff`).  The restatement may differ from the first route by 100 x that figure, at least 1e-12
(values of magnitude <= 1; a tridiagonal solve over ~50 vertices loses a few hundred ulps at most)."""
import hashlib
import json
import os

import numpy as np
import pytest

from video_gcp_amd import nav_gen as NG
from video_gcp_amd import nav_layout as NL

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ("a", "b", "c", "d", "e")


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(HERE, "golden", "ref_prm.npz")) as z:
        return {k: z[k] for k in z.files}


def spline_bound(gold, case):
    return max(100.0 * float(gold[f"case_{case}/spline_route_diff"]), 1e-12)


def case_inputs(gold, case):
    g = lambda k: gold[f"case_{case}/{k}"]
    L = NL.layout(int(g("rooms_per_side")))
    sg = g("start_goal")
    return dict(px=g("px"), py=g("py"), sx=sg[0], sy=sg[1], gx=sg[2], gy=sg[3], ox=L.ox, oy=L.oy, rr=L.robot_size, n_knn=int(g("n_knn")),
                max_edge_len=float(g("max_edge_len")), cost_power=float(g("cost_power")))


@pytest.mark.parametrize("n", [3, 4, 5])
def test_layout_equals_the_reference(gold, n):
    L = NL.layout(n)
    g = lambda k: gold[f"layout{n}/{k}"]
    assert L.ox.dtype == np.float64 and L.ox.shape[0] == int(g("n_points")) == {3: 3828, 4: 6210, 5: 9304}[n]
    assert [hashlib.sha256(a.tobytes()).hexdigest() for a in (L.ox, L.oy)] == list(g("sha256"))
    if n == 3:
        assert np.array_equal(L.ox, g("ox")) and np.array_equal(L.oy, g("oy"))
    assert np.array_equal(np.array(L.doors), g("doors"))
    assert L.table_size == float(g("table_size")) and L.robot_size == float(g("robot_size"))
    q = g("ridx_query")
    assert [L.coords2ridx(a, b) for a, b in q] == g("ridx").tolist()
    assert np.array_equal(L.coords2ridx(q[:, 0], q[:, 1]), g("ridx"))
    boxes = NL.RoomBoxes(n)
    pos = np.stack([boxes.get_door_pos(a, b) for a, b in L.doors])
    assert np.abs(pos - g("door_pos")).max() <= 1e-15
    want = [boxes.sampling_width, boxes.door_sampling_width, *boxes.hor_door_sampling_width, *boxes.vert_door_sampling_width]
    assert np.array_equal(np.array(want), g("room_box"))
    tab = boxes.box_table(L.doors)
    assert tab.shape == (n * n + 2 * len(L.doors), 4) and (tab[-len(L.doors):, 2:] == 0).all()
    assert np.array_equal(tab[n * n:n * n + len(L.doors), :2], pos)


@pytest.mark.parametrize("n", [3, 5])
def test_room_sequences_equal_the_reference(gold, n):
    g = lambda k: gold[f"layout{n}/{k}"]
    L = NL.layout(n)
    bfs, boff, multi, moff, cnt = g("bfs"), g("bfs_off"), g("multi"), g("multi_off"), g("multi_count")
    pair = m0 = 0
    for a in range(n * n):
        for b in range(n * n):
            assert NL.plan_room_seq(a, b, L.doors) == bfs[boff[pair]:boff[pair + 1]].tolist()
            want = [multi[moff[m0 + k]:moff[m0 + k + 1]].tolist() for k in range(cnt[pair])]
            assert NL.room_paths(n, a, b) == want
            m0 += int(cnt[pair])
            pair += 1
    assert int(cnt.max()) == {3: 4, 5: 40}[n]


@pytest.mark.parametrize("n", [3, 5])
def test_compute_shortest_path(gold, n):
    pts, want = gold[f"layout{n}/sp_points"], gold[f"layout{n}/sp_length"]
    got = np.array([NL.compute_shortest_path(n, p[0], p[1])[0] for p in pts])
    assert np.abs(got - want).max() <= 1e-15
    if n == 5:
        assert (want == 10.).any() and (want != 10.).any()          # the invalid-coordinate branch is among the 20 pairs
    assert NL.compute_shortest_path(n, [0.6, 0.], [0., 0.]) == (10., [])


@pytest.mark.parametrize("case", CASES)
def test_prm_numpy_equals_the_reference(gold, case):
    g = lambda k: gold[f"case_{case}/{k}"]
    assert float(g("margins").min()) > 1e-9, "the golden seed must keep every decision further than 1e-9 from its threshold"
    r = NG.prm_numpy(**case_inputs(gold, case))
    assert np.array_equal(r["kept"], g("kept"))
    assert np.array_equal(r["road_map"], g("road_map"))
    assert r["success"] == bool(g("success"))
    assert np.array_equal(r["path"], g("path"))
    if r["success"]:
        assert abs(r["cost"] - float(g("cost"))) <= 1e-12 * float(g("cost"))
        assert NG.path_is_free_numpy(r["x"][r["path"]], r["y"][r["path"]], NL.layout(int(g("rooms_per_side"))).ox,
                                     NL.layout(int(g("rooms_per_side"))).oy, 0.02, float(g("max_edge_len")))
    else:
        assert case == "e" and r["path"].shape == (0,) and r["cost"] == np.inf


def test_case_sizes(gold):
    n = {c: int(gold[f"case_{c}/kept"].sum()) + 2 for c in CASES}
    assert n["a"] < 64 and 200 < n["b"] < 300 and n["c"] > 512 and 1200 < n["d"] <= 1324 and n["e"] < 20
    # more than 64 candidates per node in case c: some node has more than 64 others within max_edge_len
    r = NG.prm_numpy(**case_inputs(gold, "a"))
    i = case_inputs(gold, "c")
    keep = gold["case_c/kept"]
    x, y = i["px"][keep], i["py"][keep]
    d = np.sqrt((x[:, None] - x[None, :]) ** 2 + (y[:, None] - y[None, :]) ** 2)
    assert ((d < 0.1).sum(axis=1) - 1).max() > 64
    assert r["x"].shape[0] == n["a"]


def test_obstacle_grid_equals_a_brute_force_scan():
    L = NL.layout(3)
    grid = NG.obstacle_grid(L.ox, L.oy, L.robot_size)
    assert grid["cell"] > L.robot_size and grid["cell_start"][-1] == L.ox.shape[0] and (np.diff(grid["cell_start"]) >= 0).all()
    rs = np.random.RandomState(0)
    q = rs.uniform(-0.56, 0.56, size=(400, 2))               # some outside the walls
    brute = NG.nearest_obstacle_numpy(L.ox, L.oy, q[:, 0], q[:, 1])
    for (x, y), b in zip(q, brute):
        v = NG.nearest_obstacle_grid_numpy(grid, x, y)
        assert v == b if b <= grid["cell"] else v > grid["cell"]
    assert NG.nearest_obstacle_grid_numpy(grid, 5., 5.) == np.inf


@pytest.mark.parametrize("case", ["a", "b", "c", "d"])
@pytest.mark.parametrize("ns", [4, 5, 60, 100])
def test_spline_numpy_against_scipy(gold, case, ns):
    i = case_inputs(gold, case)
    keep, path = gold[f"case_{case}/kept"], gold[f"case_{case}/path"]
    x = np.concatenate([i["px"][keep], [i["sx"], i["gx"]]])
    y = np.concatenate([i["py"][keep], [i["sy"], i["gy"]]])
    got = NG.spline_numpy(x[path], y[path], ns)
    err = np.abs(got - gold[f"case_{case}/spline_{ns}"]).max()
    print(f"case {case} n_steps {ns}: max |spline - splev| = {err:.3e}, bound {spline_bound(gold, case):.3e}")
    assert err <= spline_bound(gold, case)


def test_spline_numpy_raises_like_splprep():
    with pytest.raises(TypeError):
        NG.spline_numpy([0., 1., 2.], [0., 1., 0.], 10)
    with pytest.raises(ValueError):
        NG.spline_numpy([0., 1., 1., 2.], [0., 1., 1., 0.], 10)


def test_counter_based_draws():
    u = NG.uniform01(3, np.arange(5)[:, None], np.arange(1000)[None, :])
    assert u.dtype == np.float64 and (u >= 0).all() and (u < 1).all() and len(np.unique(u)) == u.size
    assert abs(u.mean() - 0.5) < 0.02
    assert np.array_equal(NG.uniform01(3, 2, np.arange(1000)), u[2])                    # a key's draws do not depend on the batch
    assert int(NG.mix64(np.uint64(0))) == 0xE220A8397B1DCDAF                            # splitmix64's first output for seed 0
    boxes = NL.RoomBoxes(3).box_table(NL.layout(3).doors)
    pt_box = np.repeat(np.arange(boxes.shape[0]), 20)
    px, py = NG.sample_points_numpy(boxes, pt_box, key=7, draw0=0, seed=1)
    b = boxes[pt_box]
    assert (np.abs(px - b[:, 0]) <= b[:, 2] / 2).all() and (np.abs(py - b[:, 1]) <= b[:, 3] / 2).all()
    px2, _ = NG.sample_points_numpy(boxes, pt_box[5:], key=7, draw0=5, seed=1)
    assert np.array_equal(px2, px[5:])


def test_assets_contract_and_wall_pixels(tmp_path):
    from video_gcp_amd.dataset import load_topdown_assets
    for n_rooms, S in ((9, 256), (25, 426)):
        NG.write_spec_and_assets(str(tmp_path / str(n_rooms)), n_rooms, 100)
        a = load_topdown_assets(str(tmp_path / str(n_rooms)))
        assert a["S"] == S and a["cw"] == 40 and a["background"].shape == (S + 80, S + 80, 3)
        assert a["agent_stamp"].shape == (11, 11) and a["agent_stamp"].sum() == 81 and a["agent_stamp"][5, 0] and not a["agent_stamp"][1, 1]
        assert a["agent_color"].tolist() == [0, 0, 255] and a["goal_color"].tolist() == [0, 255, 0]
    plain = NG.draw_layout_picture(9, crop_window=40, plain=True)[40:-40, 40:-40]
    assert set(np.unique(plain)) == {0, 255}
    # by hand, 9 rooms at scale 256: the wall at y = 1/3 is the row 256 - int(256 / 3 - 1) = 172, three pixels thick; its first
    # segment runs from x = 0 to int((1/6 - 0.05002...) * 256) = 29, the next starts at int((1/6 + 0.05002...) * 256) = 55: the door
    # between is open.  The door at x = 0.5 (pixels 115 .. 140) of that wall is one of the two the layout closes.
    black = lambda r, c: (plain[r, c] == 0).all()
    assert all(black(r, 10) for r in (171, 172, 173)) and not black(170, 10) and not black(174, 10)
    assert black(172, 29) and black(172, 30) and not black(172, 31) and not black(171, 30)      # the cap pixel past the end
    assert not black(172, 40) and black(172, 55) and not black(172, 53)
    assert black(172, 128) and black(87, 128)                                                  # the two closed doors
    assert not black(128, 85) and not black(128, 170)                                          # the open doors of the middle row
    # the outer walls, clipped at the border: x = 0 -> columns -1 .. 1, x = 1 -> columns 255 .. 257, y = 1 -> rows 0 .. 2; the wall at
    # y = 0 lies on row 256 - int(0 * 256 - 1) = 257, outside the picture
    assert black(128, 255) and black(128, 0) and black(128, 1) and not black(128, 2) and black(1, 128) and not black(255, 128)
    # the vertical wall at x = 1/3: column int(256 / 3) = 85
    assert all(black(10, c) for c in (84, 85, 86)) and not black(10, 83) and not black(10, 87)
    colour = NG.draw_layout_picture(9, crop_window=40)[40:-40, 40:-40]
    assert (colour[40, 40] == NG.PALETTE[0]).all() and (colour[130, 40] == NG.PALETTE[1]).all() and (colour[40, 130] == NG.PALETTE[3]).all()
    assert np.array_equal(colour == 0, plain == 0) or ((plain == 0).all(axis=2) <= (colour == 0).all(axis=2)).all()
    pad = NG.draw_layout_picture(9, crop_window=40)
    assert (pad[:40] == 0).all() and (pad[:, -40:] == 0).all()


def test_episode_relations():
    T = 12
    t = np.linspace(0, 1, 7)
    plan = np.stack([0.3 * t - 0.1, 0.2 * t * t], axis=1)
    goal = (0.25, -0.3)
    st, ac, pm = NG.episode_numpy(plan, goal, T)
    assert st.shape == (T + 1, 5) and ac.shape == (T, 2) and pm.shape == (T + 1,) and st.dtype == ac.dtype == pm.dtype == np.float32
    assert pm.tolist() == [1.] * 8 + [0.] * 5                                           # get_pad_mask(7 actions, 12)
    assert np.allclose(st[:7, 0], 27 * plan[:, 0], rtol=1e-6) and np.allclose(st[:7, 1], -27 * plan[:, 1], rtol=1e-6, atol=1e-7)
    assert np.array_equal(st[7, :2], st[6, :2]) and (st[8:] == 0).all() and (ac[6:] == 0).all()
    assert np.allclose(ac[:6], np.diff(27 * plan * [1, -1], axis=0), rtol=1e-6)         # the state differences, then the zero action
    assert np.allclose(st[:8, 3:], [27 * 0.25, 27 * 0.3])
    assert np.allclose(st[:6, 2], np.arctan2(ac[:6, 1], ac[:6, 0]), atol=1e-5) and st[6, 2] == st[5, 2] == st[7, 2]
    end_ind = int(np.argmax(pm * np.arange(T + 1)))                                     # what dataset.VideoDataset.draw reads
    assert end_ind == 7
    with pytest.raises(ValueError):
        NG.get_pad_mask(13, 12)
    assert NG.n_steps_for(1.234, 100) == 24 and NG.n_steps_for(10., 100) == 100


def test_key_table():
    hp = NG.screen_prm_params(dict(n_samples_per_room=30, use_scripted_path=False, replan_eps=0.1, type="PrmPolicy"))
    assert hp["n_samples_per_room"] == 30 and hp["n_knn"] == 10 and hp["cost_power"] == 2 and hp["max_planning_retries"] == 2
    for k in ("use_scripted_path", "straight_through_door", "smooth_trajectory"):
        with pytest.raises(ValueError, match="not built"):
            NG.screen_prm_params({k: True})
    with pytest.raises(ValueError, match="unknown"):
        NG.screen_prm_params(dict(n_sample_per_room=3))
    groups = [set(NG.KEY_TABLE[g]) for g in ("mapped", "inert", "unbuilt")]
    assert not (groups[0] & groups[1]) and not (groups[0] & groups[2]) and not (groups[1] & groups[2])
    ref = {"n_samples_per_room", "n_samples_per_door", "n_knn", "max_edge_len", "replan_eps", "max_planning_retries", "cost_power",
           "bottleneck_sampling", "use_var_sampling", "subsample_factor", "max_traj_length", "smooth_trajectory", "sample_door_center",
           "use_scripted_path", "straight_through_door", "n_rooms", "use_fallback_plan", "logger"}       # prm_policy.py:44-64
    assert ref <= set().union(*groups)


def test_experiment_conf_fixture(tmp_path):
    """gen_nav --experiment on a conf in the reference's format: the values of experiments/data_gen/nav_16rooms/mod_hyper.py (recorded
    in the JSON fixture) written back as such a file"""
    from video_gcp_amd import gen_nav
    with open(os.path.join(HERE, "golden", "ref_nav_16rooms_mod_hyper.json")) as f:
        conf = json.load(f)["config"]
    s = NG.experiment_settings(conf)
    assert s == dict(n_rooms=16, crop_window=40, T=100, start_index=0, end_index=999, traj_per_file=1, policy=dict(max_traj_length=100))
    path = tmp_path / "mod_hyper.py"
    env = conf["agent"]["env"][1]
    path.write_text("import os.path\nfrom blox import AttrDict\nfrom gcp.planning.infra.agent.general_agent import GeneralAgent\n"
                    "from gcp.planning.infra.envs.miniworld_env.multiroom3d.multiroom3d_env import TopdownMultiroom3dEnv\n"
                    "from gcp.planning.infra.policy.prm_policy.prm_policy import PrmPolicy\n"
                    f"env_params = {env!r}\n"
                    f"agent = AttrDict(type=GeneralAgent, env=(TopdownMultiroom3dEnv, env_params), T={conf['agent']['T']})\n"
                    "policy = AttrDict(type=PrmPolicy, max_traj_length=agent.T)\n"
                    f"config = AttrDict(start_index={conf['start_index']}, end_index={conf['end_index']}, agent=agent, policy=policy,\n"
                    f"                  data_save_dir=os.environ['GCP_DATA_DIR'] + '/nav_16rooms', traj_per_file={conf['traj_per_file']})\n")
    got = gen_nav.read_experiment(str(path))
    assert got == s
    args = gen_nav.parse_args(["--experiment", str(path), "--out", str(tmp_path / "d")])
    assert (args.n_rooms, args.T, args.n_traj, args.traj_per_file, args.crop_window, args.start_index) == (16, 100, 1000, 1, 40, 0)
    assert args.policy == dict(max_traj_length=100)
    args = gen_nav.parse_args(["--n_rooms", "9", "--n_traj", "24", "--out", "x", "--seed", "3"])
    assert (args.n_rooms, args.T, args.n_traj, args.seed, args.plain) == (9, 100, 24, 3, 0)


def test_generator_bookkeeping_on_the_host():
    """the draws that pick rooms and the point tables need no device: start and goal lie in their rooms' boxes, the room path is one
    of the simple paths between them, n_steps follows compute_shortest_path, and a task depends on (seed, index, redraw) alone"""
    gen = NG.NavGenerator(9, T=100, seed=5, device="cpu")
    L, rb = NL.layout(3), NL.RoomBoxes(3)
    seen = set()
    for i in range(40):
        t = gen.draw_task(i, 0)
        assert t == gen.draw_task(i, 0) and t["key"] == i * 256
        sg, path = t["start_goal"], t["room_path"]
        assert L.coords2ridx(sg[0], sg[1]) == path[0] and L.coords2ridx(sg[2], sg[3]) == path[-1]
        for room, (x, y) in ((path[0], sg[:2]), (path[-1], sg[2:])):
            assert (np.abs(np.array([x, y]) - rb.room_center(room)) <= rb.sampling_width / 2).all()
        assert path in NL.room_paths(3, path[0], path[-1])
        assert t["n_steps"] == min(int(NL.compute_shortest_path(3, sg[:2], sg[2:])[0] * 20), 100)
        tab = gen.point_boxes(t, 0)
        assert tab == [r for r in path for _ in range(50)] + [gen._door_box[(min(a, b), max(a, b))] for a, b in zip(path[:-1], path[1:])
                                                             for _ in range(3)]
        seen.add((path[0], path[-1]))
    assert len(seen) > 20 and gen.draw_task(3, 1)["start_goal"] != gen.draw_task(3, 0)["start_goal"]
    assert NG.NavGenerator(9, seed=6, device="cpu").draw_task(3, 0)["start_goal"] != gen.draw_task(3, 0)["start_goal"]
    var = NG.NavGenerator(9, seed=5, device="cpu", use_var_sampling=True, sample_door_center=True, n_samples_per_door=2)
    counts = set()
    for i in range(12):
        t = var.draw_task(i, 0)
        tab, path = var.point_boxes(t, 0), t["room_path"]
        doors = tab[len(tab) - 2 * (len(path) - 1):] if len(path) > 1 else []
        rooms = tab[:len(tab) - len(doors)]
        assert all(b >= 9 + len(L.doors) for b in doors) and all(b < 9 for b in rooms)      # the zero-width boxes of the door centres
        per_room = [rooms.count(r) for r in path]
        counts.update(per_room)
        assert sum(per_room) == len(rooms)
    assert counts == {30, 300}                                                              # PrmPolicy.VAR_SAMPLING_RATES
    assert NG.NavGenerator(9, device="cpu", bottleneck_sampling=False).point_boxes(gen.draw_task(0, 0), 0) == \
        [r for r in gen.draw_task(0, 0)["room_path"] for _ in range(50)]
    with pytest.raises(ValueError, match="max_traj_length"):
        NG.NavGenerator(9, T=100, device="cpu", max_traj_length=80)
    with pytest.raises(ValueError, match="not built"):
        NG.NavGenerator(9, device="cpu", smooth_trajectory=True)
    with pytest.raises(ValueError, match="9, 16 and 25"):
        NG.NavGenerator(36, device="cpu")
