"""The control experiments' maze environment on the host (no GPU): the numpy restatements of csrc/nav_env.hip (nav_env.goal_dist_numpy,
step_numpy), the environment settings of a control configuration (conf_loader.environment_from_control_conf) and the control-performance
numbers (control_perf.control_perf) against hand-built cases and against the reference's compute_control_perf.main, executed by
tests/golden/make_ref_control_perf_goldens.py (tests/golden/ref_control_perf.npz)."""
import glob
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import video_gcp_amd  # noqa: E402,F401
from video_gcp_amd import conf_loader as CL  # noqa: E402
from video_gcp_amd import control_perf as CP  # noqa: E402
from video_gcp_amd import nav_env as NE  # noqa: E402
from video_gcp_amd import nav_gen as NG  # noqa: E402
from video_gcp_amd import nav_layout as NL  # noqa: E402
from nav_env_cases import CONF, POST, R, hand_case_rows  # noqa: E402

REFERENCE = "/root/reference"


# ---- the goal distance --------------------------------------------------------------------------------------------------------------------
def _point_pairs(rps, n=200):
    """n seeded pairs in table coordinates: uniform ones (same room, adjacent rooms, far apart as they fall), then on purpose pairs in
    one room, in adjacent rooms, in opposite corners, and points outside [-0.5, 0.5]"""
    rng = np.random.RandomState(10 + rps)
    pairs = [rng.uniform(-0.499, 0.499, size=(2, 2)) for _ in range(n - 40)]
    boxes = NL.RoomBoxes(rps)
    for k in range(10):                                    # one room
        c = boxes.room_center(int(rng.randint(rps * rps)))
        c = np.clip(c, -0.4, 0.4)
        pairs.append(c + rng.uniform(-0.09, 0.09, size=(2, 2)))
    doors = NL.layout(rps).doors
    for k in range(10):                                    # two rooms that share a door
        a, b = doors[int(rng.randint(len(doors)))]
        ca, cb = np.clip(boxes.room_center(a), -0.45, 0.45), np.clip(boxes.room_center(b), -0.45, 0.45)
        pairs.append(np.stack([ca + rng.uniform(-0.04, 0.04, 2), cb + rng.uniform(-0.04, 0.04, 2)]))
    for k in range(10):                                    # opposite corners of [-0.5, 0.5]^2
        s = 1.0 if k % 2 else -1.0
        pairs.append(np.array([[-0.49, s * 0.49], [0.49, -s * 0.49]]) + rng.uniform(-0.009, 0.009, size=(2, 2)))
    for k in range(10):                                    # a coordinate outside [-0.5, 0.5]: of the position, of the goal, of both
        p = rng.uniform(-0.45, 0.45, size=(2, 2))
        v = (0.5 + 0.3 * 10.0 ** -(k % 5)) * (1.0 if k % 2 else -1.0)       # 0.8 down to 0.50003, either sign
        if k % 3 != 1:
            p[0, k % 2] = v
        if k % 3 != 0:
            p[1, (k + 1) % 2] = v
        pairs.append(p)
    return pairs


@pytest.mark.parametrize("rps", [3, 4, 5])
def test_goal_distance_equals_compute_shortest_path(rps):
    pairs = _point_pairs(rps)
    assert len(pairs) == 200
    n_out = n_same = n_far = 0
    for p, g in pairs:
        want, way = NL.compute_shortest_path(rps, p, g)
        got = NE.goal_dist_numpy(rps, p, NE.goal_table(rps, g))
        assert abs(got - want) <= 1e-12, (p, g, got, want)
        n_out += want == 10.0 and len(way) == 0
        n_same += len(way) == 2
        n_far += len(way) >= 5
    assert n_out >= 10 and n_same >= 10 and n_far >= 10, (n_out, n_same, n_far)


def test_goal_table_marks():
    tab = NE.goal_table(3, (0.3, -0.2))
    room = NL.layout(3).coords2ridx(0.3, -0.2)
    assert tab[room].tolist() == [0.3, -0.2, -1.0] and (np.delete(tab[:, 2], room) > 0).all()
    assert np.isnan(NE.goal_table(3, (0.3, 0.6))[:, 2]).all()
    assert NE.goal_dist_numpy(3, (0.0, 0.0), NE.goal_table(3, (0.3, 0.6))) == 10.0
    assert NE.wall_table(3).shape == (30, 4) and NE.wall_table(5).shape == (74, 4)
    w = NE.wall_table(3)
    assert np.abs(w).max() == 0.5 and ((w[:, 0] == w[:, 2]) | (w[:, 1] == w[:, 3])).all()      # centred, axis-parallel


# ---- the step, on hand-built cases in the 9-room maze ---------------------------------------------------------------------------------------
def test_step_numpy_hand_built_cases():
    walls = NE.wall_table(3)
    for name, s, a, blocked in hand_case_rows():
        r = NE.step_numpy(s, a, walls)
        assert r["blocked"] == blocked, (name, r)
        if blocked:
            assert np.array_equal(r["state"], s) and r["step_len"] == 0.0, name          # rejected whole: position and heading stay
        elif name == "a zero action":
            assert np.array_equal(r["state"], s) and r["step_len"] == 0.0 and r["clearance"] == math.inf
        else:
            new = s[:2] + a                                                              # float32
            want = np.array([new[0], new[1], np.float32(math.atan2(float(new[1]) - float(s[1]), float(new[0]) - float(s[0])))], np.float32)
            assert np.array_equal(r["state"], want), (name, r["state"], want)
            assert abs(r["step_len"] - math.hypot(float(a[0]), float(a[1]))) < 1e-5 and r["clearance"] > R
    # the post cases sit where they are meant to: 1e-4 on either side of r (the float32 states move them by ~1e-8)
    near = {name: NE.step_numpy(s, a, walls)["clearance"] for name, s, a, _ in hand_case_rows() if "post" in name}
    assert abs(near["past a door post at just under r"] - (R - 1e-4)) < 1e-6 and abs(near["past a door post at just over r"] - (R + 1e-4)) < 1e-6
    # a crossing has clearance 0 whatever its ends; a NaN or an overflowing action moves nowhere
    assert NE.step_numpy(*hand_case_rows()[2][1:3], walls)["clearance"] == 0.0
    for bad in ((np.nan, 0.0), (np.inf, 1.0), (3e38, 3e38)):
        r = NE.step_numpy(np.array([3e38, 0.0, 0.1], np.float32) if bad[0] == 3e38 else np.zeros(3, np.float32), np.array(bad, np.float32), walls)
        assert r["blocked"] and r["step_len"] == 0.0


def prm_vertex_paths(n_rooms=9, seed=0, n=24):
    """the vertex paths (environment units, float32 [m, 2]) of the first n trajectories of NavGenerator(n_rooms, seed) whose first
    planning attempt succeeds, planned by prm_numpy at the generator's default parameters"""
    gen = NG.NavGenerator(n_rooms, seed=seed, device="cpu")
    L, out, i = gen.layout, [], 0
    while len(out) < n:
        t = gen.draw_task(i, 0)
        i += 1
        px, py = NG.sample_points_numpy(gen.box_table, gen.point_boxes(t, 0), t["key"], 0, gen.seed)
        sg = t["start_goal"]
        r = NG.prm_numpy(px, py, sg[0], sg[1], sg[2], sg[3], L.ox, L.oy, L.robot_size)
        if r["success"]:
            out.append(NE.table2env(np.stack([r["x"][r["path"]], r["y"][r["path"]]], axis=1)))
    return out


CLOUD_MARGIN = 1e-4


def cloud_clearance(p, q, ox, oy):
    """the least distance from the segment [p, q] (table coordinates) to the layout's obstacle CLOUD, by brute force: the segment
    sampled every <= 2e-5, against every cloud point near it.  Independent of nav_env's segment arithmetic.  The cloud's points lie
    <= 0.002 apart along every wall (Layout: int((hi - lo + 1) * 100) points per segment), so this exceeds the distance to the walls
    themselves by at most sqrt(r^2 + 0.001^2) - r = 2.5e-5 at distances around r = 0.02, plus 1e-5 of sampling: < CLOUD_MARGIN."""
    p, q = np.asarray(p, dtype=np.float64), np.asarray(q, dtype=np.float64)
    n = int(math.ceil(float(np.hypot(*(q - p))) / 2e-5)) + 1
    pts = p[None] + np.linspace(0.0, 1.0, n)[:, None] * (q - p)[None]
    lo, hi = np.minimum(p, q) - 0.06, np.maximum(p, q) + 0.06
    near = (ox >= lo[0]) & (ox <= hi[0]) & (oy >= lo[1]) & (oy <= hi[1])
    if not near.any():
        return math.inf
    best = math.inf
    for s in range(0, n, 1024):
        dx, dy = pts[s:s + 1024, 0, None] - ox[near][None], pts[s:s + 1024, 1, None] - oy[near][None]
        best = min(best, float(np.sqrt((dx * dx + dy * dy).min())))
    return best


def test_planned_paths_are_never_blocked():
    """PRM plans (seed 0, 9 rooms, the generator's default parameters) executed vertex to vertex: every edge of the first 20 plans
    that clear the walls by more than r is free, and over ALL plans drawn a move is blocked only where it does come within r.

    Which plans: is_collision (prm.py:96-122) tests an edge at points rr = r apart, so the expert's own edges may pass a door post as
    close as sqrt(rr^2 - (rr / 2)^2) = 0.866 rr, inside the radius at which the environment must block (segment distance <= r).
    "Never blocked" can therefore only be asked of plans whose edges all clear the walls by more than r.  That is decided here without
    the code under test: by cloud_clearance, a brute-force distance to the reference's obstacle cloud, with CLOUD_MARGIN for the
    cloud's spacing.  An edge is `clear` when its cloud clearance is > r + CLOUD_MARGIN (its true clearance is then > r), `close`
    when it is <= r (its true clearance is then <= r too); between the two the cloud cannot tell.  Of the first 24 plans of seed 0,
    one has a close edge (plan 20, edge 61: 0.0179) and is passed over; none has an edge the cloud cannot tell."""
    L, walls = NL.layout(3), NE.wall_table(3)
    n_edges = n_qualified = 0
    passed_over = []
    for j, path in enumerate(prm_vertex_paths()):
        s = np.array([path[0, 0], path[0, 1], 0.0], dtype=np.float32)
        verdicts = []
        for k in range(1, len(path)):
            a = (path[k] - s[:2]).astype(np.float32)
            r = NE.step_numpy(s, a, walls)
            c = cloud_clearance(NE.env2table(s[:2]), NE.env2table((s[:2] + a).astype(np.float32)), L.ox, L.oy)
            clear, close = c > R + CLOUD_MARGIN, c <= R
            assert not (r["blocked"] and clear), (j, k, c, r)              # never blocked where the move clears the walls by > r
            assert not (close and not r["blocked"]), (j, k, c, r)          # and never let through where it comes within r
            if c < 0.05:                                                   # (the cloud is searched up to 0.06 around the edge)
                assert abs(r["clearance"] - c) < CLOUD_MARGIN or (r["clearance"] == 0.0 and c < 0.002), (j, k, c, r)
            else:
                assert r["clearance"] > 0.05 - CLOUD_MARGIN, (j, k, c, r)
            verdicts.append(clear)
            n_edges += 1
            s = r["state"] if not r["blocked"] else np.array([path[k, 0], path[k, 1], 0.0], dtype=np.float32)
        if all(verdicts) and n_qualified < 20:
            n_qualified += 1                                             # (the asserts above: none of its edges was blocked)
        elif not all(verdicts):
            passed_over.append(j)
    print(f"{n_edges} edges, {n_qualified} plans clear of the walls by > r, passed over: {passed_over}")
    assert n_qualified == 20 and n_edges > 200 and len(passed_over) <= 4, (n_qualified, passed_over)


# ---- the environment of a control configuration ---------------------------------------------------------------------------------------------
ENV = dict(GCP_DATA_DIR="/nowhere/data", GCP_EXP_DIR="/nowhere/exp")


def _conf(tmp_path, env_params, env_cls="TopdownMultiroom3dEnv"):
    p = tmp_path / "mod_hyper.py"
    p.write_text(CONF.format(env_params=env_params, env_cls=env_cls, T=24))
    return CL.exec_control_conf(str(p), ENV)


def test_environment_from_a_control_conf(tmp_path):
    c = _conf(tmp_path, "n_rooms=25, crop_window=20, heading_smoothing=0.1, init_pos=None, goal_pos=None")
    before = list(CL.planner_from_control_conf(c).ignored)
    e = CL.environment_from_control_conf(c)
    assert (e.n_rooms, e.crop_window, e.T, e.img_sz) == (25, 20, 24, 32)
    reasons = dict(k.split(":", 1) for k in e.ignored)
    assert set(reasons) == {"agent.env.heading_smoothing", "agent.env.init_pos", "agent.env.goal_pos"}
    assert "unsmoothed" in reasons["agent.env.heading_smoothing"]
    after = CL.planner_from_control_conf(c).ignored
    assert after == before and "agent.env:simulator" in after                        # the planner's description is untouched
    e = CL.environment_from_control_conf(_conf(tmp_path, "n_rooms=9"))
    assert (e.n_rooms, e.crop_window) == (9, CL.DEFAULT_CROP_WINDOW) and e.ignored == []
    with pytest.raises(ValueError, match="made_up_key"):
        CL.environment_from_control_conf(_conf(tmp_path, "n_rooms=9, made_up_key=1"))
    with pytest.raises(ValueError, match="init_pos"):
        CL.environment_from_control_conf(_conf(tmp_path, "n_rooms=9, init_pos=(0.1, 0.2)"))
    with pytest.raises(ValueError, match="goal_pos"):
        CL.environment_from_control_conf(_conf(tmp_path, "n_rooms=9, goal_pos=0"))
    with pytest.raises(ValueError, match="Multiroom3dEnv"):
        CL.environment_from_control_conf(_conf(tmp_path, "n_rooms=9", env_cls="Multiroom3dEnv"))
    broken = dict(c, agent=dict(c["agent"], env=dict(n_rooms=9)))
    with pytest.raises(ValueError, match="agent.env"):
        CL.environment_from_control_conf(broken)
    with pytest.raises(ValueError, match="image_height"):
        CL.environment_from_control_conf(dict(c, agent=dict(c["agent"], image_width=64)))


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="the reference checkout is not on this machine")
def test_environment_from_the_shipped_control_confs():
    files = sorted(glob.glob(os.path.join(REFERENCE, "experiments", "control", "*", "*", "mod_hyper.py")))
    assert len(files) == 4
    for f in files:
        c = CL.exec_control_conf(f, ENV)
        before = list(CL.planner_from_control_conf(c).ignored)
        e = CL.environment_from_control_conf(c)
        assert e.n_rooms == (25 if "25room" in f else 9) and e.crop_window == 40 and e.img_sz == 32, f
        assert e.T == c["agent"]["T"] and e.T in (200, 400), f
        assert any(k.startswith("agent.env.heading_smoothing:") for k in e.ignored)
        assert CL.planner_from_control_conf(c).ignored == before


# ---- the control-performance numbers ----------------------------------------------------------------------------------------------------------
def test_control_perf_hand_built():
    """9 rooms; room (i, j) of the table has the index 3 i + 2 - j.  Task 0 walks 3 + 4 = 7 units and ends in its goal's room; task 1
    ends in the centre room with its goal in the room to the right (an open door: 2 rooms); task 2 ends bottom left with its goal top
    right (5 rooms by the breadth-first search)."""
    traj = np.zeros((3, 3, 3), dtype=np.float32)
    traj[0, :, :2] = [(-9.0, -9.0), (-6.0, -9.0), (-6.0, -13.0)]         # stays in one room: 1 room traversed
    traj[1, :, :2] = [(-9.0, 0.0), (-6.0, 0.0), (0.0, 0.0)]              # left middle -> centre: 2 rooms traversed
    traj[2, :, :2] = [(-9.0, 9.0), (-9.0, 9.0), (-9.0, 9.0)]             # never moves
    goals = np.array([(-7.0, -12.0), (9.0, 0.0), (9.0, -9.0)], dtype=np.float32)
    res = dict(full_traj=traj, reset_state=np.concatenate([traj[:, 0], goals], axis=1))
    L = NL.layout(3)
    rooms = lambda p: L.coords2ridx(p[0] / 27, -p[1] / 27)
    far = len(NL.plan_room_seq(rooms(traj[2, -1]), rooms(goals[2]), L.doors))
    assert rooms(traj[0, -1]) == rooms(goals[0]) and far == 5
    p = CP.control_perf(res, n_rooms=9, max_seq_len=200)
    assert p["success"] == 1 / 3 and abs(p["cost"] - (7.0 + 200 + 200) / 3) < 1e-12 and p["n_tasks"] == 3
    assert p["room2goal_mean"] == (1 + 2 + far) / 3 and abs(p["room2goal_std"] - np.std([1, 2, far])) < 1e-12
    assert p["rtravers_mean"] == (1 + 2 + 1) / 3 and abs(p["rtravers_std"] - np.std([1, 2, 1])) < 1e-12
    first = CP.control_perf(res, n_rooms=9, n_tasks=1, max_seq_len=50)
    assert first["success"] == 1.0 and first["cost"] == 7.0 and first["room2goal_mean"] == 1.0 and first["room2goal_std"] == 0.0
    assert CP.report(first) == ["Success: \t1.0", "Cost: \t7.00", "", "Room2Goal: \t1.0\t0.0", "RTravers: \t1.0\t0.0"]
    with pytest.raises(ValueError, match="n_tasks"):
        CP.control_perf(res, n_rooms=9, n_tasks=4)


@pytest.mark.parametrize("case", ["exact", "walk9", "walk25"])
def test_control_perf_equals_the_reference(case):
    """compute_control_perf.main executed on synthetic trajectories (make_ref_control_perf_goldens.py).  Its `Cost` is printed with two
    decimals: case `exact` has a cost that two decimals hold exactly (103), the random walks' costs are compared as printed."""
    with np.load(os.path.join(ROOT, "tests", "golden", "ref_control_perf.npz")) as z:
        g = {k[len(case) + 1:]: z[k] for k in z.files if k.startswith(case + "/")}
    p = CP.control_perf(dict(full_traj=g["full_traj"], reset_state=g["reset_state"]), int(g["n_rooms"]), None, int(g["max_seq_len"]))
    got = [p["success"], p["cost"], p["room2goal_mean"], p["room2goal_std"], p["rtravers_mean"], p["rtravers_std"]]
    for k, (a, b) in enumerate(zip(got, g["values"])):
        assert abs(a - b) <= (1e-9 if k != 1 or case == "exact" else 0.005 + 1e-9), (k, a, b)
    assert CP.report(p) == [str(s) for s in g["lines"]]
    assert 0 < p["success"] < 1
