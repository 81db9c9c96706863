"""The control experiments on the device: the environment kernels (csrc/nav_env.hip) called directly against their numpy restatement
(nav_env.step_numpy / goal_dist_numpy), the observation against the dataset path's renderer, the batched runner against its own record
and against ImageCEMPolicy driven one episode at a time, and the entry point end to end.

Shapes: 9 rooms (and 25 at E = 5, where the wall count differs), crop_window 40, img_sz 32, T = 6, E in {1, 5, 70} (70 crosses a
wavefront).  Bounds: states, `full_traj` and pixels are float32 / integer results of the same operations in the same order -- equal bit
for bit; `blocked` equal; `path_len` and `goal_dist` are float64 sums of a few terms, compared at 1e-9 absolute -- far above float64
round-off (~1e-14 at these magnitudes), far below a float32 slip (~1e-6).  A decision could differ only where a clearance lies within
1e-9 of the robot radius: the seeds below have no such step (checked here, on the host).
The runner's model is the smallest of tests/test_gpu_control_conf.py: 32 x 32, max_seq_len 12, 32-wide latents, random weights."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from video_gcp_amd import control as CT  # noqa: E402
from video_gcp_amd import control_perf as CP  # noqa: E402
from video_gcp_amd import dataset as DS  # noqa: E402
from video_gcp_amd import nav_env as NE  # noqa: E402
from video_gcp_amd import nav_layout as NL  # noqa: E402
from video_gcp_amd import planning as P  # noqa: E402
from video_gcp_amd import runtime as rt  # noqa: E402
from video_gcp_amd.hparams import GCPHParams  # noqa: E402
from nav_env_cases import CONF, R, hand_case_rows  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T, CW, IMG, SCALE = 6, 40, 32, 256
HP = GCPHParams(batch_size=1, max_seq_len=12, img_sz=32, hierarchy_levels=4, nz_mid_lstm=64, n_lstm_layers=2, nz_mid=32, nz_enc=32,
                nz_vae=32, state_dim=2, ngf=16, n_actions=2)
# the rows that carry the hand-built cases, per E: {row: case}; the case's action is step (case % T), zero actions before it
HAND_ROWS = {1: {0: 5}, 5: {0: 2, 1: 3, 2: 5, 3: 6, 4: 8}, 70: {3: 0, 10: 1, 17: 2, 24: 3, 31: 4, 38: 5, 45: 6, 52: 7, 66: 8}}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module")
def lib():
    return rt.load_library()


# ---- the step kernel ----------------------------------------------------------------------------------------------------------------------
def episodes(n_rooms, E, seed):
    """start [E, 3], goal [E, 2], actions [E, T, 2] (float32, environment units): drawn tasks walked by seeded random steps of length up
    to 2; in the 9-room maze the rows of HAND_ROWS start at a hand-built case's state, stand still until its step and take its action"""
    tasks = NE.draw_tasks(n_rooms, seed, range(E))
    start, goal = tasks["start"].copy(), tasks["goal"].copy()
    rng = np.random.RandomState(seed)
    ang, ln = rng.uniform(-np.pi, np.pi, size=(E, T)), rng.uniform(0.0, 2.0, size=(E, T))
    actions = np.stack([ln * np.cos(ang), ln * np.sin(ang)], axis=-1).astype(np.float32)
    hand = {}
    if n_rooms == 9:
        cases = hand_case_rows()
        for row, k in HAND_ROWS[E].items():
            name, s, a, blocked = cases[k]
            start[row] = s
            actions[row, :k % T] = 0.0
            actions[row, k % T] = a
            hand[row] = (k % T, blocked, name)
    return start, goal, actions, hand


def run_kernels(lib, n_rooms, start, goal, actions):
    rps = NL.rooms_per_side_of(n_rooms)
    E = start.shape[0]
    walls = dev(NE.wall_table(rps))
    tabs = dev(np.stack([NE.goal_table(rps, NE.env2table(g)) for g in goal]))
    S, half = int(DS.topdown_table_size(n_rooms) * SCALE), float(np.float32(0.5 * DS.topdown_table_size(n_rooms)))
    table = NL.ROOM_SIZE * rps
    state, acts = dev(start), dev(actions)
    o = dict(full_traj=torch.full((E, T + 1, 3), -7.0, device=DEV), path_len=torch.full((E,), -7.0, dtype=torch.float64, device=DEV),
             goal_dist=torch.full((E, T + 1), -7.0, dtype=torch.float64, device=DEV),
             blocked=torch.full((E, T), 9, dtype=torch.uint8, device=DEV), pix=torch.full((E, 2), -7, dtype=torch.int32, device=DEV))
    s = rt.current_stream()
    rt.check(lib.gcpx_nav_env_reset(state.data_ptr(), tabs.data_ptr(), rps, table, E, T, half, float(SCALE), S, CW, o["full_traj"].data_ptr(),
                                    o["path_len"].data_ptr(), o["goal_dist"].data_ptr(), o["pix"].data_ptr(), s), "nav_env_reset")
    pixels, keep = [o["pix"].clone()], []
    for t in range(T):
        a = acts[:, t].contiguous()
        keep.append(a)
        rt.check(lib.gcpx_nav_env_step(state.data_ptr(), a.data_ptr(), walls.data_ptr(), walls.shape[0], R, tabs.data_ptr(), rps, table, E, T,
                                       t, half, float(SCALE), S, CW, o["full_traj"].data_ptr(), o["path_len"].data_ptr(),
                                       o["goal_dist"].data_ptr(), o["blocked"].data_ptr(), o["pix"].data_ptr(), s), "nav_env_step")
        pixels.append(o["pix"].clone())
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in o.items()}
    out.update(state=state.cpu().numpy(), pixels=torch.stack(pixels, dim=1).cpu().numpy(), S=S)
    return out


@pytest.mark.parametrize("n_rooms,E", [(9, 1), (9, 5), (9, 70), (25, 5)])
def test_step_kernel_equals_step_numpy(lib, n_rooms, E):
    start, goal, actions, hand = episodes(n_rooms, E, seed=11 + E)
    ref = [NE.rollout_numpy(n_rooms, start[e], goal[e], actions[e]) for e in range(E)]
    clear = np.stack([r["clearance"] for r in ref])
    excluded = np.isfinite(clear) & (np.abs(clear - R) <= 1e-9)
    assert excluded.sum() == 0 and excluded.mean() <= 0.01           # no step of these seeds is decided within 1e-9 of the radius
    for row, (t, blocked, name) in hand.items():                     # the hand-built cases are where they were put
        assert ref[row]["blocked"][t] == blocked and not ref[row]["blocked"][:t].any(), (row, name)
    got = run_kernels(lib, n_rooms, start, goal, actions)
    want = {k: np.stack([r[k] for r in ref]) for k in ("full_traj", "blocked", "path_len", "goal_dist")}
    assert np.array_equal(got["full_traj"].view(np.uint32), want["full_traj"].view(np.uint32))
    assert np.array_equal(got["state"].view(np.uint32), want["full_traj"][:, -1].view(np.uint32))
    assert np.array_equal(got["blocked"], want["blocked"].astype(np.uint8))
    assert np.abs(got["path_len"] - want["path_len"]).max() <= 1e-9 and np.abs(got["goal_dist"] - want["goal_dist"]).max() <= 1e-9
    pix = DS.topdown_pixels(want["full_traj"][..., :2].reshape(-1, 2), n_rooms, SCALE, got["S"], CW).reshape(E, T + 1, 2)
    assert np.array_equal(got["pixels"], pix)
    # the walk meets walls and open space alike, and the distances are those of the maze
    # (the 25-room table reaches past [-0.5, 0.5], where the reference's distance is the constant 10)
    if E >= 5:
        assert 0 < want["blocked"].mean() < 1 and (want["path_len"] > 0).any() and (want["goal_dist"] < 10.0).any()
        assert (want["goal_dist"] == 10.0).any() == (n_rooms == 25)


def test_step_kernel_refuses_bad_arguments(lib):
    start, goal, actions, _ = episodes(9, 5, seed=1)
    E = 5
    walls, tabs, state, a = dev(NE.wall_table(3)), dev(np.stack([NE.goal_table(3, NE.env2table(g)) for g in goal])), dev(start), dev(actions[:, 0])
    full, plen = torch.full((E, T + 1, 3), -7.0, device=DEV), torch.full((E,), -7.0, dtype=torch.float64, device=DEV)
    gd, blocked = torch.full((E, T + 1), -7.0, dtype=torch.float64, device=DEV), torch.full((E, T), 9, dtype=torch.uint8, device=DEV)
    pix = torch.full((E, 2), -7, dtype=torch.int32, device=DEV)
    ptrs = dict(state=state.data_ptr(), action=a.data_ptr(), walls=walls.data_ptr(), tabs=tabs.data_ptr(), full=full.data_ptr(),
                plen=plen.data_ptr(), gd=gd.data_ptr(), blocked=blocked.data_ptr(), pix=pix.data_ptr())

    def step(E_=E, t=0, n_walls=30, radius=R, rps=3, **over):
        p = dict(ptrs, **over)
        return lib.gcpx_nav_env_step(p["state"], p["action"], p["walls"], n_walls, radius, p["tabs"], rps, 1.0, E_, T, t, 0.5, 256.0, 256, CW,
                                     p["full"], p["plen"], p["gd"], p["blocked"], p["pix"], rt.current_stream())

    def reset(E_=E, rps=3, **over):
        p = dict(ptrs, **over)
        return lib.gcpx_nav_env_reset(p["state"], p["tabs"], rps, 1.0, E_, T, 0.5, 256.0, 256, CW, p["full"], p["plen"], p["gd"], p["pix"],
                                      rt.current_stream())

    for name in ptrs:
        assert step(**{name: None}) == -1 and b"gcpx_nav_env_step" in lib.gcpx_last_error() and b"null" in lib.gcpx_last_error(), name
    for kw in (dict(E_=0), dict(t=T), dict(t=-1), dict(n_walls=0), dict(n_walls=1025), dict(radius=-1.0), dict(radius=float("nan")),
               dict(rps=0), dict(rps=17)):
        assert step(**kw) == -1 and b"gcpx_nav_env_step" in lib.gcpx_last_error(), kw
    for name in ("state", "tabs", "full", "plen", "gd", "pix"):
        assert reset(**{name: None}) == -1 and b"gcpx_nav_env_reset" in lib.gcpx_last_error(), name
    assert reset(E_=0) == -1 and reset(rps=0) == -1
    torch.cuda.synchronize()
    # nothing was launched: every output keeps its fill
    assert (full == -7).all() and (plen == -7).all() and (gd == -7).all() and (blocked == 9).all() and (pix == -7).all()
    assert torch.equal(state.cpu(), torch.from_numpy(start))


# ---- the observation ------------------------------------------------------------------------------------------------------------------------
def _frames_numpy(env, states, goal_pix):
    """the dataset path's frames of `states` [E, >= 2]: render_topdown_numpy + resize_frames_numpy, uint8 [E, IMG, IMG, 3]"""
    pix = DS.topdown_pixels(states, env.n_rooms, env.scale, env.S, env.cw)
    return np.stack([DS.resize_frames_numpy(DS.render_topdown_numpy(env.assets, pix[e:e + 1], goal_pix[e]), IMG)[0]
                     for e in range(states.shape[0])])


def test_observation_equals_the_dataset_renderer():
    E = 5
    tasks = NE.draw_tasks(9, 4, range(E))
    tasks["start"][0] = (-12.7, -12.7, 0.3)                          # near the table's corner: the window reaches into the padding
    tasks["goal"][1] = tasks["start"][1, :2] + np.float32(0.15)     # the goal's dot over the agent's
    rng = np.random.RandomState(4)
    actions = rng.uniform(-0.6, 0.6, size=(E, 3, 2)).astype(np.float32)
    env = NE.NavEnvBatch(9, CW, T, IMG, DEV)
    goal_pix = DS.topdown_pixels(tasks["goal"], 9, env.scale, env.S, env.cw)
    obs = env.reset(tasks)
    assert np.array_equal(env.goal_frames.cpu().numpy(), _frames_numpy(env, tasks["goal"], goal_pix))
    for t in range(4):
        if t:
            env.step(dev(actions[:, t - 1]))
            obs = env.observe()
        states = env.full_traj[:, t].cpu().numpy()
        want = _frames_numpy(env, states, goal_pix)
        assert np.array_equal(env.frames[:, t].cpu().numpy(), want), t
        assert obs.shape == (E, 3, IMG, IMG) and torch.equal(obs.cpu(), P.env2planner(want)), t
        if t == 0:
            assert np.array_equal(states, tasks["start"])
            corner = DS.render_topdown_numpy(env.assets, DS.topdown_pixels(states[:1], 9, env.scale, env.S, env.cw), goal_pix[0])[0]
            assert (corner[:5, :5] == 0).all() and (corner == np.array(env.assets["agent_color"])).all(axis=-1).any()
    assert (env.frames[:, 4:] == 0).all()                            # steps not taken yet
    ev = env.eval()
    assert ev["full_traj"].shape == (E, T + 1, 3) and ev["all_goal_distances"].shape == (E, T + 1) and ev["blocked"].shape == (E, T)
    assert np.array_equal(ev["improvement"], ev["initial_dist"] - ev["final_dist"]) and np.array_equal(ev["goal"], tasks["goal"])
    assert np.array_equal(ev["final_dist"], ev["all_goal_distances"][:, 3])


# ---- the runner -----------------------------------------------------------------------------------------------------------------------------
class ShortPlans:
    """a planner whose plans are cut to n frames: a plan shorter than T, so that the episode has to plan again"""

    def __init__(self, planner, n):
        self.planner, self.n = planner, n

    def __call__(self, state, goal):
        img, act, lat, cost = self.planner(state, goal)
        return img[:self.n], act[:self.n - 1], lat[:self.n], cost


class Replay:
    """hands an ImageCEMPolicy the plans an episode of the runner made, in order, and checks the frame each was made from"""

    def __init__(self, plans, frames):
        self.plans, self.frames, self.calls = plans, frames, 0

    def __call__(self, state, goal):
        p = self.plans[self.calls]
        assert np.array_equal(np.asarray(state)[0], self.frames[p["t"]])
        self.calls += 1
        return p["image_plan"], p["action_plan"], p["latent_plan"], p["cost"]


@pytest.fixture(scope="module")
def model():
    from video_gcp_amd.model import GCPTreeModel
    from video_gcp_amd.params import init_params
    n = GCPTreeModel._n_models
    m = GCPTreeModel(HP, params=init_params(HP, seed=0), device=torch.device("cuda", 0))
    m.eval()
    yield m
    GCPTreeModel._n_models = max(n, GCPTreeModel._n_models) + 8      # later modules' models: streams none of these used


@pytest.mark.parametrize("closed_loop", [True, False])
def test_runner_record_is_consistent(model, closed_loop):
    """the record, not a chaotic trajectory: the states are step_numpy's of the recorded actions, the frames the renders of the states,
    and every action is what ImageCEMPolicy gives for that episode's recorded frames and plans -- bit for bit: the runner encodes one
    frame per call, as _infer_action does, and the inverse model's rows do not depend on their batch-mates.  (Measured once, for the
    record: the encoder + inverse model on a top-down frame alone and in a batch of 3 differ by 0.0 at both control shapes,
    profiles/control_time.jsonl -- no bound is needed, and none is used.)"""
    E = 3
    planner = ShortPlans(P.HierarchicalCEMPlanner(P.GCPImageSimulator(model), P.LearnedCostEstimate(model), 4, [3, 3], n_ll_samples=5,
                                                  action_dim=32, max_seq_len=12, fast_draws=True, seed=1), 4)
    env = NE.NavEnvBatch(9, CW, T, IMG, DEV)
    runner = CT.ControlRunner(model, planner, env, replan_interval=T + 2, num_max_replans=10, closed_loop_execution=closed_loop)
    tasks = NE.draw_tasks(9, 2, range(E))
    res = runner.run(tasks)
    assert res["full_traj"].shape == (E, T + 1, 3) and res["actions"].shape == (E, T, 2) and np.isfinite(res["actions"]).all()
    frames, goal_frames = env.frames.cpu().numpy(), env.goal_frames.cpu().numpy()
    goal_pix = DS.topdown_pixels(tasks["goal"], 9, env.scale, env.S, env.cw)
    for t in range(T + 1):
        assert np.array_equal(frames[:, t], _frames_numpy(env, res["full_traj"][:, t], goal_pix)), t
    for e in range(E):
        ref = NE.rollout_numpy(9, tasks["start"][e], tasks["goal"][e], res["actions"][e])
        assert np.array_equal(ref["full_traj"].view(np.uint32), res["full_traj"][e].view(np.uint32))
        assert np.array_equal(ref["blocked"], res["blocked"][e].astype(bool))
        assert abs(ref["path_len"] - res["path_len"][e]) <= 1e-9 and np.abs(ref["goal_dist"] - res["all_goal_distances"][e]).max() <= 1e-9
        # the policy of the reference's loop, one episode at a time, on the recorded frames and plans
        replay = Replay(runner.plans[e], frames[e])
        policy = P.ImageCEMPolicy(model, replay, replan_interval=T + 2, num_max_replans=10, closed_loop_execution=closed_loop)
        planned_at = []
        for t in range(T):
            before = replay.calls
            a = np.asarray(policy.act(t=t, i_tr=0, images=frames[e, :t + 1], goal_image=goal_frames[e][None]).actions, dtype=np.float32)
            if replay.calls != before:
                planned_at.append(t)
            assert np.array_equal(a.view(np.uint32), res["actions"][e, t].view(np.uint32)), (e, t, a, res["actions"][e, t])
        assert planned_at == [p["t"] for p in runner.plans[e]] and replay.calls == len(runner.plans[e]) == res["n_replans"][e]
        # a plan of n <= 4 frames is used up after n - 1 steps: the next plan is made at that step
        lens = [p["image_plan"].shape[0] for p in runner.plans[e]]
        assert planned_at[0] == 0 and all(b - a == n - 1 for a, b, n in zip(planned_at[:-1], planned_at[1:], lens[:-1]))
        assert len(planned_at) >= 2 and planned_at[-1] + lens[-1] - 1 >= T


# ---- the entry point ------------------------------------------------------------------------------------------------------------------------
def test_control_main_end_to_end(tmp_path, capsys):
    conf = tmp_path / "mod_hyper.py"
    conf.write_text(CONF.format(env_params="n_rooms=9, crop_window=40, heading_smoothing=0.1, init_pos=None, goal_pos=None",
                                env_cls="TopdownMultiroom3dEnv", T=T))
    out = str(tmp_path / "out")
    from video_gcp_amd import nav_gen as NG
    NG.write_spec_and_assets(str(tmp_path / "nav"), 9, T, crop_window=CW)      # a nav dataset's topdown_assets.npz
    res = CT.main(["--experiment", str(conf), "--data_dir", str(tmp_path / "data"), "--exp_dir", str(tmp_path / "exp"), "--random_weights", "1",
                   "--n_tasks", "2", "--task_seed", "3", "--out", out, "--topdown_assets", str(tmp_path / "nav" / "topdown_assets.npz")])
    K = 2
    assert sorted(os.listdir(out)) == ["control_results.npz", "task_0_traj.png", "task_1_traj.png"]     # and a picture per task
    shapes = dict(improvement=(K,), initial_dist=(K,), final_dist=(K,), all_goal_distances=(K, T + 1), full_traj=(K, T + 1, 3), goal=(K, 2),
                  path_len=(K,), blocked=(K, T), reset_state=(K, 5), term_t=(K,), actions=(K, T, 2))
    with np.load(os.path.join(out, "control_results.npz")) as z:
        assert set(shapes) <= set(z.files)
        for k, shape in shapes.items():
            assert z[k].shape == shape and np.array_equal(z[k], res[k]), k
        tasks = NE.draw_tasks(9, 3, range(K))
        assert np.array_equal(z["reset_state"], np.concatenate([tasks["start"], tasks["goal"]], axis=1))
        assert np.array_equal(z["full_traj"][:, 0], tasks["start"]) and (z["term_t"] == T - 1).all()
        assert np.array_equal(z["improvement"], z["initial_dist"] - z["final_dist"]) and np.isfinite(z["actions"]).all()
    capsys.readouterr()
    perf = CP.main(["--path", os.path.join(out, "control_results.npz"), "--n_rooms", "9", "--max_seq_len", "100"])
    lines = capsys.readouterr().out.strip().split("\n")
    assert perf["n_tasks"] == K and 0.0 <= perf["success"] <= 1.0 and perf["room2goal_mean"] >= 1.0
    assert lines[0].startswith("Success: \t") and lines[1].startswith("Cost: \t") and lines[3].startswith("Room2Goal: \t") and \
        lines[4].startswith("RTravers: \t")
