"""-m gpu: control experiments over the flat predictor (policy.model_cls = SequentialModel), from the conf text to the executed actions.

The confs are tests/test_flat_control_conf_cpu.py's at the widths every flat-predictor test of this suite runs (the c1 widths: nz_enc =
nz_mid = nz_mid_lstm = 128, three LSTM layers; 32 x 32 frames), max_seq_len 12, random weights:
  visual MPC   base_configs.vmpc + act_cond, FlatCEMSampler over action sequences [11, 2], L2ImageCost, use_inferred_actions = False,
               no inverse model, horizon 5, replan_interval 1
  latent CEM   base_configs.gcp_sequential, FlatCEMSampler over z [11, 256], the learned cost, closed-loop execution, horizon 5
Shapes: E = 3 episodes of 6 steps in the 9-room maze, 5 candidates, 2 iterations, max_rows = 10: the K n = 15 rows of a step are no
multiple of the 16-row GEMM tile, and the scoring forwards hold two tasks (10 rows), then one (5 rows).

Everything is compared bit for bit: an executed action is a row of a sample (visual MPC) or the inverse model's output for recorded
frames and latents (closed loop), which the per-episode ImageCEMPolicy computes by the same calls from the recorded plans -- the method
of tests/test_gpu_cem_batch.py::test_runner_with_batched_flat_plans."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from video_gcp_amd import conf_loader as CL  # noqa: E402
from video_gcp_amd import control as CT  # noqa: E402
from video_gcp_amd import nav_env as NE  # noqa: E402
from video_gcp_amd import planning as P  # noqa: E402
from test_flat_control_conf_cpu import FLAT_CONF, SEQ_LATENT, VMPC  # noqa: E402
from test_gpu_nav_env import CW, IMG, T as TE, Replay  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E, HORIZON, N_CAND, N_ITERS, MAX_ROWS, SEQ = 3, 5, 5, 2, 10, 12
WIDE = "nz_mid_lstm=128, lstm_init='zero'"
GPU_VMPC = dict(VMPC, widths=WIDE)
GPU_LATENT = dict(SEQ_LATENT, widths=WIDE, params=SEQ_LATENT["params"].replace("nz_vae=8", "nz_vae=256"), action_dim=256, horizon=HORIZON)


def describe(tmp, conf):
    p = tmp / "mod_hyper.py"
    p.write_text(FLAT_CONF.format(**conf))
    return CL.planner_from_control_conf(CL.exec_control_conf(str(p), {}))


def _built(tmp_path_factory, conf):
    from video_gcp_amd.model import GCPTreeModel
    n = GCPTreeModel._n_models
    desc = describe(tmp_path_factory.mktemp("conf"), conf)
    model, planner, policy = CL.build_policy(desc, torch.device("cuda", 0), seed=0, random_weights=True)
    yield desc, model, planner, policy
    GCPTreeModel._n_models = max(n, GCPTreeModel._n_models) + 8      # later modules' models: streams none of these used


@pytest.fixture(scope="module")
def vmpc(tmp_path_factory):
    yield from _built(tmp_path_factory, GPU_VMPC)


@pytest.fixture(scope="module")
def latent(tmp_path_factory):
    yield from _built(tmp_path_factory, GPU_LATENT)


class Counting:
    """the planner with both kinds of call counted, plan_batch at max_rows = MAX_ROWS; `forwards`: the rows of every rollout"""
    device_plans = True

    def __init__(self, planner):
        self.planner, self.single_calls, self.batch_calls, self.forwards, self.host_rollouts = planner, 0, [], [], 0
        sim = planner._sim
        dev_roll, host_roll = sim.rollout_device, sim.rollout

        def rollout_device(state, goal, samples, *a, **k):
            self.forwards.append(int(samples.shape[0]))
            return dev_roll(state, goal, samples, *a, **k)

        def rollout(*a, **k):
            self.host_rollouts += 1
            return host_roll(*a, **k)
        sim.rollout_device, sim.rollout = rollout_device, rollout    # (instance attributes over the class's methods)

    def close(self):
        del self.planner._sim.rollout_device, self.planner._sim.rollout

    def reseed(self):
        self.planner._sampler._gen.manual_seed(1)                    # build_policy(seed=0): the planner draws from seed + 1

    def __call__(self, state, goal):
        self.single_calls += 1
        return self.planner(state, goal)

    def plan_batch(self, states, goals, **kw):
        self.batch_calls.append(len(states))
        return self.planner.plan_batch(states, goals, max_rows=MAX_ROWS, **kw)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def run(desc, model, planner, **kw):
    env = NE.NavEnvBatch(9, CW, TE, IMG, DEV)
    counting = Counting(planner)
    counting.reseed()
    try:
        runner = CT.ControlRunner(model, counting, env, **dict(desc.policy_args, **kw))
        res = runner.run(NE.draw_tasks(9, 2, range(E)))
    finally:
        counting.close()
    return env, runner, counting, res


def check_against_the_policy(desc, model, env, runner, res):
    """every executed action is what a per-episode ImageCEMPolicy gives on the recorded frames and plans"""
    frames, goal_frames = env.frames.cpu().numpy(), env.goal_frames.cpu().numpy()
    for e in range(E):
        replay = Replay(runner.plans[e], frames[e])
        policy = P.ImageCEMPolicy(model, replay, **desc.policy_args)
        for t in range(TE):
            a = np.asarray(policy.act(t=t, i_tr=0, images=frames[e, :t + 1], goal_image=goal_frames[e][None]).actions, dtype=np.float32)
            assert np.array_equal(bits(a), bits(res["actions"][e, t])), (e, t, a, res["actions"][e, t])
        assert replay.calls == len(runner.plans[e]) == res["n_replans"][e] == TE          # a plan at every step
        assert [p["t"] for p in runner.plans[e]] == list(range(TE))


def test_build_policy_acts_from_the_best_sample(vmpc):
    from video_gcp_amd.sequential import GCPSequentialModel
    desc, model, planner, _ = vmpc
    assert isinstance(model, GCPSequentialModel) and isinstance(planner._sim, P.ActCondGCPImageSimulator)
    assert planner.horizon == HORIZON and not planner.use_inferred_actions and planner.decode_candidates
    rng = np.random.RandomState(3)
    frames = rng.randint(0, 256, size=(5, IMG, IMG, 3)).astype(np.uint8)
    goal = rng.rand(1, IMG, IMG, 3).astype(np.float32)
    best, sim = [], planner._sim
    host_roll = sim.rollout

    def rollout(state, goal_, samples, *a, **k):                     # the final rollout of a plan is made from its best sample
        best.append(np.array(samples, dtype=np.float32))
        return host_roll(state, goal_, samples, *a, **k)
    sim.rollout = rollout
    try:
        policy = P.ImageCEMPolicy(model, planner, replan_interval=3, num_max_replans=6)
        steps = []
        for t in range(5):
            a = policy.act(t=t, i_tr=0, images=frames[:t + 1], goal_image=goal).actions
            step = policy.current_exec_step - 1
            steps.append(step)
            assert best[-1].shape == (1, SEQ - 1, 2) and np.array_equal(bits(a), bits(best[-1][0, step])), t
            assert policy.image_plan.shape == (HORIZON, 3 * IMG * IMG + 128) and policy.latent_plan.shape == (HORIZON, 128)
            assert np.array_equal(bits(policy.action_plan), bits(best[-1][0]))            # the whole sample, not cut to the horizon
        assert steps == [0, 1, 2, 0, 1] and len(best) == policy.num_replans == 2 and np.isfinite(policy.plan_cost)
        assert float(np.abs(best[-1]).max()) <= 2.0                  # sampler_clip_val
    finally:
        del sim.rollout


@pytest.fixture(scope="module")
def vmpc_runs(vmpc):
    desc, model, planner, _ = vmpc
    return {(bp, kp): run(desc, model, planner, batch_plans=bp, keep_plans=kp) for bp, kp in ((False, True), (True, True), (True, False))}


@pytest.mark.parametrize("batch_plans", [False, True])
def test_runner_as_visual_mpc(vmpc, vmpc_runs, batch_plans):
    desc, model, planner, _ = vmpc
    env, runner, counting, res = vmpc_runs[batch_plans, True]
    assert res["actions"].shape == (E, TE, 2) and np.isfinite(res["actions"]).all() and (res["n_replans"] == TE).all()
    check_against_the_policy(desc, model, env, runner, res)
    for e in range(E):
        for p in runner.plans[e]:
            assert p["image_plan"].shape[0] == p["latent_plan"].shape[0] == HORIZON and p["action_plan"].shape == (SEQ - 1, 2)
    if batch_plans:
        # one plan_batch call per step carries all episodes: two scoring forwards (two tasks, then one) per iteration, then the plans
        assert counting.single_calls == 0 and counting.batch_calls == [E] * TE
        assert counting.forwards == ([2 * N_CAND, N_CAND] * N_ITERS + [E]) * TE
    else:
        assert counting.single_calls == E * TE and counting.batch_calls == []
        assert counting.forwards == ([N_CAND] * N_ITERS + [1]) * (E * TE)


def test_plans_that_stay_on_the_device(vmpc_runs):
    """keep_plans=False with batch_plans: plan_batch(device=True) -- the same seeds, the same executed actions, no host copy of a plan"""
    _, kept_runner, _, kept = vmpc_runs[True, True]
    env, runner, counting, res = vmpc_runs[True, False]
    assert np.array_equal(bits(res["actions"]), bits(kept["actions"])) and np.array_equal(bits(res["full_traj"]), bits(kept["full_traj"]))
    assert (res["n_replans"] == TE).all() and counting.batch_calls == [E] * TE and counting.single_calls == 0
    # neither a decoded final rollout nor any other: the plan is the best sample
    assert counting.host_rollouts == 0 and counting.forwards == ([2 * N_CAND, N_CAND] * N_ITERS) * TE
    for e in range(E):
        assert [sorted(p) for p in runner.plans[e]] == [["cost", "t"]] * TE
        assert all(type(p["t"]) is int and type(p["cost"]) is float for p in runner.plans[e])
        assert [p["cost"] for p in runner.plans[e]] == [p["cost"] for p in kept_runner.plans[e]]


def test_latent_conf_closed_loop(latent):
    desc, model, planner, _ = latent
    from video_gcp_amd.sequential import GCPSequentialModel
    assert isinstance(model, GCPSequentialModel) and type(planner._sim) is P.GCPImageSimulator and not planner._sim.pred_length
    assert desc.policy_args["closed_loop_execution"] and planner.use_inferred_actions and planner.horizon == HORIZON
    env, runner, counting, res = run(desc, model, planner, batch_plans=True, keep_plans=True)
    assert np.isfinite(res["actions"]).all() and (res["n_replans"] == TE).all() and counting.batch_calls == [E] * TE
    check_against_the_policy(desc, model, env, runner, res)
    p = runner.plans[0][0]
    # _cap_to_horizon cuts each list to its first `horizon` entries: 5 of the 12 frames and latents, 5 of the 11 actions
    assert p["latent_plan"].shape == (HORIZON, 128) and p["action_plan"].shape == (HORIZON, 2) and p["image_plan"].shape[0] == HORIZON
    # the same run with the plans kept on the device: the final rollout's latents are read there
    env2, runner2, counting2, res2 = run(desc, model, planner, batch_plans=True, keep_plans=False)
    assert counting2.host_rollouts == 0 and counting2.forwards == ([2 * N_CAND, N_CAND] * N_ITERS + [E]) * TE
    assert np.array_equal(bits(res2["actions"]), bits(res["actions"]))
    assert [sorted(q) for q in runner2.plans[0]] == [["cost", "t"]] * TE


def test_control_main_on_a_visual_mpc_conf(tmp_path):
    conf = tmp_path / "mod_hyper.py"
    conf.write_text(FLAT_CONF.format(**GPU_VMPC))
    out = str(tmp_path / "out")
    res = CT.main(["--experiment", str(conf), "--random_weights", "1", "--n_tasks", "2", "--task_seed", "3", "--out", out,
                   "--batch_plans", "1", "--keep_plans", "0"])
    with np.load(os.path.join(out, "control_results.npz")) as z:
        assert set(CT.RESULT_KEYS) <= set(z.files)
        for k in CT.RESULT_KEYS:
            assert z[k].shape[0] == 2 and np.array_equal(z[k], res[k]), k
        assert z["actions"].shape == (2, TE, 2) and np.isfinite(z["actions"]).all() and float(np.abs(z["actions"]).max()) <= 2.0


@pytest.mark.parametrize("which", ["vmpc", "latent"])
def test_candidates_scored_without_the_decoder(request, which):
    """rollout_device(decode=False) on both flat simulators: the plan without decoder and head launches returns no images, and latents
    and lengths equal to the decoding rollout's bit for bit (the same launches compute them); under the learned cost a plan made with
    and without decoded candidates has the same cost and the same best sample"""
    desc, model, planner, _ = request.getfixturevalue(which)
    sim, dim = planner._sim, (2 if which == "vmpc" else 256)
    assert sim.supports_latent_only
    rng = np.random.RandomState(8)
    states, goals = (rng.randint(0, 256, size=(2, IMG, IMG, 3)).astype(np.uint8) for _ in range(2))
    z = torch.randn(N_CAND, SEQ - 1, dim, generator=torch.Generator().manual_seed(4)).to(DEV)
    full = sim.rollout_device(states[:1], goals[:1], z, SEQ)
    lat, lens, images = full.latents.clone(), full.lengths.clone(), full.images
    lean = sim.rollout_device(states[:1], goals[:1], z, SEQ, decode=False)
    assert lean.images is None and tuple(images.shape) == (N_CAND, SEQ, 3, IMG, IMG)
    assert np.array_equal(bits(lean.latents.cpu()), bits(lat.cpu())) and torch.equal(lean.lengths, lens) and lens.tolist() == [SEQ] * N_CAND
    assert bool(torch.isfinite(lean.latents).all()) and float(lean.latents[:, 1:].std()) > 0
    plans = {}
    for decoded in (False, True):
        sampler = P.FlatCEMSampler(2.0, SEQ - 1, dim, 0.5, device=DEV, seed=6)
        p = P.CEMPlanner(sim, P.LearnedCostEstimate(model), sampler, n_iters=N_ITERS, batch_size=N_CAND, elite_frac=0.4, max_seq_len=SEQ,
                         horizon=HORIZON, decode_candidates=decoded, use_inferred_actions=planner.use_inferred_actions)
        assert p.decode_candidates == decoded
        out = p.plan_batch(states, goals, record=True, max_rows=MAX_ROWS)
        plans[decoded] = (p.batch_record.best_samples.clone(), [o.cost for o in out], torch.stack(p.batch_record.scores).clone())
    assert plans[False][1] == plans[True][1] and all(np.isfinite(plans[False][1]))
    assert np.array_equal(bits(plans[False][0].cpu()), bits(plans[True][0].cpu())) and np.array_equal(bits(plans[False][2].cpu()), bits(plans[True][2].cpu()))


@pytest.mark.parametrize("conf", [GPU_VMPC, GPU_LATENT], ids=["vmpc", "latent"])
def test_plan_entry_point_on_a_flat_predictor_conf(tmp_path, conf):
    """plan.py --experiment goes through build_policy as control.py does: a plan per pair, cut to the horizon"""
    from video_gcp_amd import plan as PL
    path = tmp_path / "mod_hyper.py"
    path.write_text(FLAT_CONF.format(**conf))
    out = str(tmp_path / "plans")
    res = PL.main(["--experiment", str(path), "--random_weights", "1", "--nstart_goal_pairs", "2", "--out", out])
    assert [r["pair"] for r in res] == [0, 1] and all(r["plan_len"] == HORIZON and np.isfinite(r["cost"]) for r in res)
    with np.load(os.path.join(out, "plan_1.npz")) as z:
        assert z["image_plan"].shape == (HORIZON, 3 * IMG * IMG + 128) and z["latents"].shape == (HORIZON, 128)
        assert z["actions"].shape == ((SEQ - 1, 2) if conf is GPU_VMPC else (HORIZON, 2)) and np.isfinite(z["actions"]).all()
