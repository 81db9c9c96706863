"""Executed steps per second of the closed-loop control experiment at the 9-room and 25-room control shapes, random weights.

  batched   control.ControlRunner over --E tasks at once: nav_env.NavEnvBatch (gcpx_nav_env_step, gcpx_topdown_assemble_batch), plans per
            episode, the closed-loop encoder one frame per call, the inverse model on all rows;
  serial    the same tasks (the first --serial of them) one episode at a time, the way the reference's GeneralAgent.rollout runs:
            planning.ImageCEMPolicy.act on the frames so far, nav_env.step_numpy, dataset.render_topdown_numpy + resize_frames_numpy.
Both loops make the same plans per episode (at t = 0 and when a plan is used up); the time inside the planner is measured apart, so
that `steps_per_s` (everything) and `exec_steps_per_s` (planner time taken out) can both be read.  --steps caps agent.T.
Also measured once: the largest difference between the encoder + inverse model on a frame alone and on the same frame in a batch of 3
(`row_alone_vs_batch3_max_abs`), the figure behind the runner's one-frame-per-call encoding.
--batch_plans: instead of the serial loop, the batched loop twice over the same tasks, --repeats times each: plans per episode (the
planner call of the loop above) and plans per step (ControlRunner(batch_plans=True): the planner's plan_batch); planner
seconds, calls, tasks per call and the t = 0 call (all --E tasks) apart, each as the list of the repeats.  --max_rows: the rows per
forward of plan_batch (one value: used by the loop; several: the t = 0 call alone is timed with each first).
--batch_encode: instead of the serial loop, the batched loop with the closed-loop encoder one frame per call and with one
encode_frames launch per step (ControlRunner(batch_encode=True), csrc/enc_frames.hip), taking turns over the same tasks, --repeats times
each: wall and planner seconds, executed steps per second and microseconds per episode-step with the planner time taken out.
--planner vmpc / seq_latent (with --batch_plans): the same template over the flat predictor (model_cls = SequentialModel), re-planned at
every step -- visual MPC (base_configs.vmpc, act_cond, action sequences scored by L2ImageCost, the best sample executed) and CEM in the
latents of gcp_sequential (learned cost, closed loop); --keep_plans 0 leaves the plans of the plans-per-step loop on the device,
--decode_candidates 1 decodes every candidate while scoring.  The population (MPC_CEM) is written into the line.
Prints one JSON line per shape; --out appends them to a file under profiles/.
"""
import argparse
import json
import os
import sys
import tempfile
import textwrap
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# the settings of experiments/control/{9room,25room}/{gcp_tree,gcp_sequential}/mod_hyper.py (--planner tree / flat)
CONF = textwrap.dedent('''
    from blox import AttrDict
    from gcp.planning.infra.agent.benchmarking_agent import BenchmarkAgent
    from gcp.planning.infra.envs.miniworld_env.multiroom3d.multiroom3d_env import TopdownMultiroom3dEnv
    from gcp.planning.planner_policy import ImageCEMPolicy
    from gcp.planning.cem.sampler import {sampler}
    from gcp.planning.cem.cem_planner import HierarchicalImageCEMPlanner
    from gcp.planning.cem.cost_fcn import {cost}
    from gcp.prediction.models.sequential import SequentialModel
    from experiments.prediction.base_configs import {base} as base_conf

    agent = AttrDict(type=BenchmarkAgent, env=(TopdownMultiroom3dEnv, dict(init_pos=None, goal_pos=None, n_rooms={n_rooms},
                     heading_smoothing=0.1, crop_window=40)), T={T}, image_height=32, image_width=32)
    h_config = AttrDict(base_conf.model_config)
    h_config.update(dict(state_dim=2, ngf=16, max_seq_len={seq}, hierarchy_levels={levels}, nz_mid_lstm=512, n_lstm_layers=3, nz_mid=128,
                         nz_enc=128, nz_vae=256, regress_length=True, attach_state_regressor=True, attach_inv_mdl=True,
                         inv_mdl_params=AttrDict(n_actions=2, use_convs=False, build_encoder=False),
                         decoder_distribution='discrete_logistic_mixture'))
    h_config.update(dict({model_extra}))
    h_config.pop("add_weighted_pixel_copy")
    cem_params = AttrDict(prune_final=True, horizon={horizon}, action_dim={action_dim}, verbose=False, {cem_extra},
                          n_level_hierarchy={levels}, sampler={sampler},
                          cost_fcn={cost}, cost_config=AttrDict(checkpt_path='none'))
    policy = AttrDict(type=ImageCEMPolicy, params=h_config, checkpt_path='none', cem_planner=HierarchicalImageCEMPlanner,
                      cem_params=cem_params, replan_interval={replan}, closed_loop_execution={closed_loop}{policy_extra})
    config = AttrDict(start_index=0, end_index=99, agent=agent, policy=policy)
''')
# cem_params of .../gcp_tree/mod_hyper.py (the hierarchical planner) and of .../gcp_sequential/mod_hyper.py (the flat planner, same model)
TREE_MODEL = dict(base="gcp_tree", model_extra="", action_dim=256, horizon=None, replan="agent.T + 2", closed_loop=True, policy_extra="")
# the flat predictor (model_cls = SequentialModel), re-planned at every step.  No shipped conf fixes these populations: MPC_CEM is this
# tool's choice, written into every line it prints
MPC_CEM = dict(batch_size=10, n_iters=2, elite_frac=0.3, horizon=10)
MPC_EXTRA = "n_iters={n_iters}, batch_size={batch_size}, elite_frac={elite_frac}".format(**MPC_CEM)
MPC_POLICY = ", model_cls=SequentialModel, num_max_replans=agent.T"
PLANNERS = {"tree": dict(TREE_MODEL, sampler="ImageHierarchicalTreeCEMSampler", cost="ImageLearnedCostEstimate",
                         cem_extra="n_iters=3, batch_size=10, sampling_rates_per_layer=[10, 10]"),
            "flat": dict(TREE_MODEL, sampler="SimpleTreeCEMSampler", cost="ImageWrappedLearnedCostFcn",
                         cem_extra="n_iters=1, batch_size=5, elite_frac=1.0"),
            # visual MPC: base_configs.vmpc + act_cond, action sequences scored in pixel space, the best sample executed open loop
            "vmpc": dict(base="vmpc", model_extra="nz_vae=0, attach_inv_mdl=False, lstm_init='zero'", action_dim=2, horizon=MPC_CEM["horizon"], replan=1,
                         closed_loop=False, policy_extra=MPC_POLICY + ", act_cond=True", sampler="FlatCEMSampler", cost="L2ImageCost",
                         cem_extra=MPC_EXTRA + ", use_inferred_actions=False, dense_cost=True"),
            # CEM in the latents of the goal-conditioned flat predictor, the learned cost, closed-loop execution
            "seq_latent": dict(base="gcp_sequential", model_extra="lstm_init='zero'", action_dim=256, horizon=MPC_CEM["horizon"], replan=1,
                               closed_loop=True, policy_extra=MPC_POLICY, sampler="FlatCEMSampler", cost="ImageLearnedCostEstimate",
                               cem_extra=MPC_EXTRA)}
SHAPES = {9: dict(n_rooms=9, T=200, seq=100, levels=7), 25: dict(n_rooms=25, T=400, seq=200, levels=8)}


class TimedPlanner:
    """the planner, with the wall time spent inside it (device work included) and its calls counted"""

    def __init__(self, planner, torch):
        self.planner, self.torch, self.seconds, self.calls = planner, torch, 0.0, 0
        self.tasks_per_call, self.first_call_s, self.max_rows = [], None, None

    @property
    def device_plans(self):
        return getattr(self.planner, "device_plans", False)

    def plan_batch(self, states, goals, **kw):
        self.torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = self.planner.plan_batch(states, goals, max_rows=self.max_rows, **kw)
        self.torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        self.seconds += dt
        self.calls += 1
        self.tasks_per_call.append(len(states))
        if self.first_call_s is None:
            self.first_call_s = dt
        return out

    def __call__(self, state, goal):
        self.torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = self.planner(state, goal)
        self.torch.cuda.synchronize()
        self.seconds += time.perf_counter() - t0
        self.calls += 1
        return out


def time_batch_plans(a, torch, CT, model, planner, env, tasks, desc, n_rooms, T):
    """the batched loop with plans per episode and with plans per step, --repeats runs each, on the same tasks"""
    import numpy as np
    row = {"workload": "control_time", "batch_plans": True, "planner": a.planner, "n_rooms": n_rooms, "E": a.E, "T": T, "max_seq_len": desc.hp.max_seq_len,
           "repeats": a.repeats}
    sweep = a.max_rows or [planner.MAX_ROWS]
    if len(sweep) > 1:                                   # the t = 0 call alone, per rows-per-forward (second of two calls: the first warms up)
        env.reset(tasks)
        frames, goals = env.frames[:, 0].cpu().numpy(), env.goal_frames.cpu().numpy()
        row["t0_call_s_by_max_rows"] = {}
        for mr in sweep:
            timed = TimedPlanner(planner, torch)
            timed.max_rows = mr
            timed.plan_batch(frames, goals)
            timed.first_call_s = None
            timed.plan_batch(frames, goals)
            row["t0_call_s_by_max_rows"][str(mr)] = round(timed.first_call_s, 4)
        best = min(sweep, key=lambda mr: row["t0_call_s_by_max_rows"][str(mr)])
    else:
        best = sweep[0]
    row["max_rows"] = best
    runs = {False: [], True: []}
    for flag in (False, True):
        timed = TimedPlanner(planner, torch)
        timed.max_rows = best
        runner = CT.ControlRunner(model, timed, env, batch_plans=flag, keep_plans=bool(a.keep_plans) or not flag, **desc.policy_args)
        runner.run({k: v[:2] for k, v in tasks.items()})            # warm-up: plans and buffers of both kinds of call
        for _ in range(a.repeats):
            timed.seconds, timed.calls, timed.tasks_per_call, timed.first_call_s = 0.0, 0, [], None
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = runner.run(tasks)
            torch.cuda.synchronize()
            runs[flag].append(dict(wall=time.perf_counter() - t0, planner=timed.seconds, calls=timed.calls, plans=int(res["n_replans"].sum()),
                                   tasks=list(timed.tasks_per_call), first=timed.first_call_s))
    per, bat = runs[False], runs[True]
    r3 = lambda xs: [round(x, 4) for x in xs]
    row.update(per_episode_wall_s=r3([r["wall"] for r in per]), per_episode_planner_s=r3([r["planner"] for r in per]),
               per_episode_plans=[r["plans"] for r in per],
               per_episode_ms_per_plan=r3([1e3 * r["planner"] / max(r["plans"], 1) for r in per]),
               batched_wall_s=r3([r["wall"] for r in bat]), batched_planner_s=r3([r["planner"] for r in bat]),
               batched_plans=[r["plans"] for r in bat], plan_batch_calls=[r["calls"] for r in bat],
               tasks_per_call_mean=r3([float(np.mean(r["tasks"])) for r in bat]), tasks_per_call_max=[int(max(r["tasks"])) for r in bat],
               batched_ms_per_plan=r3([1e3 * r["planner"] / max(r["plans"], 1) for r in bat]),
               t0_call_s=r3([r["first"] for r in bat]),
               t0_call_ms_per_plan=r3([1e3 * r["first"] / r["tasks"][0] for r in bat]),
               per_episode_steps_per_s=[round(a.E * T / r["wall"], 1) for r in per], batched_steps_per_s=[round(a.E * T / r["wall"], 1) for r in bat],
               batched_keep_plans=bool(a.keep_plans))
    if a.planner in ("vmpc", "seq_latent"):
        row.update(cem=dict(MPC_CEM), replan_interval=1, candidates_decoded=bool(planner.decode_candidates))
    return row


def time_batch_encode(a, torch, CT, model, planner, env, tasks, desc, n_rooms, T):
    """the batched loop with one encoder call per frame and with one encode_frames launch per step, taking turns, --repeats runs each, on
    the same tasks; plans per step when --batch_plans is given too"""
    row = {"workload": "control_time", "batch_encode": True, "batch_plans": bool(a.batch_plans), "planner": a.planner, "n_rooms": n_rooms,
           "E": a.E, "T": T, "max_seq_len": desc.hp.max_seq_len, "repeats": a.repeats}
    timed = TimedPlanner(planner, torch)
    timed.max_rows = (a.max_rows or [planner.MAX_ROWS])[0] if a.batch_plans else None
    runners = {flag: CT.ControlRunner(model, timed, env, batch_plans=bool(a.batch_plans), batch_encode=flag, **desc.policy_args)
               for flag in (False, True)}
    for flag in (False, True):
        runners[flag].run({k: v[:2] for k, v in tasks.items()})     # warm-up: plans and buffers of both kinds of call
    runs = {False: [], True: []}
    for _ in range(a.repeats):
        for flag in (False, True):
            timed.seconds, timed.calls, timed.tasks_per_call, timed.first_call_s = 0.0, 0, [], None
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = runners[flag].run(tasks)
            torch.cuda.synchronize()
            runs[flag].append(dict(wall=time.perf_counter() - t0, planner=timed.seconds, plans=int(res["n_replans"].sum())))
    r3 = lambda xs: [round(x, 4) for x in xs]
    for flag, tag in ((False, "per_frame"), (True, "batch_encode")):
        rs = runs[flag]
        row.update({f"{tag}_wall_s": r3([r["wall"] for r in rs]), f"{tag}_planner_s": r3([r["planner"] for r in rs]),
                    f"{tag}_plans": [r["plans"] for r in rs],
                    f"{tag}_exec_steps_per_s": [round(a.E * T / max(r["wall"] - r["planner"], 1e-9), 1) for r in rs],
                    f"{tag}_exec_us_per_episode_step": r3([1e6 * (r["wall"] - r["planner"]) / (a.E * T) for r in rs])})
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--E", type=int, default=100)
    ap.add_argument("--serial", type=int, default=None, help="episodes of the one-at-a-time loop (default: --E)")
    ap.add_argument("--steps", type=int, default=None, help="steps per episode (default: the conf's agent.T, 200 / 400)")
    ap.add_argument("--rooms", type=int, nargs="+", default=[9, 25])
    ap.add_argument("--out", default=None)
    ap.add_argument("--planner", choices=sorted(PLANNERS), default="tree", help="the conf's planner: tree = gcp_tree (hierarchical), "
                    "flat = gcp_sequential (CEMPlanner over all tree latents); over the flat predictor, re-planned at every step "
                    "(with --batch_plans): vmpc = visual MPC (action sequences, L2ImageCost), seq_latent = CEM in its latents")
    ap.add_argument("--decode_candidates", type=int, default=0, help="1 = the flat planner decodes the images of every candidate while it scores "
                    "(CEMPlanner.decode_candidates; a hand-written cost always does)")
    ap.add_argument("--keep_plans", type=int, default=1, help="--batch_plans: 0 = the plans-per-step loop keeps its plans on the device "
                    "(ControlRunner(keep_plans=False))")
    ap.add_argument("--batch_plans", action="store_true", help="time planning per step (plan_batch) beside planning per episode")
    ap.add_argument("--repeats", type=int, default=3, help="--batch_plans: runs of each loop")
    ap.add_argument("--max_rows", type=int, nargs="+", default=None, help="--batch_plans: candidate rows per forward of plan_batch")
    ap.add_argument("--batch_encode", action="store_true", help="time the batched loop with one encoder call per frame and with one "
                    "encode_frames launch per step (ControlRunner(batch_encode=True)), taking turns, --repeats runs each; with "
                    "--batch_plans both plan per step")
    a = ap.parse_args()
    import numpy as np
    import torch
    import video_gcp_amd  # noqa: F401
    from video_gcp_amd import conf_loader as CL
    from video_gcp_amd import control as CT
    from video_gcp_amd import dataset as DS
    from video_gcp_amd import nav_env as NE
    from video_gcp_amd import planning as P

    dev = torch.device("cuda", 0)
    lines = []
    for n_rooms in a.rooms:
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "mod_hyper.py")
            with open(path, "w") as f:
                kw = dict(SHAPES[n_rooms], **PLANNERS[a.planner])
                kw["horizon"] = kw["horizon"] or kw["seq"]
                f.write(CONF.format(**kw))
            conf = CL.exec_control_conf(path, {})
        desc, env_desc = CL.planner_from_control_conf(conf), CL.environment_from_control_conf(conf)
        model, planner, _ = CL.build_policy(desc, dev, seed=0, random_weights=True, verbose=False)
        if a.decode_candidates:
            planner.decode_candidates = True
        T = min(a.steps or env_desc.T, env_desc.T)
        tasks = NE.draw_tasks(n_rooms, 0, range(a.E))
        env = NE.NavEnvBatch(n_rooms, env_desc.crop_window, T, env_desc.img_sz, dev)

        # one frame alone against the same frame in a batch of 3: encoder + inverse model
        row_diff = enc_diff = None
        if model._hp.attach_inv_mdl and not (a.batch_plans or a.batch_encode):
            obs = NE.NavEnvBatch(n_rooms, env_desc.crop_window, 1, env_desc.img_sz, dev).reset({k: v[:3] for k, v in tasks.items()})
            target = torch.randn(3, model._hp.nz_enc, generator=torch.Generator().manual_seed(0)).to(dev)
            together = model.inv_mdl.run_single(model.encode(obs), target)
            alone = torch.cat([model.inv_mdl.run_single(model.encode(obs[e:e + 1]), target[e:e + 1]) for e in range(3)])
            row_diff = float((together - alone).abs().max())
            enc_diff = float((model.encode(obs) - torch.cat([model.encode(obs[e:e + 1]) for e in range(3)])).abs().max())

        if a.batch_encode:
            lines.append(time_batch_encode(a, torch, CT, model, planner, env, tasks, desc, n_rooms, T))
            print(json.dumps(lines[-1]), flush=True)
            del model, planner, env
            torch.cuda.empty_cache()
            continue

        if a.batch_plans:
            lines.append(time_batch_plans(a, torch, CT, model, planner, env, tasks, desc, n_rooms, T))
            print(json.dumps(lines[-1]), flush=True)
            del model, planner, env
            torch.cuda.empty_cache()
            continue

        # batched
        timed = TimedPlanner(planner, torch)
        runner = CT.ControlRunner(model, timed, env, **desc.policy_args)
        runner.run({k: v[:2] for k, v in tasks.items()})            # warm-up: plans and buffers of both kinds of call
        timed.seconds, timed.calls = 0.0, 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = runner.run(tasks)
        torch.cuda.synchronize()
        wall_b, plan_b, calls_b = time.perf_counter() - t0, timed.seconds, timed.calls

        # one episode at a time
        n_serial = min(a.serial or a.E, a.E)
        walls = NE.wall_table(env.rps)
        timed = TimedPlanner(planner, torch)
        goal_pix = DS.topdown_pixels(tasks["goal"], n_rooms, env.scale, env.S, env.cw)

        def frame_of(state, e):
            pix = DS.topdown_pixels(state[None, :2], n_rooms, env.scale, env.S, env.cw)
            return DS.resize_frames_numpy(DS.render_topdown_numpy(env.assets, pix, goal_pix[e]), env_desc.img_sz)[0]

        torch.cuda.synchronize()
        t0 = time.perf_counter()
        final = []
        for e in range(n_serial):
            policy = P.ImageCEMPolicy(model, timed, **desc.policy_args)
            state = tasks["start"][e].copy()
            goal_image = frame_of(np.concatenate([tasks["goal"][e], [0.0]]).astype(np.float32), e)[None]
            frames = [frame_of(state, e)]
            for t in range(T):
                act = np.asarray(policy.act(t=t, i_tr=e, images=np.stack(frames), goal_image=goal_image).actions, dtype=np.float32)
                state = NE.step_numpy(state, act, walls)["state"]
                frames.append(frame_of(state, e))
            final.append(state)
        torch.cuda.synchronize()
        wall_s, plan_s, calls_s = time.perf_counter() - t0, timed.seconds, timed.calls
        lines.append({"workload": "control_time", "n_rooms": n_rooms, "E": a.E, "T": T, "max_seq_len": desc.hp.max_seq_len,
                      "batched_wall_s": round(wall_b, 3), "batched_planner_s": round(plan_b, 3), "batched_plans": calls_b,
                      "batched_steps_per_s": round(a.E * T / wall_b, 1),
                      "batched_exec_steps_per_s": round(a.E * T / max(wall_b - plan_b, 1e-9), 1),
                      "serial_episodes": n_serial, "serial_wall_s": round(wall_s, 3), "serial_planner_s": round(plan_s, 3),
                      "serial_plans": calls_s, "serial_steps_per_s": round(n_serial * T / wall_s, 1),
                      "serial_exec_steps_per_s": round(n_serial * T / max(wall_s - plan_s, 1e-9), 1), "planner": a.planner,
                      "blocked_fraction": round(float(res["blocked"].mean()), 4),
                      "row_alone_vs_batch3_max_abs": row_diff, "encoder_alone_vs_batch3_max_abs": enc_diff})
        print(json.dumps(lines[-1]), flush=True)
        del model, planner, runner, env
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for l in lines:
                f.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
