"""Closed-loop control experiments: `python -m video_gcp_amd.control --experiment <experiments/control/.../mod_hyper.py> --exp_dir D
--data_dir D [--random_weights 1] [--tasks tasks.npz | --task_seed S] [--n_tasks K] --out OUT`, the reference's
`python gcp/planning/run.py <mod_hyper.py>`: the planner's actions are executed in the maze, the agent re-observes, and the executed
trajectories are written for video_gcp_amd.control_perf (compute_control_perf.py).

ControlRunner is the batched form of BenchmarkAgent + ImageCEMPolicy (general_agent.py `rollout`, planner_policy.py:89-113,222-227): the
executed steps of all E tasks advance together on the device (nav_env.NavEnvBatch).
  planning    per episode through the planner object, at t = 0 and whenever ImageCEMPolicy.act's condition holds for that episode; a plan's
              length is known on the host when it is made, so the execution counters are host integers.  A re-plan reads that episode's
              current frame back: the only read-back of the loop.  With batch_plans (--batch_plans 1) the episodes that plan at a step
              plan together: one read-back of their frames, one planner.plan_batch call (HierarchicalCEMPlanner or the flat CEMPlanner).
              With the flat planner a re-plan can start from the episode's previous best sample (--warm_start 1, with --warm_std,
              --keep_elites, --noise_rho: receding-horizon CEM, which the reference does not have).
  plans       padded device tensors: latents [E, Lmax, nz], actions [E, Lmax, 2]
  a step      gather the next planned latent (closed loop) or the planned action (open loop) of every row; the encoder on the current
              frames; inv_mdl.run_single on all rows; env.step; env.observe
  the encoder its split-f16 convolution blocks share one power-of-two scale among the frames a workgroup stages (csrc/conv_enc_split.hip),
              so a frame's latent depends on its batch-mates in the last bits: the closed-loop encoding runs one frame per call, which is
              the call ImageCEMPolicy._infer_action makes.  The inverse model's rows are independent (csrc/mlp.hip: a row is a column of the
              MFMA tile) and run as one batch.  With batch_encode (--batch_encode 1) the frames of all episodes go through ONE launch of
              the frame-independent encoder (model.encode_frames, csrc/enc_frames.hip: exact f32, a frame's latent depends on that frame
              and the weights only), the call ImageCEMPolicy(batch_encode=True)._infer_action makes for one frame.  Not the bits of the
              default path (split-f16 with shared scales); both are within the oracle's latent tolerance.  It combines
              with --batch_plans and --reference_rng and changes nothing without closed_loop_execution.
  the model   the tree model, or the flat predictor of a conf with policy.model_cls = SequentialModel: visual MPC (act_cond: the best sample's
              actions, no inverse model needed) and CEM in its latents (conf_loader.build_policy); --keep_plans 0 for loops
              that re-plan at every step.
The loop runs agent.T steps, as GeneralAgent.rollout does: no early stop."""
import argparse
import json
import os

import numpy as np
import torch


class ControlRunner:
    """ControlRunner(model, planner, env, replan_interval, num_max_replans, closed_loop_execution).run(tasks) -> results (numpy)
    batch_plans: the episodes that plan at a step plan together, one `planner.plan_batch` call (any planner that has one:
    HierarchicalCEMPlanner, CEMPlanner) and one read-back
    of their frames per step; off (the default), every episode plans through its own planner call.
    batch_encode: closed-loop acting encodes the current frames of all episodes in one `model.encode_frames` launch; off (the default),
    one `model.encode` call per frame.  An error if the model's encoder shape is not one `encode_frames` takes.
    keep_plans: `plans` holds a host copy of every plan made (the default); off, `dict(t, cost)` per plan, and with batch_plans and a
    planner that hands its plans over on the device (CEMPlanner.plan_batch(device=True)) neither frames nor plans visit the host: what
    a loop that re-plans at every step (visual MPC, replan_interval = 1) needs.
    warm_start (with batch_plans, the flat CEMPlanner): `best` [E, n_steps, dim] keeps every episode's last best sample on the device, and a
    re-plan starts from it moved up by the steps executed since: plan_batch(warm=(best[due], shift)), shift the episode's exec_step, -1
    for an episode without a plan.  The shifts go up as one small int32 tensor per planning step; the samples never visit the host."""

    def __init__(self, model, planner, env, replan_interval=1, num_max_replans=10, closed_loop_execution=False, batch_plans=False,
                 batch_encode=False, keep_plans=True, warm_start=False):
        self.model, self.planner, self.env = model, planner, env
        self.batch_plans, self.batch_encode, self.keep_plans = bool(batch_plans), bool(batch_encode), bool(keep_plans)
        self.warm_start, self.best = bool(warm_start), None
        if self.warm_start and not self.batch_plans:
            raise ValueError("warm_start re-plans through planner.plan_batch(warm=...): it needs batch_plans")
        if closed_loop_execution and not model._hp.attach_inv_mdl:
            raise ValueError("closed_loop_execution needs the model's inverse model (attach_inv_mdl)")
        if self.batch_encode:
            from .packing import encoder_frames_unsupported
            why = encoder_frames_unsupported(model._hp)
            if why:
                raise ValueError(f"batch_encode needs an encoder shape model.encode_frames takes ({why})")
        self.replan_interval, self.num_max_replans = int(replan_interval), int(num_max_replans)
        self.closed_loop_execution = bool(closed_loop_execution)
        # per episode, every plan made: dict(t, image_plan, action_plan, latent_plan, cost) (host copies); keep_plans=False: dict(t, cost)
        self.plans = []

    # -- planning: ImageCEMPolicy.act's condition and _plan, per episode --
    def _needs_plan(self, e, t):
        return (self.plan_len[e] is None or self.plan_len[e] - 1 <= self.exec_step[e]
                or (t % self.replan_interval == 0 and self.num_replans[e] < self.num_max_replans))

    def _store(self, e, actions, latents):
        dev = self.env.device
        n = max(len(latents), len(actions), 1)
        if self.lat is None:                                # the first plan gives the latents' width
            self.lat = torch.zeros(self.env.E, max(n, self._lmax), np.asarray(latents).shape[-1], device=dev)
            self.act = torch.zeros(self.env.E, max(n, self._lmax), self.model._hp.n_actions, device=dev)
        if n > self.lat.shape[1]:                           # a longer plan than any before: grow the padded tensors
            grow = lambda x: torch.cat([x, torch.zeros(x.shape[0], n - x.shape[1], x.shape[2], device=dev)], dim=1)
            self.lat, self.act = grow(self.lat), grow(self.act)
        self.lat[e, :len(latents)] = torch.as_tensor(np.asarray(latents), dtype=torch.float32).to(dev)
        if len(actions):
            self.act[e, :len(actions)] = torch.as_tensor(np.asarray(actions), dtype=torch.float32).reshape(len(actions), -1).to(dev)
        self.lat_len[e], self.act_len[e] = len(latents), len(actions)

    def _plan(self, e, t):
        frame = self.env.frames[e, t].cpu().numpy()         # the read-back of a re-plan
        goal = self.goal_frames_np[e]
        image_plan, action_plan, latent_plan, cost = self.planner(frame[None], goal[None])
        self._record(e, t, image_plan, action_plan, latent_plan, cost)

    def _warm(self, idx, due):
        """warm_start: plan_batch's `warm` for the episodes `due` (read before their counters are reset), as keyword arguments"""
        if not self.warm_start:
            return {}
        shift = torch.tensor([-1 if self.plan_len[e] is None else self.exec_step[e] for e in due], dtype=torch.int32).to(self.env.device)
        return dict(warm=(None if self.best is None else self.best[idx], shift))

    def _keep_best(self, idx):
        if not self.warm_start:
            return
        best = self.planner.batch_best
        if self.best is None:                               # the first plan gives the samples' shape
            self.best = torch.zeros((self.env.E,) + tuple(best.shape[1:]), device=best.device)
        self.best[idx.to(best.device)] = best

    def _plan_batch(self, due, t):
        """the episodes `due` at step t through one planner.plan_batch call; their frames come back in one copy"""
        if self._device_plans:
            return self._plan_batch_device(due, t)
        idx = torch.as_tensor(due, device=self.env.device)
        frames = self.env.frames[idx, t].cpu().numpy()
        plans = self.planner.plan_batch(frames, self.goal_frames_np[due], **self._warm(idx, due))
        self._keep_best(idx)
        for e, r in zip(due, plans):
            self._record(e, t, r.predictions, r.actions, r.latents, r.cost)

    def _plan_batch_device(self, due, t):
        """keep_plans=False: frames and plans stay on the device (CEMPlanner.plan_batch(device=True)): the frames of the due episodes go
        from env.frames to the planner as they are, the plans into `act` / `lat` with one indexed copy each; what comes back are the
        plans' costs and lengths (2 numbers per episode: the execution counters are host integers)"""
        dev = self.env.device
        idx = torch.as_tensor(due, device=dev)
        r = self.planner.plan_batch(self.env.frames[idx, t], self.env.goal_frames[idx], device=True, latents=self.closed_loop_execution,
                                    **self._warm(idx, due))
        self._keep_best(idx)
        K, A = len(due), r.actions.shape[1]
        L = r.latents.shape[1] if r.latents is not None else 0
        if self.act is None or self.act.shape[1] < max(A, L):
            n, E = max(A, L, self._lmax), self.env.E
            grow = lambda old, width: torch.zeros(E, n, width, device=dev) if old is None else \
                torch.cat([old, torch.zeros(E, n - old.shape[1], width, device=dev)], dim=1)
            self.act = grow(self.act, self.model._hp.n_actions)
            self.lat = grow(self.lat, self.model._hp.nz_enc)
        self.act[idx, :A] = r.actions.reshape(K, A, -1).to(torch.float32)
        if r.latents is not None:
            self.lat[idx, :L] = r.latents
        host = torch.stack([r.costs.to(torch.float64), r.lengths.to(torch.float64), r.n_actions.to(torch.float64)]).cpu().numpy()
        for j, e in enumerate(due):
            self.plan_len[e], self.exec_step[e] = int(host[1, j]), 0
            self.lat_len[e], self.act_len[e] = (int(host[1, j]) if r.latents is not None else 0), int(host[2, j])
            self.num_replans[e] += 1
            self.plans[e].append(dict(t=t, cost=float(host[0, j])))

    def _record(self, e, t, image_plan, action_plan, latent_plan, cost):
        actions = np.zeros((0, 2), dtype=np.float32) if action_plan is None else np.asarray(action_plan)
        self._store(e, actions, np.asarray(latent_plan))
        self.plan_len[e], self.exec_step[e] = int(np.asarray(image_plan).shape[0]), 0
        self.num_replans[e] += 1
        if self.keep_plans:
            self.plans[e].append(dict(t=t, image_plan=np.asarray(image_plan), action_plan=actions, latent_plan=np.asarray(latent_plan),
                                      cost=cost))
        else:
            self.plans[e].append(dict(t=t, cost=cost))

    # -- acting: ImageCEMPolicy.get_action for all rows --
    def _encode(self, obs):
        if self.batch_encode:
            return self.model.encode_frames(obs)
        return torch.cat([self.model.encode(obs[e:e + 1]) for e in range(obs.shape[0])], dim=0)

    def _actions(self, obs):
        E, dev = self.env.E, self.env.device
        if self.closed_loop_execution:
            idx = [s + 1 for s in self.exec_step]
            bad = [e for e in range(E) if idx[e] >= self.lat_len[e]]
            if bad:
                raise IndexError(f"episodes {bad}: the plan has no latent {[idx[e] for e in bad]} (ImageCEMPolicy.get_action)")
            target = self.lat[torch.arange(E, device=dev), torch.tensor(idx, device=dev)]
            return self.model.inv_mdl.run_single(self._encode(obs), target)
        idx =[min(s, max(n - 1, 0)) for s, n in zip(self.exec_step, self.act_len)]
        bad = [e for e in range(E) if self.act_len[e] >= 1 and self.exec_step[e] >= self.act_len[e]]
        if bad:
            raise IndexError(f"episodes {bad}: the action plan is used up (ImageCEMPolicy.get_action)")
        a = self.act[torch.arange(E, device=dev), torch.tensor(idx, device=dev)]
        for e in range(E):                                  # planner_policy.py:215-216: an empty action plan acts at random
            if self.act_len[e] < 1:
                a[e] = torch.as_tensor(0.05 * np.random.rand(2), dtype=torch.float32).to(dev)
        return a

    def run(self, tasks):
        env = self.env
        obs = env.reset(tasks)
        E, T, hp = env.E, env.T, self.model._hp
        self._lmax, self.lat, self.act = hp.max_seq_len + 2, None, None
        self.plan_len, self.exec_step, self.num_replans = [None] * E, [None] * E, [0] * E
        self.lat_len, self.act_len = [0] * E, [0] * E
        self.plans, self.best = [[] for _ in range(E)], None
        self.goal_frames_np = env.goal_frames.cpu().numpy()
        # plans per step that nobody keeps stay on the device, with a planner that can hand them over there
        self._device_plans = self.batch_plans and not self.keep_plans and bool(getattr(self.planner, "device_plans", False))
        for t in range(T):
            if self.batch_plans:
                due = [e for e in range(E) if self._needs_plan(e, t)]
                if due:
                    self._plan_batch(due, t)
            else:
                for e in range(E):
                    if self._needs_plan(e, t):
                        self._plan(e, t)
            env.step(self._actions(obs))
            self.exec_step = [s + 1 for s in self.exec_step]
            obs = env.observe()
        res = env.eval()
        res["reset_state"] = np.concatenate([np.asarray(tasks["start"], dtype=np.float32).reshape(E, 3),
                                             np.asarray(tasks["goal"], dtype=np.float32).reshape(E, 2)], axis=1)
        res["term_t"] = np.full(E, T - 1, dtype=np.int64)   # every episode runs its T steps
        res["actions"] = env.actions.cpu().numpy()
        res["n_replans"] = np.array(self.num_replans, dtype=np.int64)
        return res


RESULT_KEYS = ("improvement", "initial_dist", "final_dist", "all_goal_distances", "full_traj", "goal", "path_len", "blocked", "reset_state",
               "term_t", "actions")


def get_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--experiment", required=True, help="a control configuration in the reference's format (mod_hyper.py)")
    p.add_argument("--data_dir", default="", help="GCP_DATA_DIR as the --experiment file sees it")
    p.add_argument("--exp_dir", default="", help="GCP_EXP_DIR as the --experiment file sees it")
    p.add_argument("--random_weights", type=int, default=0, help="1 = run on the seeded initialisation when the conf's checkpoint does not "
                   "resolve (an error otherwise)")
    p.add_argument("--weights", default="", help="a checkpoint file instead of the conf's")
    p.add_argument("--use_ema", type=int, default=0, choices=(0, 1), help="1 = act on the checkpoint's averaged weights (trained with "
                   "--ema_decay), the cost model's own checkpoint included; an error when a checkpoint holds none")
    p.add_argument("--tasks", default="", help=".npz with `start` [K, 3] and `goal` [K, 2] in the environment's units")
    p.add_argument("--task_seed", type=int, default=0, help="without --tasks: the seed of the drawn tasks (NavGenerator.draw_task)")
    p.add_argument("--n_tasks", type=int, default=None, help="at most this many of the tasks start_index .. end_index of the conf")
    p.add_argument("--batch", type=int, default=100, help="episodes advanced together")
    p.add_argument("--T", type=int, default=None, help="steps per episode instead of the conf's agent.T")
    p.add_argument("--topdown_assets", default="", help="a nav dataset's topdown_assets.npz: the observation is rendered from its picture "
                   "(what the model was trained on), and OUT/task_{i}_traj.png shows the executed trajectory of every task")
    p.add_argument("--out", required=True, help="directory for control_results.npz")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--reference_rng", action="store_true", help="the hierarchical planner replays the reference's np.random sequence")
    p.add_argument("--batch_plans", type=int, default=0, help="1 = the episodes that plan at a step plan together (the planner's plan_batch, "
                   "hierarchical or flat): not the per-episode planner's bits, see DESIGN.md 5.7; not with --reference_rng")
    p.add_argument("--batch_encode", type=int, default=0, help="1 = closed-loop acting encodes the frames of all episodes in one launch of the "
                   "frame-independent encoder (model.encode_frames): not the default encoder's bits, see DESIGN.md 5.7; no effect without "
                   "closed_loop_execution; an error if the model's encoder shape is unsupported")
    p.add_argument("--keep_plans", type=int, default=1, help="0 = keep only the step and the cost of every plan (ControlRunner.plans); with "
                   "--batch_plans 1 and a flat planner the plans then stay on the device: no image plan is decoded or copied to the host")
    p.add_argument("--warm_start", type=int, default=0, choices=(0, 1), help="1 = a re-plan starts from the episode's previous best sample, moved "
                   "up by the steps executed since (ControlRunner(warm_start=True), DESIGN.md 5.7); with --batch_plans 1 and a flat planner")
    p.add_argument("--warm_std", type=float, default=None, help="in (0, 1]: the std of a warm start on the steps the previous plan covers, in "
                   "units of the sampler's initial std (CEMPlanner.warm_std)")
    p.add_argument("--keep_elites", type=float, default=None, help="in [0, 1): this fraction of an iteration's elites are candidates of the next "
                   "(CEMPlanner.keep_elites)")
    p.add_argument("--noise_rho", type=float, default=None, help="in [0, 1): AR(1) correlation of a candidate's noise along its steps "
                   "(CEMPlanner.noise_rho)")
    return p.parse_args(argv)


RECEDING_FLAGS = ("warm_start", "warm_std", "keep_elites", "noise_rho")


def receding_options(args):
    """the receding-horizon flags that were given, refused where they cannot apply: {flag: value}"""
    given = {k: getattr(args, k) for k in RECEDING_FLAGS if getattr(args, k) not in (None, 0)}
    if given and not args.batch_plans:
        raise ValueError(f"--{' --'.join(given)}: options of the flat planner's plan_batch, which plans per step: they need --batch_plans 1")
    if given and args.reference_rng:
        raise ValueError(f"--{' --'.join(given)}: plan_batch draws from a device generator; the reference's np.random stream "
                         "(--reference_rng) is defined per plan")
    return given


def apply_receding_options(planner, given):
    """hands --warm_std, --keep_elites and --noise_rho to the planner; refuses a planner whose plan_batch is not the flat CEMPlanner's"""
    from .planning import CEMPlanner
    if not given:
        return
    if getattr(type(planner), "plan_batch", None) is not CEMPlanner.plan_batch:
        raise ValueError(f"--{' --'.join(given)}: options of the flat CEMPlanner's plan_batch (warm starts, carried elites, correlated noise); "
                         f"the conf builds {type(planner).__name__}, which has none of them")
    planner.set_receding(**{k: v for k, v in given.items() if k != "warm_start"})


def main(argv=None):
    from . import conf_loader as CL
    from . import nav_env as NE
    args = get_args(argv)
    receding = receding_options(args)
    if args.batch_plans and args.reference_rng:
        raise ValueError("--batch_plans 1 plans on a device generator; the reference's np.random stream (--reference_rng) is defined per plan")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    # the shipped confs read both names while they execute; a name given nowhere gets a placeholder (with --random_weights no path is read)
    environ = {k: v or k.lower() for k, v in (("GCP_DATA_DIR", args.data_dir), ("GCP_EXP_DIR", args.exp_dir)) if v or k not in os.environ}
    conf = CL.exec_control_conf(args.experiment, environ)
    desc, env_desc = CL.planner_from_control_conf(conf), CL.environment_from_control_conf(conf)
    for k in env_desc.ignored:
        print(f"[control] not used from {os.path.basename(args.experiment)}: {k}", flush=True)
    model, planner, _ = CL.build_policy(desc, dev, weights=args.weights or None, seed=args.seed, random_weights=bool(args.random_weights),
                                        reference_rng=args.reference_rng, verbose=False, use_ema=bool(args.use_ema))
    apply_receding_options(planner, receding)
    needs_inv = [k for k, v in (("policy.closed_loop_execution = True", desc.policy_args["closed_loop_execution"]),
                                ("cem_params.use_inferred_actions = True", desc.get("action_source", "inverse_model") == "inverse_model")) if v]
    if needs_inv and not model._hp.attach_inv_mdl:
        raise ValueError(f"{' and '.join(needs_inv)}: the control loop needs the inverse model (attach_inv_mdl) for its actions")
    assets = None
    if args.topdown_assets:
        from .dataset import load_topdown_assets
        assets = load_topdown_assets(args.topdown_assets)
    T = int(args.T) if args.T else env_desc.T
    # run.py: the tasks start_index .. end_index (inclusive)
    lo = int(desc.pairs[0] or 0)
    if args.tasks:
        tasks = NE.load_tasks(args.tasks)
        hi = min(int(desc.pairs[1]) if desc.pairs[1] is not None else len(tasks["start"]) - 1, len(tasks["start"]) - 1)
        idx = list(range(lo, hi + 1))
        tasks = {k: v[idx] for k, v in tasks.items()}
    else:
        hi = int(desc.pairs[1]) if desc.pairs[1] is not None else lo + (args.n_tasks or 100) - 1
        idx = list(range(lo, hi + 1))
        if args.n_tasks is not None:
            idx = idx[:args.n_tasks]
        tasks = NE.draw_tasks(env_desc.n_rooms, args.task_seed, idx)
    if args.n_tasks is not None:
        idx = idx[:args.n_tasks]
        tasks = {k: v[:args.n_tasks] for k, v in tasks.items()}
    if not idx:
        raise ValueError("no task selected (start_index .. end_index of the conf, --n_tasks)")
    env = NE.NavEnvBatch(env_desc.n_rooms, env_desc.crop_window, T, env_desc.img_sz, dev, assets=assets)
    if args.batch_plans and not hasattr(planner, "plan_batch"):
        raise ValueError(f"--batch_plans 1 needs a planner with plan_batch; the conf builds {type(planner).__name__}, which has none")
    runner =ControlRunner(model, planner, env, batch_plans=bool(args.batch_plans), batch_encode=bool(args.batch_encode),
                           keep_plans=bool(args.keep_plans), warm_start=bool(args.warm_start), **desc.policy_args)
    parts = []
    for s in range(0, len(idx), max(args.batch, 1)):
        parts.append(runner.run({k: v[s:s + max(args.batch, 1)] for k, v in tasks.items()}))
    res = {k: np.concatenate([p[k] for p in parts], axis=0) for k in RESULT_KEYS}
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, "control_results.npz")
    np.savez_compressed(path, task_index=np.array(idx, dtype=np.int64), **res)
    if args.topdown_assets:
        from .image_log import TrajectoryRenderer, write_trajectory_png
        renderer = TrajectoryRenderer(assets, dev)
        for k, i in enumerate(idx):
            write_trajectory_png(os.path.join(args.out, f"task_{i}_traj.png"), renderer, res["full_traj"][k, :, :2], dev, lib=model.lib)
    print(json.dumps({"tasks": len(idx), "T": T, "results": path, "mean_final_dist": float(np.mean(res["final_dist"])),
                      "blocked_steps": int(res["blocked"].sum())}), flush=True)
    return res


if __name__ == "__main__":
    main()
