"""Planning entry point: `python -m video_gcp_amd.plan --config c4 --weights <ckpt> --nstart_goal_pairs K [--planner cem|hierarchical]`,
or `python -m video_gcp_amd.plan --experiment <experiments/control/.../mod_hyper.py> --exp_dir D --data_dir D`: model, planner and cost
from a control configuration in the reference's format (gcp/planning/run.py <mod_hyper.py>; conf_loader.planner_from_control_conf).

Counterpart of the device path behind /root/reference/gcp/planning/run.py: for every (start, goal) image pair the planner
(`CEMPlanner` / `HierarchicalCEMPlanner`, gcp/planning/cem/cem_planner.py:55-218) searches the latent space of the
goal-conditioned predictor and returns (image_plan, actions, latents, cost) (cem_planner.py:96).  What run.py adds around
that — the MiniWorld simulator, agents, policies, trajectory savers (gcp/planning/infra/*) — is host infrastructure outside
SURVEY.md §8 and is not rebuilt here (the executed loop is video_gcp_amd.control): start / goal frames come from an .npz (`--pairs file.npz` with uint8 arrays `start`,
`goal` [K, H, W, 3]) or are seeded synthetic images.  Two ways to use several GPUs, as in the reference and in SURVEY §8(e):
  * one process per GPU over disjoint pair ranges (run.py:78-94 splits start_index..end_index over workers) — `--split pairs`;
  * one process per GPU sharing every CEM population (candidates sharded, one all-gather of costs per iteration) —
    `--split candidates` (the default under torch.distributed.run)."""
import argparse
import json
import os

import numpy as np
import torch


_NOT_WITH_EXPERIMENT = ("config", "planner", "candidates", "iters", "elite_frac")       # the conf decides these


def get_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--experiment", default="", help="a control configuration in the reference's format (mod_hyper.py): model "
                   "hyper-parameters, planner, sampler, cost, weights path and pair range come from it")
    p.add_argument("--data_dir", default="", help="GCP_DATA_DIR as the --experiment file sees it")
    p.add_argument("--exp_dir", default="", help="GCP_EXP_DIR as the --experiment file sees it")
    p.add_argument("--random_weights", type=int, default=0, help="with --experiment: 1 = plan on the seeded initialisation when the "
                   "conf's checkpoint does not resolve (an error otherwise)")
    p.add_argument("--config", default="c4")
    p.add_argument("--weights", default="", help="checkpoint (weights_ep*.pth); random init when empty")
    p.add_argument("--use_ema", type=int, default=0, choices=(0, 1), help="1 = plan on the checkpoint's averaged weights (trained with "
                   "--ema_decay), the cost model's own checkpoint included; an error when a checkpoint holds none")
    p.add_argument("--pairs", default="", help=".npz with uint8 `start`, `goal` [K, H, W, 3]")
    p.add_argument("--nstart_goal_pairs", type=int, default=4)
    p.add_argument("--planner", default="cem", choices=["cem", "hierarchical"])
    p.add_argument("--candidates", type=int, default=512)
    p.add_argument("--iters", type=int, default=3)
    p.add_argument("--elite_frac", type=float, default=0.1)
    p.add_argument("--split", default="candidates", choices=["candidates", "pairs"])
    p.add_argument("--out", default="", help="directory for plan_{i}.npz")
    p.add_argument("--topdown_assets", default="", help="a nav dataset's topdown_assets.npz: when the plan carries regressed states, "
                   "plan_{i}_inferStateTraj.png (the state trajectory on the maze) is written next to plan_{i}.npz, which then "
                   "also holds `states`")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--reference_rng", action="store_true",
                   help="hierarchical planner: replay the reference's np.random call sequence draw for draw (6x the host time per "
                        "call) instead of drawing only the kept rows from a seeded numpy Generator")
    args = p.parse_args(argv)
    if args.experiment:
        given = [k for k in _NOT_WITH_EXPERIMENT if getattr(args, k) != p.get_default(k)]
        if given:
            raise ValueError(f"--experiment decides {', '.join('--' + k for k in given)}: do not give them together with it")
    return args


def main(argv=None):
    from . import dist as D
    from .checkpoint import load_weights
    from .hparams import config
    from .model import GCPTreeModel
    from .params import init_params
    from . import planning as P
    args = get_args(argv)
    rank, local_rank, world = D.init_from_env()
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    desc = None
    if args.experiment:
        from . import conf_loader as CL
        env = {k: v for k, v in (("GCP_DATA_DIR", args.data_dir), ("GCP_EXP_DIR", args.exp_dir)) if v}
        desc = CL.planner_from_control_conf(CL.exec_control_conf(args.experiment, env))
        for k in desc.ignored:
            print(f"[plan] not used from {os.path.basename(args.experiment)}: {k}", flush=True)
        hp = desc.hp
        model, planner, _ = CL.build_policy(desc, dev, weights=args.weights or None, seed=args.seed,
                                            random_weights=bool(args.random_weights), reference_rng=args.reference_rng,
                                            verbose=desc.verbose and bool(args.out), use_ema=bool(args.use_ema))
    else:
        hp = config(args.config)
        model = GCPTreeModel(hp, params=init_params(hp, seed=args.seed), device=dev)
        if args.use_ema and not args.weights:
            raise ValueError("--use_ema 1 needs --weights: averaged weights exist only in a checkpoint")
        if args.weights:
            load_weights(args.weights, model, use_ema=bool(args.use_ema))
        model.eval()                                                 # planner_policy.py:51
    if args.pairs:
        z = np.load(args.pairs)
        starts, goals = z["start"], z["goal"]
    else:
        rng = np.random.RandomState(args.seed)
        K = args.nstart_goal_pairs
        starts = rng.randint(0, 256, size=(K, hp.img_sz, hp.img_sz, 3)).astype(np.uint8)
        goals = rng.randint(0, 256, size=(K, hp.img_sz, hp.img_sz, 3)).astype(np.uint8)
    idx = list(range(len(starts)))
    if desc is not None and args.pairs and desc.pairs[0] is not None:        # run.py: start_index..end_index (inclusive) of the pair file
        lo, hi = int(desc.pairs[0]), int(desc.pairs[1] if desc.pairs[1] is not None else len(starts) - 1)
        idx = [i for i in idx if lo <= i <= hi]
    if args.split == "pairs" and world > 1:                          # run.py:78-94: disjoint index ranges per worker
        per = (len(idx) + world - 1) // world
        idx = idx[rank * per:(rank + 1) * per]
        if torch.distributed.is_initialized():                       # no collective on this path: plan alone
            torch.distributed.destroy_process_group()
    sim, cost = P.GCPImageSimulator(model), P.LearnedCostEstimate(model)
    if desc is not None:                                             # build_policy made the planner
        del sim, cost
    elif args.planner == "cem":
        sampler = P.SimpleTreeCEMSampler(float("inf"), None, hp.nz_vae, 1.0, n_level_hierarchy=hp.hierarchy_levels, device=dev,
                                         seed=args.seed + 1)
        planner = P.CEMPlanner(sim, cost, sampler, n_iters=args.iters, batch_size=args.candidates, elite_frac=args.elite_frac,
                               max_seq_len=hp.max_seq_len)
    else:
        planner = P.HierarchicalCEMPlanner(sim, cost, hp.hierarchy_levels, [10, 10], action_dim=hp.nz_vae,       # rates of the
                                           max_seq_len=hp.max_seq_len,                                       # 25-room control config
                                           fast_draws=not args.reference_rng, seed=args.seed + 1)
    renderer = None
    if args.topdown_assets and args.out:                             # log_single_topdown_traj (logger.py:255-261, cem_planner.py:244-250)
        from .dataset import load_topdown_assets
        from .image_log import TrajectoryRenderer
        renderer = TrajectoryRenderer(load_topdown_assets(args.topdown_assets), dev)
    results = []
    for i in idx:
        r = planner.plan(starts[i:i + 1], goals[i:i + 1])
        plan, actions, latents, c, states = r.predictions, r.actions, r.latents, r.cost, r.states
        results.append({"pair": int(i), "cost": float(c), "plan_len": int(plan.shape[0])})
        if args.out and (rank == 0 or args.split == "pairs"):
            os.makedirs(args.out, exist_ok=True)
            drawn = renderer is not None and states is not None and len(states) and np.asarray(states).shape[-1] == 2
            extra = {"states": np.asarray(states)} if drawn else {}                   # the drawn states travel with the picture
            np.savez_compressed(os.path.join(args.out, f"plan_{i}.npz"), image_plan=plan, latents=latents,
                                actions=(actions if actions is not None else np.zeros(0)), cost=c, **extra)
            if drawn:
                from .image_log import write_trajectory_png
                write_trajectory_png(os.path.join(args.out, f"plan_{i}_inferStateTraj.png"), renderer, states, dev, lib=model.lib)
            if getattr(planner, "verbose", False):                   # ImageCEMPlanner.log_verbose (cem_planner.py:222-254)
                from .image_log import planner_pictures, write_planner_pictures
                for rp, vlog in enumerate(planner.verbose_logs):
                    write_planner_pictures(args.out, i, rp, planner_pictures(model, vlog, starts[i:i + 1], desc.horizon, renderer))
        if getattr(planner, "verbose", False):
            planner.verbose_logs.clear()
    if rank == 0 or args.split == "pairs":
        print(json.dumps({"rank": rank, "plans": results}), flush=True)
    return results


if __name__ == "__main__":
    main()
