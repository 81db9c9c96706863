"""What the receding-horizon options of the flat batch planner cost per call: one `CEMPlanner.plan_batch(device=True)` call over --E tasks
with the options off (the call as it was before they existed: the same launches) and with all three on -- a warm start from the previous
call's best samples moved up one step, half of the elites carried, AR(1) noise (gcpx_cem_warm_start, gcpx_cem_population_ex) -- at the
control shapes of tools/control_time.py over the flat predictor, random weights: visual MPC (`vmpc`: action sequences, L2ImageCost,
candidates decoded) and CEM in the latents of gcp_sequential (`seq_latent`: the learned cost).  Same population either way: the options
change what the rows hold, not how many are rolled out.

Both kinds of call are warmed up, then timed taking turns, --repeats times each, a host clock around the call between two device
synchronisations; the line holds every time, the medians, the spread (max - min) of each kind and the ratio of the medians.  What the
options buy -- fewer iterations or candidates for the same plan -- needs trained weights and is not measured here.
Prints one JSON line per planner; --out appends them to a file under profiles/."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

OPTIONS = dict(noise_rho=0.5, keep_elites=0.5, warm_std=0.5)
OFF = dict(noise_rho=0.0, keep_elites=0.0, warm_std=1.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--E", type=int, default=100)
    ap.add_argument("--rooms", type=int, default=9, choices=(9, 25))
    ap.add_argument("--planners", nargs="+", default=["vmpc", "seq_latent"], choices=("vmpc", "seq_latent"))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import video_gcp_amd  # noqa: F401
    from control_time import CONF, MPC_CEM, PLANNERS, SHAPES
    from video_gcp_amd import conf_loader as CL
    from video_gcp_amd import nav_env as NE

    if not torch.cuda.is_available():
        raise RuntimeError("cem_warm_time measures on the GPU: no device found")
    dev = torch.device("cuda", 0)
    lines = []
    for name in a.planners:
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "mod_hyper.py")
            with open(path, "w") as f:
                f.write(CONF.format(**dict(SHAPES[a.rooms], **PLANNERS[name])))
            conf = CL.exec_control_conf(path, {})
        desc, env_desc = CL.planner_from_control_conf(conf), CL.environment_from_control_conf(conf)
        model, planner, _ = CL.build_policy(desc, dev, seed=0, random_weights=True, verbose=False)
        env = NE.NavEnvBatch(a.rooms, env_desc.crop_window, 1, env_desc.img_sz, dev)
        env.reset(NE.draw_tasks(a.rooms, 0, range(a.E)))
        frames, goals = env.frames[:, 0], env.goal_frames
        shift = torch.ones(a.E, dtype=torch.int32, device=dev)
        n_elite = max(int(planner.batch_size * planner.elite_frac), 1)

        def call(on):
            planner.set_receding(**(OPTIONS if on else OFF))
            warm = dict(warm=(planner.batch_best, shift)) if on else {}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            planner.plan_batch(frames, goals, device=True, latents=bool(desc.policy_args["closed_loop_execution"]), **warm)
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        call(False)                                          # the first plan: what the warm calls start from
        for _ in range(a.warmup):
            call(False), call(True)
        times = {False: [], True: []}
        for _ in range(a.repeats):
            for on in (False, True):
                times[on].append(call(on))
        planner.set_receding(**OFF)
        med = {on: statistics.median(ts) for on, ts in times.items()}
        r4 = lambda xs: [round(1e3 * x, 3) for x in xs]
        s = planner._sampler
        lines.append({"workload": "cem_warm_time", "planner": name, "n_rooms": a.rooms, "E": a.E, "max_seq_len": desc.hp.max_seq_len,
                      "cem": dict(MPC_CEM), "sample": [s._n_steps, s._action_dim], "rows_per_iteration": a.E * planner.batch_size,
                      "options": dict(OPTIONS, m=int(OPTIONS["keep_elites"] * n_elite), shift=1), "repeats": a.repeats, "warmup": a.warmup,
                      "off_ms": r4(times[False]), "on_ms": r4(times[True]),
                      "off_median_ms": round(1e3 * med[False], 3), "on_median_ms": round(1e3 * med[True], 3),
                      "off_spread_ms": round(1e3 * (max(times[False]) - min(times[False])), 3),
                      "on_spread_ms": round(1e3 * (max(times[True]) - min(times[True])), 3),
                      "on_over_off": round(med[True] / med[False], 4)})
        print(json.dumps(lines[-1]), flush=True)
        del model, planner, env
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for l in lines:
                f.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
