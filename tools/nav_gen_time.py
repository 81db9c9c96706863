"""Trajectories per second of the nav data generator (nav_gen.NavGenerator.generate) at 9 and 25 rooms, beside the reference's PRM.

  device    generate(--n) with the defaults of PrmPolicy (50 samples per room, 3 per door, n_knn 10), wall time around the call after
            a warm-up call (the call synchronises once per planning attempt: the host must know who needs another);
  kernels   the four launches of one planning attempt (points, road map, shortest path, resample) for --n trajectories, device events;
  baseline  the reference's generate_roadmap + dijkstra_planning, executed by tests/golden/make_ref_prm_goldens.py on the golden
            inputs (case b: 9 rooms, 5-room sequence, 264 nodes; case d: 25 rooms, longest sequence, 1 271 nodes) on the build
            machine's CPU and stored in tests/golden/ref_prm.npz as seconds per plan.
Prints one JSON line per layout; --out appends them to a file under profiles/.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import video_gcp_amd  # noqa: F401
    from video_gcp_amd import nav_gen as NG

    with np.load(os.path.join(ROOT, "tests", "golden", "ref_prm.npz")) as z:
        ref = {9: (float(z["ref_seconds_per_plan_9rooms"]), int(z["case_b/kept"].sum()) + 2),
               25: (float(z["ref_seconds_per_plan_25rooms"]), int(z["case_d/kept"].sum()) + 2)}
    lines = []
    for n_rooms in (9, 25):
        gen = NG.NavGenerator(n_rooms, T=100, seed=0)
        gen.generate(min(a.n, 64))
        torch.cuda.synchronize()
        wall = []
        for r in range(a.rounds):
            gen.start_index = (r + 1) * a.n
            t0 = time.perf_counter()
            res = gen.generate(a.n)
            torch.cuda.synchronize()
            wall.append(time.perf_counter() - t0)
        tasks = [gen.draw_task(i, 0) for i in range(min(a.n, gen.CHUNK))]
        tasks = [t for t in tasks if t["n_steps"] >= 2]
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        gen.plan_batch(tasks, 0)
        torch.cuda.synchronize()
        e[0].record()
        o = gen.plan_batch(tasks, 0)
        e[1].record()
        gen.resample_into(o, [t["n_steps"] for t in tasks], torch.cuda.current_stream().cuda_stream)
        e[2].record()
        e[2].synchronize()
        nodes = o["n_nodes"].cpu().numpy()
        sec, ref_nodes = ref[n_rooms]
        best = min(wall)
        lines.append({"workload": "nav_gen_time", "n_rooms": n_rooms, "n": a.n, "traj_per_s": round(a.n / best, 1),
                      "wall_s": [round(w, 4) for w in wall], "redrawn": int(res["redraws"].sum()),
                      "attempt_batch": len(tasks), "attempt_plan_ms": round(e[0].elapsed_time(e[1]), 3),
                      "attempt_resample_ms": round(e[1].elapsed_time(e[2]), 3), "nodes_mean": round(float(nodes.mean()), 1),
                      "nodes_max": int(nodes.max()), "success_rate": round(float(o["success"].float().mean()), 4),
                      "reference_s_per_plan": round(sec, 3), "reference_nodes": ref_nodes,
                      "reference_plans_per_s": round(1.0 / sec, 2), "speedup_over_reference_plan": round(a.n / best * sec, 1)})
        print(json.dumps(lines[-1]), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            for l in lines:
                f.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
