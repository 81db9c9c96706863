"""`python -m video_gcp_amd.control_perf --path OUT/control_results.npz --n_rooms N [--n_tasks K] [--max_seq_len L]`: the reference's
control-performance numbers (gcp/evaluation/compute_control_perf.py) from the results of video_gcp_amd.control:

  Success     final room == goal room, averaged over the tasks
  Cost        path length (environment units) of a successful task, max_seq_len of a failed one, averaged
  Room2Goal   mean and standard deviation of len(plan_room_seq(final room, goal room))
  RTravers    mean and standard deviation of len(plan_room_seq(start room, final room))

Host only."""
import argparse

import numpy as np

from . import nav_layout as NL


def control_perf(results, n_rooms=9, n_tasks=None, max_seq_len=200):
    """results: the arrays of control_results.npz -- `full_traj` [K, T + 1, >= 2] and `reset_state` [K, 5] (its last two entries: the
    goal), environment units.  Returns dict(success, cost, room2goal_mean, room2goal_std, rtravers_mean, rtravers_std, n_tasks)."""
    layout = NL.layout(NL.rooms_per_side_of(n_rooms))
    paths, reset = np.asarray(results["full_traj"]), np.asarray(results["reset_state"])
    n_tasks = paths.shape[0] if n_tasks is None else int(n_tasks)
    if not 1 <= n_tasks <= paths.shape[0]:
        raise ValueError(f"n_tasks = {n_tasks}: the results hold {paths.shape[0]} tasks")
    success, penalized, to_goal, traversed = 0, 0.0, [], []
    for i in range(n_tasks):
        goal_pos, final_pos, start_pos = (np.array(v, dtype=np.float64) / 27 for v in (reset[i][-2:], paths[i][-1][:2], paths[i][0][:2]))
        for p in (goal_pos, final_pos, start_pos):
            p[1] *= -1
        goal_room, final_room, start_room = (layout.coords2ridx(p[0], p[1]) for p in (goal_pos, final_pos, start_pos))
        if final_room == goal_room:
            success += 1
        path = np.asarray(paths[i], dtype=np.float64)[:, :2]          # summed in float64 whatever the file holds
        path_len = np.sum(np.linalg.norm(path[1:] - path[:-1], axis=-1))
        penalized += path_len if final_room == goal_room else max_seq_len
        to_goal.append(len(NL.plan_room_seq(final_room, goal_room, layout.doors)))
        traversed.append(len(NL.plan_room_seq(start_room, final_room, layout.doors)))
    return dict(success=success / n_tasks, cost=float(penalized / n_tasks), room2goal_mean=float(np.mean(to_goal)),
                room2goal_std=float(np.std(to_goal)), rtravers_mean=float(np.mean(traversed)), rtravers_std=float(np.std(traversed)),
                n_tasks=n_tasks)


def report(perf):
    """the four lines compute_control_perf.py prints"""
    return ["Success: \t{}".format(perf["success"]), "Cost: \t{:.2f}".format(perf["cost"]), "",
            "Room2Goal: \t{}\t{}".format(perf["room2goal_mean"], perf["room2goal_std"]),
            "RTravers: \t{}\t{}".format(perf["rtravers_mean"], perf["rtravers_std"])]


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--path", required=True, help="control_results.npz written by video_gcp_amd.control")
    p.add_argument("--n_rooms", default=9, type=int, help="number of rooms in navigation layout")
    p.add_argument("--n_tasks", default=None, type=int, help="number of task instances in eval set (default: all in the file)")
    p.add_argument("--max_seq_len", default=200, type=int, help="maximum length of sequence (for cost computation)")
    args = p.parse_args(argv)
    with np.load(args.path) as z:
        results = {k: z[k] for k in ("full_traj", "reset_state")}
    perf = control_perf(results, args.n_rooms, args.n_tasks, args.max_seq_len)
    print("\n".join(report(perf)), flush=True)
    return perf


if __name__ == "__main__":
    main()
