"""Golden data for control_perf from the REFERENCE's own code, executed (build container only: needs scipy and matplotlib).

It loads the reference's gcp/evaluation/compute_control_perf.py by path and calls its `main` on synthetic trajectories pickled to a
temporary file, with the stubs of make_ref_prm_goldens.py (`blox.AttrDict`, an empty `cv2`, a `Policy` base class, no textures), and
records what `main` prints.

Run from the repo root:  python tests/golden/make_ref_control_perf_goldens.py <reference checkout>
Writes tests/golden/ref_control_perf.npz (data only).  Per case: `full_traj` [K, T + 1, 3] and `reset_state` [K, 5] (environment units;
the pickle holds them as the reference's savers do: a list of trajectories, and a list of dicts whose `goal` ends in the goal), n_rooms,
max_seq_len, the printed lines and the numbers parsed from them (success, cost, room-to-goal mean / std, rooms-traversed mean / std).

`Cost` is printed with two decimals.  Case "exact" therefore walks axis-parallel steps whose lengths are multiples of 0.5: its four
successful tasks have path lengths 6, 2, 12 and 4, its four failed ones cost max_seq_len = 200, so the cost is 824 / 8 = 103 exactly.
The other cases walk seeded random steps: their cost is known to the printed two decimals only."""
import contextlib
import importlib.util
import io
import os
import pickle
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
OUT = os.path.join(HERE, "ref_control_perf.npz")


def run_reference(ccp, trajs, goals, n_rooms, max_seq_len):
    data = dict(full_traj=[np.array(t) for t in trajs],
                reset_state=[dict(goal=np.concatenate([np.asarray(t[0], dtype=np.float64), np.asarray(g, dtype=np.float64)]))
                             for t, g in zip(trajs, goals)])
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "traj_data.pkl")
        with open(path, "wb") as f:
            pickle.dump(data, f)
        argv, sys.argv = sys.argv, ["compute_control_perf.py", "--path", path, "--n_rooms", str(n_rooms), "--n_tasks", str(len(trajs)),
                                    "--max_seq_len", str(max_seq_len)]
        buf = io.StringIO()
        try:
            with contextlib.redirect_stdout(buf):
                ccp.main()
        finally:
            sys.argv = argv
    lines = buf.getvalue().split("\n")[:5]
    assert lines[0].startswith("Success: \t") and lines[1].startswith("Cost: \t") and lines[2] == ""
    assert lines[3].startswith("Room2Goal: \t") and lines[4].startswith("RTravers: \t"), lines
    values = [float(lines[0].split("\t")[1]), float(lines[1].split("\t")[1])] + [float(v) for v in lines[3].split("\t")[1:3]] + \
             [float(v) for v in lines[4].split("\t")[1:3]]
    return lines, np.array(values)


def random_walks(rng, K, T, half):
    """K seeded random walks of T steps inside the square |x|, |y| < half (environment units), with headings; and a goal each"""
    trajs = np.zeros((K, T + 1, 3), dtype=np.float32)
    for k in range(K):
        p = rng.uniform(-half, half, size=2)
        trajs[k, 0, :2] = p
        for t in range(T):
            step = rng.uniform(-1.5, 1.5, size=2)
            q = np.clip(p + step, -half, half)
            trajs[k, t + 1] = (q[0], q[1], np.arctan2(q[1] - p[1], q[0] - p[0]))
            p = q
    goals = rng.uniform(-half, half, size=(K, 2)).astype(np.float32)
    for k in range(0, K, 3):                                # every third task ends in its goal's room: at the goal
        goals[k] = trajs[k, -1, :2]
    return trajs, goals


def exact_walks():
    """8 tasks in the 9-room maze: axis-parallel steps of lengths 0.5 k; the successful ones have path lengths 6, 2, 12 and 4"""
    legs = [[(4.0, 0.0), (0.0, -2.0)], [(0.0, 2.0)], [(-6.0, 0.0), (0.0, 6.0)], [(1.5, 0.0), (0.0, 2.5)],
            [(9.0, 0.0)], [(0.0, -18.0)], [(-0.5, 0.0)], [(2.0, 0.0), (2.0, 0.0)]]
    starts = [(-2.0, 1.0), (9.0, 8.0), (3.0, -3.0), (-10.0, -10.0), (-10.0, 0.0), (-9.5, 9.0), (0.5, 0.5), (8.0, -9.0)]
    trajs = np.zeros((8, 5, 3), dtype=np.float32)
    goals = np.zeros((8, 2), dtype=np.float32)
    for k, (s, leg) in enumerate(zip(starts, legs)):
        p = np.array(s)
        trajs[k, 0, :2] = p
        for t in range(4):
            if t < len(leg):
                p = p + np.array(leg[t])
            trajs[k, t + 1, :2] = p
        goals[k] = p if k < 4 else (-p[0], -p[1] + 9.0 if abs(p[1]) < 4.5 else -p[1])
    return trajs, goals


def main():
    ref = sys.argv[1]
    import make_ref_prm_goldens as G
    lay, _, _, _ = G.load_reference(ref)
    lay.load_textures = lambda texture_dir: None            # no textures here; define_layout is called for its coords2ridx
    lay.default_texture_dir = lambda: "none"                # define_layout(n, None) asks for the downloaded datasets' texture folder
    spec = importlib.util.spec_from_file_location("ref_compute_control_perf", os.path.join(ref, "gcp", "evaluation", "compute_control_perf.py"))
    ccp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ccp)
    out = {}
    cases = dict(exact=(exact_walks(), 9, 200), walk9=(random_walks(np.random.RandomState(1), 12, 10, 13.0), 9, 200),
                 walk25=(random_walks(np.random.RandomState(2), 12, 20, 22.0), 25, 400))
    for name, ((trajs, goals), n_rooms, max_seq_len) in cases.items():
        lines, values = run_reference(ccp, trajs, goals, n_rooms, max_seq_len)
        print(name, lines)
        out[f"{name}/full_traj"] = trajs
        out[f"{name}/reset_state"] = np.concatenate([trajs[:, 0], goals], axis=1).astype(np.float32)
        out[f"{name}/n_rooms"], out[f"{name}/max_seq_len"] = np.int64(n_rooms), np.int64(max_seq_len)
        out[f"{name}/lines"], out[f"{name}/values"] = np.array(lines), values
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
