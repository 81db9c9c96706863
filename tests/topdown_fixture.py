"""A seeded top-rendered (nav) dataset for the tests of the top-down data path: a GlobalSplit tree of `.npz` files WITHOUT images whose
states lie inside the maze, a dataset_spec.py naming Nav9Rooms, and `topdown_assets.npz` with a random background and asymmetric stamps
(agent and goal differ, neither equals its transpose or a flip of itself: a swapped axis or a swapped stamp cannot pass)."""
import math
import os

import numpy as np

from dataset_fixture import write_npz


def asymmetric_stamps(rng, k):
    """two different bool [k, k] stamps with the centre set, each unequal to its transpose, its flips and its half turn"""
    def one():
        while True:
            s = rng.rand(k, k) < 0.5
            s[k // 2, k // 2] = True
            if not any(np.array_equal(s, v) for v in (s.T, s[::-1], s[:, ::-1], s[::-1, ::-1], s[::-1, ::-1].T)):
                return s
    a, g = one(), one()
    while np.array_equal(a, g):
        g = one()
    return a, g


def make_assets(seed=0, n_rooms=9, scale=256, cw=40, k=11, agent_color=(0, 0, 255), goal_color=(0, 255, 0)):
    """the arrays of topdown_assets.npz (the data contract of video-gcp_amd/dataset.py) with random content"""
    rng = np.random.RandomState(seed)
    S = int((1 / 3) * int(math.sqrt(n_rooms)) * scale)
    a, g = asymmetric_stamps(rng, k)
    return dict(background=rng.randint(0, 256, size=(S + 2 * cw, S + 2 * cw, 3)).astype(np.uint8), crop_window=np.array(cw),
                n_rooms=np.array(n_rooms), render_scale=np.array(scale), agent_stamp=a, goal_stamp=g,
                agent_color=np.array(agent_color, dtype=np.uint8), goal_color=np.array(goal_color, dtype=np.uint8))


def write_assets(root, arrays):
    write_npz(os.path.join(root, "topdown_assets.npz"), arrays)


def states_for_pixels(pix, n_rooms, scale, S, cw):
    """float32 states [n, 2] whose picture pixels are `pix` (x, y): the middle of the pixel's cell, so float32 rounding cannot move it"""
    pix = np.asarray(pix, dtype=np.float64).reshape(-1, 2)
    half = 0.5 * (1 / 3) * int(math.sqrt(n_rooms))
    vx, vy = pix[:, 0] - cw, (S + cw) - pix[:, 1]                    # the truncated products int(q * scale)
    mid = lambda v: np.where(v == 0, 0.0, v + np.sign(v) * 0.5)      # a value that truncates to v (0 for v = 0)
    qx, qy = mid(vx) / scale, mid(vy) / scale
    return np.stack([(qx - half) * 27.0, -(qy - half) * 27.0], axis=1).astype(np.float32)


def write_spec(root, T, split, extra=""):
    with open(os.path.join(root, "dataset_spec.py"), "w") as f:
        f.write("from blox import AttrDict\nimport numpy as np\nfrom gcp.datasets.configs.nav_9rooms import Nav9Rooms\n"
                f"dataset_spec = AttrDict(\n    max_seq_len={T},\n    dataset_class=Nav9Rooms,\n"
                f"    split=AttrDict(train={split[0]}, val={split[1]}, test={split[2]}),\n{extra})\n")


def write_topdown_dataset(root, T, n_files, traj_per_file, seed=0, n_actions=2, min_len=None, split=(0.5, 0.25, 0.25), spec_extra="",
                          **asset_args):
    """`n_files` files `<root>/batch{f // 2}/file_{f}.npz` of ragged random walks inside the maze (states x, y, angle; no images), the
    spec and the assets; returns the asset arrays"""
    rng = np.random.RandomState(seed)
    arrays = make_assets(seed=seed + 1, **asset_args)
    lim = 4.5 * int(math.sqrt(int(arrays["n_rooms"])))
    for f in range(n_files):
        d = {"traj_per_file": np.array(traj_per_file)}
        for i in range(traj_per_file):
            n = int(rng.randint(min_len or max(3, T // 2), T + T // 2 + 1))
            xy = np.clip(rng.uniform(-lim, lim, size=(1, 2)) + np.cumsum(rng.randn(n, 2) * 0.6, axis=0), -lim, lim)
            d[f"traj{i}/states"] = np.concatenate([xy, rng.uniform(0, 6.28, size=(n, 1))], axis=1).astype(np.float32)
            d[f"traj{i}/actions"] = rng.randn(n - 1, n_actions).astype(np.float32)
            d[f"traj{i}/pad_mask"] = np.ones(n, dtype=np.float32)
        write_npz(os.path.join(root, f"batch{f // 2}", f"file_{f}.npz"), d)
    write_spec(root, T, split, spec_extra)
    write_assets(root, arrays)
    return arrays
