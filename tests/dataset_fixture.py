"""The fixture dataset of tests/golden/ref_dataset.npz written out in the `.npz` dataset layout, and a seeded c1 / c2-shaped dataset
for the loader tests."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_dataset.npz")
CASES = ("train", "val", "train_rl", "val_rl", "train_rs", "train_rl_std")
STATES_MEAN = np.array([0.25, -0.5], dtype=np.float32)      # as make_ref_dataset_goldens.py
STATES_STD = np.array([1.5, 0.75], dtype=np.float32)


def write_npz(path, d):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "wb") as f:
        np.savez(f, **d)


def write_golden_dataset(root):
    """the golden's folder-split tree under root (same file names as the reference saw); returns the loaded golden"""
    g = np.load(GOLDEN)
    files = {}
    for k in g.files:
        if k.startswith("data:"):
            _, name, key = k.split(":", 2)
            files.setdefault(name, {})[key] = g[k]
    for name, d in files.items():
        write_npz(os.path.join(root, name), d)
    return g


def write_spec(root, **entries):
    lines = ["import numpy as np", "from gcp.datasets.data_loader import FolderSplitVarLenVideoDataset", "dataset_spec = dict("]
    for k, v in entries.items():
        lines.append(f"    {k}={v},")
    lines.append(")")
    with open(os.path.join(root, "dataset_spec.py"), "w") as f:
        f.write("\n".join(lines) + "\n")


def write_random_dataset(root, T, img, n_files, traj_per_file, seed=0, state_dim=2, n_actions=2, phases=("train", "val"),
                         min_len=None):
    """seeded uint8 trajectories of ragged length around T in `<root>/hdf5/<phase>/`, plus a dataset_spec.py with max_seq_len = T"""
    rng = np.random.RandomState(seed)
    for phase in phases:
        for f in range(n_files):
            d = {"traj_per_file": np.array(traj_per_file)}
            for i in range(traj_per_file):
                n = int(rng.randint(min_len or max(3, T // 2), T + T // 2 + 1))
                d[f"traj{i}/images"] = rng.randint(0, 256, size=(n, img, img, 3)).astype(np.uint8)
                d[f"traj{i}/states"] = rng.randn(n, state_dim).astype(np.float32)
                d[f"traj{i}/actions"] = rng.randn(n - 1, n_actions).astype(np.float32)
                d[f"traj{i}/pad_mask"] = np.ones(n, dtype=np.float32)
            write_npz(os.path.join(root, "hdf5", phase, f"file_{f}.npz"), d)
    write_spec(root, max_seq_len=T)
