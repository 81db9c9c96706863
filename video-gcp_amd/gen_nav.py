"""python -m video_gcp_amd.gen_nav --n_rooms 9|16|25 --n_traj N --T 100 --out DIR [--seed S --traj_per_file K --crop_window 40 --split 0.9,0.05,0.05 --plain 0]

Writes a nav dataset (nav_gen.write_dataset): the GlobalSplit `.npz` tree without images, `dataset_spec.py` and `topdown_assets.npz`;
`python -m video_gcp_amd.train --path EXP --data_dir DIR` trains from it unchanged.  `--experiment <mod_hyper.py>` reads n_rooms,
crop_window, agent.T, start_index / end_index, traj_per_file and the policy's parameters from a data-collection conf in the reference's
format (experiments/data_gen/nav_16rooms/mod_hyper.py), through conf_loader's placeholder imports; flags given beside it win."""
import argparse
import os
import sys

from . import nav_gen as NG


def _plain(v):
    if isinstance(v, dict):
        return {k: _plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    return getattr(v, "__name__", repr(v))


def read_experiment(path):
    """a mod_hyper.py -> nav_gen.experiment_settings of its `config`"""
    from .conf_loader import _exec_with_placeholders
    had = "GCP_DATA_DIR" in os.environ
    os.environ.setdefault("GCP_DATA_DIR", "")               # the conf builds its data_save_dir from it; --out decides here
    try:
        ns = _exec_with_placeholders(path, "mod_hyper")
    finally:
        if not had:
            del os.environ["GCP_DATA_DIR"]
    if "config" not in ns:
        raise ValueError(f"{path}: a data-collection conf defines `config`")
    return NG.experiment_settings(_plain(dict(ns["config"])))


def parse_args(argv=None):
    p = argparse.ArgumentParser(prog="python -m video_gcp_amd.gen_nav", description=__doc__.split("\n\n")[1])
    p.add_argument("--experiment", default=None, help="a data-collection conf in the reference's format (mod_hyper.py)")
    p.add_argument("--n_rooms", type=int, default=None, choices=(9, 16, 25))
    p.add_argument("--n_traj", type=int, default=None)
    p.add_argument("--T", type=int, default=None)
    p.add_argument("--out", required=True)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--traj_per_file", type=int, default=None)
    p.add_argument("--crop_window", type=int, default=None)
    p.add_argument("--start_index", type=int, default=None)
    p.add_argument("--split", default="0.9,0.05,0.05", help="train,val,test fractions of the files (dataset_spec['split'])")
    p.add_argument("--plain", type=int, default=0, help="1: the reference's untextured picture (white rooms)")
    p.add_argument("--device", default="cuda:0")
    a = p.parse_args(argv)
    a.split = tuple(float(v) for v in a.split.split(","))
    if len(a.split) != 3 or sum(a.split) > 1.0 + 1e-9:
        p.error("--split: three fractions train,val,test that sum to at most 1")
    a.policy = {}
    s = dict(n_rooms=9, crop_window=40, T=100, start_index=0, end_index=None, traj_per_file=1)
    if a.experiment:
        e = read_experiment(a.experiment)
        a.policy = e.pop("policy")
        s.update(e)
    for k in ("n_rooms", "crop_window", "T", "start_index", "traj_per_file"):
        if getattr(a, k) is None:
            setattr(a, k, s[k])
    if a.n_traj is None:
        if s["end_index"] is None:
            p.error("--n_traj (or an --experiment with start_index / end_index) is required")
        a.n_traj = s["end_index"] - a.start_index + 1
    return a


def main(argv=None):
    a = parse_args(argv)
    res = NG.write_dataset(a.out, a.n_traj, n_rooms=a.n_rooms, T=a.T, seed=a.seed, traj_per_file=a.traj_per_file, crop_window=a.crop_window,
                           split=a.split, plain=bool(a.plain), start_index=a.start_index, device=a.device, **a.policy)
    ns = res["n_steps"].cpu().numpy()
    print(f"wrote {a.n_traj} trajectories ({a.n_rooms} rooms, T {a.T}) to {a.out}: plan lengths {ns.min()} .. {ns.max()}, "
          f"{int(res['redraws'].sum())} redrawn")
    return 0


if __name__ == "__main__":
    sys.exit(main())
