"""Time of the trajectory renderer at the nav datasets' real size: 25 rooms at scale 256 (S = 426), crop_window 40, 3 canvases, two layers
of 100 points (ground truth green, prediction red with dim_t): what one `regressed_state_topdown` panel costs on a logging step.

  device  gcpx_topdown_trajectories: device events around --calls back-to-back calls, microseconds per call, median and range over
          --rounds rounds after a warm-up round;
  host    visualization.render_trajectories_numpy, the numpy mirror, on host copies of the same layers (best of --host_reps).
The device canvases are compared with the mirror before anything is timed.  Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host_reps", type=int, default=3)
    a = ap.parse_args()
    import numpy as np
    import torch
    import video_gcp_amd  # noqa: F401
    from video_gcp_amd import dataset as DS
    from video_gcp_amd import image_log as IL
    from video_gcp_amd import runtime as rt
    from video_gcp_amd import visualization as V
    import topdown_fixture as TF

    n, P = 3, 100
    arrays = TF.make_assets(seed=6, n_rooms=25, scale=256, cw=40, k=11)
    assets = dict(background=arrays["background"], cw=40, n_rooms=25, scale=256, agent_stamp=arrays["agent_stamp"],
                  goal_stamp=arrays["goal_stamp"], agent_color=arrays["agent_color"], goal_color=arrays["goal_color"])
    assets["S"] = int(DS.topdown_table_size(25) * 256)
    dev = torch.device("cuda:0")
    lib = rt.load_library()
    rng = np.random.RandomState(6)
    walk = lambda: torch.from_numpy((rng.uniform(-22, 22, size=(n, 1, 2)) + np.cumsum(rng.randn(n, P, 2) * 0.6, axis=1)).astype(np.float32)).to(dev)
    length = torch.tensor([100, 57, 81], dtype=torch.int64, device=dev)
    dim_t = torch.from_numpy(rng.randint(0, 100, size=(n, 7)).astype(np.int32)).to(dev)
    layers = [dict(states=walk(), length=length, color=V.GREEN), dict(states=walk(), length=length, color=V.RED, dim_t=dim_t)]
    renderer = IL.TrajectoryRenderer(assets, dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    draw = lambda: renderer.render(lib, layers, n, stream, key="time")
    got = draw().cpu().numpy()
    host_layers = IL.numpy_layers(layers)
    host_ms = []
    for _ in range(a.host_reps):
        t0 = time.perf_counter()
        want = V.render_trajectories_numpy(assets, host_layers)
        host_ms.append((time.perf_counter() - t0) * 1e3)
    equal = bool(np.array_equal(got, want))

    def timed():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            draw()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.calls

    timed()
    us = [timed() for _ in range(a.rounds)]
    med = sorted(us)[len(us) // 2]
    print(json.dumps({"workload": "topdown_traj_time", "n": n, "S": assets["S"], "points": P, "layers": len(layers),
                      "canvas_bytes": int(got.nbytes), "equal_to_mirror": equal, "calls_per_round": a.calls,
                      "device_us_per_call": round(med, 2), "device_us_range": [round(min(us), 2), round(max(us), 2)],
                      "host_numpy_ms": round(min(host_ms), 2), "host_over_device": round(min(host_ms) * 1e3 / med, 1)}), flush=True)
    if not equal:
        sys.exit("the device canvases differ from the mirror")


if __name__ == "__main__":
    main()
