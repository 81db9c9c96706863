"""Host-fed against device-fed training steps at c2 (video-gcp_amd/dataset.py).

Writes a seeded uint8 c2 dataset (B=16 sequences of up to 80 frames of 64x64x3 per batch) to a temporary directory, then times
ModelTrainer.train_epoch over `--batches` batches in three ways, alternating (`--rounds` times each) so that noise of the shared host
affects all alike:
  host     — HostFedLoader: uint8 frames from a 2-slot pinned ring, H2D on its own stream, gcpx_assemble_batch into the input buffers;
  device   — the same batches assembled in numpy beforehand and resident on the device, fed through the existing staging copy;
  resident — ResidentLoader (dataset_resident.py): the split uploaded once (load time and bytes are reported), per batch a slot of
             indices and pad masks and gcpx_assemble_batch_resident into the input buffers.
`--source_size N` (default 64: frames stored at the model's size) stores the frames at N x N; with N != 64 the host loop uploads them
at that size and resizes them in the assembly (gcpx_resize_assemble_batch, train.py --resize_frames 1), the resident loop keeps them at
that size on the device and resizes in its assembly, and the device-fed batches are resized by the numpy mirror beforehand.
Prints one JSON line: steps/s of each loop, per round, and their ratios.  For the kernel trace run it under
`rocprofv3 --kernel-trace --stats -- python tools/host_fed_loop.py --rounds 1`.
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--workers", type=int, default=4)
    ap.add_argument("--slots", type=int, default=2)
    ap.add_argument("--source_size", type=int, default=64, help="side the frames are stored at (64: no resize)")
    a = ap.parse_args()
    import torch
    import video_gcp_amd  # noqa: F401
    from video_gcp_amd import dataset as DS
    from video_gcp_amd import dataset_resident as DR
    from video_gcp_amd.train import ModelTrainer, get_cmd_args
    import dataset_fixture as FX

    with tempfile.TemporaryDirectory() as tmp:
        data, exp = os.path.join(tmp, "data"), os.path.join(tmp, "exp")
        B, T = 16, 80
        # 160 recorded sequences (about 190 MB at 64 x 64) read over and over: every batch is still read, packed and uploaded
        t0 = time.time()
        N = a.source_size
        FX.write_random_dataset(data, T=T, img=N, n_files=5, traj_per_file=32, phases=("train",), min_len=T)
        FX.write_random_dataset(data, T=T, img=N, n_files=1, traj_per_file=B, phases=("val",), min_len=T)
        t_write = time.time() - t0
        os.makedirs(exp)
        with open(os.path.join(exp, "conf.json"), "w") as f:
            json.dump({"config": "c2", "num_epochs": 1}, f)
        mt = ModelTrainer(get_cmd_args(["--path", exp, "--data_dir", data, "--log_outputs_interval", "1000000",
                                        "--resize_frames", str(int(N != 64))]))
        host = DS.HostFedLoader(mt.train_loader.ds, mt.model, B, n_repeat=-(-a.batches // 10), seed=0, n_slots=a.slots,
                                n_workers=a.workers)
        sched = host.schedule()[:a.batches]
        host.schedule = lambda: sched
        dev = [{k: torch.from_numpy(v).cuda() for k, v in DS.numpy_batch(host.ds, b, 0).items()} for b in sched]
        t0 = time.perf_counter()
        res = DR.ResidentLoader(host.ds, mt.model, B, n_repeat=host.n_repeat, seed=0, n_slots=a.slots)
        torch.cuda.synchronize()
        t_load = time.perf_counter() - t0
        res.schedule = lambda: sched

        def timed(loader):
            mt.train_loader = loader
            torch.cuda.synchronize()
            t = time.perf_counter()
            mt.train_epoch(0)
            torch.cuda.synchronize()
            return len(sched) / (time.perf_counter() - t)

        timed(host)                                     # warm-up: plans, graphs, the ring's allocation
        timed(dev)
        timed(res)
        rh, rd, rr = [], [], []
        for _ in range(a.rounds):
            rh.append(timed(host))
            rd.append(timed(dev))
            rr.append(timed(res))
        mh, md, mr = (sorted(r)[len(r) // 2] for r in (rh, rd, rr))
        extra = {"resident_steps_per_s": round(mr, 3), "resident_over_device": round(mr / md, 4), "resident_over_host": round(mr / mh, 4),
                 "rounds_resident": [round(x, 3) for x in rr], "store_bytes": int(res.store.nbytes),
                 "store_frames": int(res.store.n_frames_total), "store_load_s": round(t_load, 2),
                 "slot_bytes_per_batch": 8 * DR.N_INFO_RESIDENT * B + 4 * B * T}
        print(json.dumps({"workload": "host_fed_loop", "config": "c2", "batches": len(sched), "slots": a.slots, "workers": a.workers,
                          "source_size": N,
                          "host_fed_steps_per_s": round(mh, 3), "device_fed_steps_per_s": round(md, 3),
                          "host_over_device": round(mh / md, 4), "rounds_host": [round(x, 3) for x in rh],
                          "rounds_device": [round(x, 3) for x in rd], "dataset_write_s": round(t_write, 1), **extra}), flush=True)


if __name__ == "__main__":
    main()
