"""What `train.py --log_scalars 1` costs (scalar_log.py, csrc/train_stats.hip).

--mode kernels   per configuration (--configs c2,c5): one training step, then --reps calls each of GCPTrainStep.gradient_stats()
                 (gcpx_grad_segment_norms: chunk_sqsum_kernel + segment_norm_kernel) and scalar_log.kl_layerwise (gcpx_kl_layerwise:
                 kl_node_mean_kernel + kl_level_mean_kernel).  Prints the wall time of a call (launch to sync, best of --reps), the
                 bytes the sweep reads and the floor they give at 6.0 TB/s.  Run it under `rocprofv3 --kernel-trace --stats -- python
                 tools/scalar_log_time.py --mode kernels`, in a run of its own, for the time of each kernel, i.e. of each stage.
--mode epoch     c2, ModelTrainer.train_epoch over --batches batches at --log_outputs_interval 10, the logger switched off and on in
                 turn in ONE process (off, on, off, on, ...; --rounds pairs after one warm-up epoch): the spread of the off runs is what
                 a difference has to exceed.
Prints one JSON line per configuration / epoch.
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SWEEP_RATE = 6.0e12          # bytes / s: read sweep of HBM3E on the MI355X


def kernels(a):
    import torch
    import video_gcp_amd as V
    from video_gcp_amd import scalar_log as SL
    from video_gcp_amd.model import GCPTreeModel
    from video_gcp_amd.synthetic import make_inputs_device
    from video_gcp_amd.training import GCPTrainStep

    def timed(fn):
        ts = []
        for _ in range(a.reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e6)
        return round(min(ts[1:]), 1)

    for name in a.configs.split(","):
        hp = V.config(name)
        model = GCPTreeModel(hp, params=V.init_params(hp, seed=0), device="cuda:0")
        trainer = GCPTrainStep(model, lr=1e-3)
        inputs = make_inputs_device(hp, 1000, "B", "cuda:0")
        out = trainer.step(inputs)
        torch.cuda.synchronize()
        st = trainer.gradient_stats()
        gs = trainer._grad_stats
        counted_bytes = 4 * sum(int(torch.tensor(model._poff[k][1]).prod()) for k in gs.names)
        B, L, nv = hp.batch_size, hp.hierarchy_levels, hp.nz_vae
        kl_bytes = 4 * B * (2 ** L - 1) * 4 * nv
        res = dict(config=name, batch=B, levels=L, nz_vae=nv, grad_floats=trainer.grad.numel(), segments=gs.n_seg, chunks=gs.n_chunks,
                   grad_bytes=counted_bytes, grad_floor_us=round(counted_bytes / SWEEP_RATE * 1e6, 1),
                   kl_bytes=kl_bytes, kl_floor_us=round(kl_bytes / SWEEP_RATE * 1e6, 2))
        res["gradient_stats_call_us"] = timed(trainer.gradient_stats)
        res["kl_layerwise_call_us"] = timed(lambda: SL.kl_layerwise(model, out))
        res["stats"] = [float(v) for v in st.stats.tolist()]
        res["kl_levels"] = [round(float(v), 6) for v in SL.kl_layerwise(model, out).tolist()]
        print(json.dumps(res), flush=True)
        del model, trainer
        torch.cuda.empty_cache()


def epoch(a):
    import torch
    from video_gcp_amd.scalar_log import ScalarLogger
    from video_gcp_amd.train import ModelTrainer, get_cmd_args
    exp = tempfile.mkdtemp()
    with open(os.path.join(exp, "conf.json"), "w") as f:
        json.dump({"config": "c2"}, f)
    tr = ModelTrainer(get_cmd_args(["--path", exp, "--batches_per_epoch", str(a.batches), "--log_outputs_interval", "10",
                                    "--log_scalars", "1"]))
    logger = tr.scalar_log

    def run(on, ep):
        tr.scalar_log = tr.model.scalar_log = logger if on else None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tr.train_epoch(ep)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    run(False, 0)                                               # warm-up: plans, graphs, allocator
    run(True, 0)
    for r in range(a.rounds):
        for on in (False, True):
            ms = run(on, r + 1)
            print(json.dumps(dict(config="c2", log_scalars=int(on), round=r, batches=a.batches, epoch_ms=round(ms, 2),
                                  ms_per_batch=round(ms / a.batches, 4))), flush=True)
    ms = run(False, a.rounds + 1)                               # one more off run: the spread
    print(json.dumps(dict(config="c2", log_scalars=0, round=a.rounds, batches=a.batches, epoch_ms=round(ms, 2),
                          ms_per_batch=round(ms / a.batches, 4))), flush=True)
    logger.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("kernels", "epoch"), default="kernels")
    ap.add_argument("--configs", default="c2,c5")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batches", type=int, default=60)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    (kernels if a.mode == "kernels" else epoch)(a)


if __name__ == "__main__":
    main()
