"""What the training guard costs (video_gcp_amd/health.py, csrc/train_stats.hip, `--nan_guard`), at c2.

(a) kernels   gcpx_grad_health (chunk_health_kernel + segment_health_kernel) and gcpx_grad_segment_norms (chunk_sqsum_kernel +
              segment_norm_kernel) over the SAME gradient vector and tables, in one process, in alternating blocks of --calls calls
              between two device events (--blocks blocks each after a warm-up block).  Bytes = the floats the tables name; the rate is
              set against the 6.0 TB/s of an in-order read sweep of HBM (MI355X_MICROARCH.md).  The norms kernel is the yardstick: the
              health kernel reads the same bytes and does less arithmetic.
(b) step      the training step with the guard off, "raise" and "skip": three trainers over one model's configuration in one process,
              taken in turn step by step (off, raise, skip, off, ...), --steps steps each after --warmup, each step between a
              synchronise and the synchronise behind it.  Median, quartiles, minimum.
Writes --out (default profiles/r12_nan_guard.txt) and prints the same lines.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SWEEP_RATE = 6.0e12          # bytes / s: read sweep of HBM3E on the MI355X


def quartiles(v):
    q = statistics.quantiles(v, n=4)
    return dict(median=round(statistics.median(v), 4), q1=round(q[0], 4), q3=round(q[2], 4), min=round(min(v), 4), max=round(max(v), 4))


def kernels(a, emit):
    import torch
    import video_gcp_amd as V
    from video_gcp_amd.model import GCPTreeModel
    from video_gcp_amd.synthetic import make_inputs_device
    from video_gcp_amd.training import GCPTrainStep
    hp = V.config(a.config)
    model = GCPTreeModel(hp, params=V.init_params(hp, seed=0), device="cuda:0")
    tr = GCPTrainStep(model, lr=1e-3, nan_guard="skip")
    out = tr.step(make_inputs_device(hp, 1000, "B", "cuda:0"))
    torch.cuda.synchronize()
    tr.gradient_stats()
    h, gs = tr._grad_health(), tr._grad_stats
    assert h.names == gs.names and h.n_chunks == gs.n_chunks
    n_bytes = 4 * sum(int(torch.tensor(model._poff[k][1]).prod()) for k in h.names)
    stream = torch.cuda.current_stream()
    extra = out.raw["losses"]
    calls = {"grad_health": lambda: h.launch(model.lib, tr.grad, extra, tr.opt_state.data_ptr() + 12, stream.cuda_stream),
             "grad_segment_norms": lambda: gs.launch(model.lib, tr.grad, 1.0, tr.opt_state.data_ptr() + 4, stream.cuda_stream)}
    per_call = {k: [] for k in calls}
    for block in range(a.blocks + 1):
        for name, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record(stream)
            for _ in range(a.calls):
                fn()
            e1.record(stream)
            torch.cuda.synchronize()
            if block:                                            # block 0 warms up
                per_call[name].append(e0.elapsed_time(e1) * 1e3 / a.calls)
    emit(json.dumps(dict(part="kernels", config=a.config, grad_floats=tr.grad.numel(), segments=h.n_seg, chunks=h.n_chunks,
                         bytes=n_bytes, floor_us=round(n_bytes / SWEEP_RATE * 1e6, 1), calls_per_block=a.calls, blocks=a.blocks)))
    for name, v in per_call.items():
        us = statistics.median(v)
        emit(json.dumps(dict(part="kernels", call=name, us_per_call=quartiles(v), GBps=round(n_bytes / us / 1e3, 1),
                             share_of_sweep=round(n_bytes / (us * 1e-6) / SWEEP_RATE, 3))))
    assert tr.health().summary[:7].tolist() == [0, 0, 0, 0, -1, 0, 0], "the timed gradient was not finite"
    del model, tr
    torch.cuda.empty_cache()


def steps(a, emit):
    import torch
    import video_gcp_amd as V
    from video_gcp_amd.model import GCPTreeModel
    from video_gcp_amd.synthetic import make_inputs_device
    from video_gcp_amd.training import GCPTrainStep
    hp = V.config(a.config)
    modes = ("off", "raise", "skip")
    trainers = {}
    for g in modes:
        model = GCPTreeModel(hp, params=V.init_params(hp, seed=0), device="cuda:0")
        trainers[g] = GCPTrainStep(model, lr=1e-3, **({} if g == "off" else {"nan_guard": g}))
    batches = [make_inputs_device(hp, 1000 + i, "B", "cuda:0") for i in range(4)]
    ms = {g: [] for g in modes}
    for i in range(a.warmup + a.steps):
        for g in modes:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            trainers[g].step(batches[i % len(batches)])
            torch.cuda.synchronize()
            if i >= a.warmup:
                ms[g].append((time.perf_counter() - t0) * 1e3)
    for g in modes:
        emit(json.dumps(dict(part="step", config=a.config, nan_guard=g, steps=a.steps, warmup=a.warmup, ms_per_step=quartiles(ms[g]),
                             opt_steps=float(trainers[g].opt_state[0]))))
    off = statistics.median(ms["off"])
    emit(json.dumps(dict(part="step", median_over_off_ms={g: round(statistics.median(ms[g]) - off, 4) for g in modes[1:]})))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2")
    ap.add_argument("--parts", default="kernels,step")
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_nan_guard.txt"))
    a = ap.parse_args()
    lines = []

    def emit(line):
        print(line, flush=True)
        lines.append(line)
    emit("# tools/nan_guard_time.py " + " ".join(sys.argv[1:]))
    if "kernels" in a.parts:
        kernels(a, emit)
    if "step" in a.parts:
        steps(a, emit)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
