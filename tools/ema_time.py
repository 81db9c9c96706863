"""What the weight average (GCPTrainStep(ema_decay=...), train.py --ema_decay) costs, at c2, synthetic inputs.

(a) kernel    gcpx_ema_update against gcpx_grad_accumulate (add form) over a vector of the model's flat size: both move 12 n bytes.  The
              two are taken in alternating blocks of --calls calls between two device events, --blocks blocks each after one warm-up
              block each; GB/s against the 6.0 TB/s of an in-order sweep of HBM (MI355X_MICROARCH.md).  Reported as well: whether the
              new kernel's median lies inside the accumulate kernel's q1 .. q3 of this run, and by how much it misses if not.  Both
              write the same destination buffer; --exchange times the pair on a second destination as well.
(b) steps     two trainers of the tree model in one process, ema off / on, taken in turn: one step each between two device events on
              the caller's stream, --steps steps after --warmup; median and quartiles, and the difference of the medians.  Then the time
              of one `with trainer.ema_weights(): pass` -- two swaps and two full re-packs, paid per validation, not per step.
Writes --out (default profiles/ema_step.txt; appends with --append) and prints the same lines.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWEEP_RATE = 6.0e12          # bytes / s: read sweep of HBM3E on the MI355X


def quartiles(v):
    q = statistics.quantiles(v, n=4)
    return dict(median=round(statistics.median(v), 4), q1=round(q[0], 4), q3=round(q[2], 4), min=round(min(v), 4), max=round(max(v), 4))


def kernel(a, emit):
    import torch
    import video_gcp_amd as V
    from video_gcp_amd import runtime as rt
    from video_gcp_amd.params import init_params
    lib = rt.load_library()
    n = a.n or sum((v.numel() + 3) // 4 * 4 for v in init_params(V.config(a.config), seed=0).values())
    stream = torch.cuda.current_stream()
    g = torch.Generator(device="cuda:0").manual_seed(0)
    dst, src = torch.randn(n, generator=g, device="cuda:0"), torch.randn(n, generator=g, device="cuda:0")
    dst2, src0 = dst.clone(), dst.clone()

    def ema(d=dst):
        rt.check(lib.gcpx_ema_update(d.data_ptr(), src.data_ptr(), n, a.decay, None, 0, stream.cuda_stream), "ema_update")

    def acc(d=dst):
        rt.check(lib.gcpx_grad_accumulate(d.data_ptr(), src.data_ptr(), n, 0, 0, stream.cuda_stream), "grad_accumulate")
    # both kernels on the SAME destination: where a 293 MB buffer lies moves either kernel by ~2 % (--exchange shows it: the pair again
    # on a second destination), more than the two differ
    calls = {"gcpx_ema_update": ema, "gcpx_grad_accumulate": acc}
    if a.exchange:
        calls.update({"gcpx_ema_update@second_buffer": lambda: ema(dst2), "gcpx_grad_accumulate@second_buffer": lambda: acc(dst2)})
    us = {k: [] for k in calls}
    for block in range(a.blocks + 1):
        for name, call in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record(stream)
            for _ in range(a.calls):
                call()
            e1.record(stream)
            torch.cuda.synchronize()
            if block:                                                # block 0 warms up
                us[name].append(e0.elapsed_time(e1) * 1e3 / a.calls)
        dst.copy_(src0)                                              # (200 additions of src per block: keep the values where they began)
        dst2.copy_(src0)
    n_bytes = 12 * n
    q = {k: quartiles(v) for k, v in us.items()}
    for name in calls:
        med = q[name]["median"]
        emit(json.dumps(dict(part="kernel", call=name, n=n, bytes=n_bytes, floor_us=round(n_bytes / SWEEP_RATE * 1e6, 1), us_per_call=q[name],
                             GBps=round(n_bytes / med / 1e3, 1), share_of_sweep=round(n_bytes / (med * 1e-6) / SWEEP_RATE, 3),
                             calls_per_block=a.calls, blocks=a.blocks)))
    med, lo, hi = q["gcpx_ema_update"]["median"], q["gcpx_grad_accumulate"]["q1"], q["gcpx_grad_accumulate"]["q3"]
    emit(json.dumps(dict(part="kernel", compare="ema median against accumulate q1..q3", ema_median_us=med, accumulate_q1_us=lo,
                         accumulate_q3_us=hi, inside=bool(lo <= med <= hi),
                         outside_by_us=round(0.0 if lo <= med <= hi else (med - hi if med > hi else med - lo), 4))))


def steps(a, emit):
    import torch
    import video_gcp_amd as V
    from video_gcp_amd.model import GCPTreeModel
    from video_gcp_amd.synthetic import make_inputs_device
    from video_gcp_amd.training import GCPTrainStep
    hp = V.config(a.config)
    trainers = {}
    for name, kw in (("off", {}), ("on", dict(ema_decay=a.decay))):
        trainers[name] = GCPTrainStep(GCPTreeModel(hp, params=V.init_params(hp, seed=0), device="cuda:0"), lr=1e-3, **kw)
    batches = [make_inputs_device(hp, 1000 + i, "B", "cuda:0") for i in range(8)]
    stream = torch.cuda.current_stream()
    ms = {k: [] for k in trainers}
    for i in range(a.warmup + a.steps):
        for name, tr in trainers.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record(stream)
            tr.step(batches[i % len(batches)])
            e1.record(stream)
            torch.cuda.synchronize()
            if i >= a.warmup:
                ms[name].append(e0.elapsed_time(e1))
    off, on = statistics.median(ms["off"]), statistics.median(ms["on"])
    for name in trainers:
        emit(json.dumps(dict(part="steps", config=a.config, ema=name, steps=a.steps, warmup=a.warmup, ms_per_step=quartiles(ms[name]))))
    emit(json.dumps(dict(part="steps", config=a.config, on_minus_off_ms=round(on - off, 4), share_of_step=round((on - off) / off, 4),
                         ema_updates=trainers["on"].ema_updates)))
    tr = trainers["on"]
    swaps = []
    for i in range(1 + a.swaps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(stream)
        with tr.ema_weights():
            pass
        e1.record(stream)
        torch.cuda.synchronize()
        if i:
            swaps.append(e0.elapsed_time(e1))
    emit(json.dumps(dict(part="ema_weights", config=a.config, n=tr.ema.numel(), enter_plus_exit_ms=quartiles(swaps), rounds=a.swaps)))
    trainers.clear()
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2")
    ap.add_argument("--parts", default="kernel,steps")
    ap.add_argument("--decay", type=float, default=0.999)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--swaps", type=int, default=10, help="ema_weights() enter + exit rounds timed after one of warm-up")
    ap.add_argument("--exchange", action="store_true", help="kernel part: also time each kernel on the other one's destination buffer")
    ap.add_argument("--n", type=int, default=0, help="kernel part: vector length (default: the model's flat vector)")
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ema_step.txt"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    lines = []

    def emit(line):
        print(line, flush=True)
        lines.append(line)
    emit("# tools/ema_time.py " + " ".join(sys.argv[1:]))
    parts = a.parts.split(",")
    if "kernel" in parts:
        kernel(a, emit)
    if "steps" in parts:
        steps(a, emit)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a" if a.append else "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
