"""What gradient accumulation (GCPTrainStep(accumulate=k), train.py --accumulate_steps k) costs per micro-batch, at c2, synthetic inputs.

(a) steps     three trainers of the tree model -- k = 1 (the step as it always was), 2 and 8 -- live in one process and are taken in
              turn, one whole cycle (k micro-steps, one optimizer step) each between two device events on the caller's stream:
              --steps cycles each after --warmup.  Reported: ms per micro-batch (cycle / k), median, quartiles, minimum; and the cycle
              against k plain steps.
(b) kernel    gcpx_grad_accumulate alone over a vector of the model's gradient size, add and assign: --blocks blocks of --calls
              calls between two device events after a warm-up block; 12 n (8 n) bytes against the 6.0 TB/s of an in-order sweep of HBM
              (MI355X_MICROARCH.md).
(c) profile   for a run under `rocprofv3 --kernel-trace --stats` (a run of its own): --calls calls of the kernel each way, then
              --profile-steps plain steps (k = 1) of a fresh trainer after 3 of warm-up.  With --root <another checkout> the package is
              imported from there and the kernel calls are left out when it has no such entry point: the total number of kernel
              dispatches of the two runs, less the kernel calls, is the launch count of `trainer.step` at k = 1 on the two commits
              (tools/kstats.py reads the trace).
Writes --out (default profiles/accumulate_step.txt; appends with --append) and prints the same lines.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWEEP_RATE = 6.0e12          # bytes / s: read sweep of HBM3E on the MI355X
KS = (1, 2, 8)


def quartiles(v):
    q = statistics.quantiles(v, n=4)
    return dict(median=round(statistics.median(v), 4), q1=round(q[0], 4), q3=round(q[2], 4), min=round(min(v), 4), max=round(max(v), 4))


def _trainer(a, k):
    import video_gcp_amd as V
    from video_gcp_amd.model import GCPTreeModel
    from video_gcp_amd.training import GCPTrainStep
    hp = V.config(a.config)
    kw = dict(accumulate=k) if k > 1 else {}
    return hp, GCPTrainStep(GCPTreeModel(hp, params=V.init_params(hp, seed=0), device="cuda:0"), lr=1e-3, **kw)


def steps(a, emit):
    import torch
    from video_gcp_amd.synthetic import make_inputs_device
    trainers = {}
    for k in KS:
        hp, trainers[k] = _trainer(a, k)
    batches = [make_inputs_device(hp, 1000 + i, "B", "cuda:0") for i in range(8)]
    stream = torch.cuda.current_stream()
    ms = {k: [] for k in KS}
    for i in range(a.warmup + a.steps):
        for k in KS:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record(stream)
            for j in range(k):
                trainers[k].step(batches[(i * k + j) % len(batches)])
            e1.record(stream)
            torch.cuda.synchronize()
            assert trainers[k].stepped
            if i >= a.warmup:
                ms[k].append(e0.elapsed_time(e1) / k)
    base = statistics.median(ms[1])
    for k in KS:
        med = statistics.median(ms[k])
        emit(json.dumps(dict(part="steps", config=a.config, k=k, cycles=a.steps, warmup=a.warmup, ms_per_micro_batch=quartiles(ms[k]),
                             cycle_ms=round(k * med, 4), k_plain_steps_ms=round(k * base, 4), cycle_minus_k_steps_ms=round(k * (med - base), 4),
                             opt_steps=float(trainers[k].opt_state[0]))))
    trainers.clear()
    torch.cuda.empty_cache()


def _kernel_calls(lib, n, calls, stream):
    import torch
    from video_gcp_amd import runtime as rt
    g = torch.Generator(device="cuda:0").manual_seed(0)
    dst, src = torch.randn(n, generator=g, device="cuda:0"), torch.randn(n, generator=g, device="cuda:0")

    def call(assign):
        for _ in range(calls):
            rt.check(lib.gcpx_grad_accumulate(dst.data_ptr(), src.data_ptr(), n, assign, 0, stream.cuda_stream), "grad_accumulate")
    return call


def kernel(a, emit):
    import torch
    import video_gcp_amd as V
    from video_gcp_amd import runtime as rt
    from video_gcp_amd.params import init_params
    lib = rt.load_library()
    n = a.n or sum((v.numel() + 3) // 4 * 4 for v in init_params(V.config(a.config), seed=0).values())
    stream = torch.cuda.current_stream()
    call = _kernel_calls(lib, n, a.calls, stream)
    for assign in (0, 1):
        us = []
        for block in range(a.blocks + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record(stream)
            call(assign)
            e1.record(stream)
            torch.cuda.synchronize()
            if block:                                                # block 0 warms up
                us.append(e0.elapsed_time(e1) * 1e3 / a.calls)
        n_bytes = (8 if assign else 12) * n
        med = statistics.median(us)
        emit(json.dumps(dict(part="kernel", call="gcpx_grad_accumulate", assign=assign, n=n, bytes=n_bytes,
                             floor_us=round(n_bytes / SWEEP_RATE * 1e6, 1), us_per_call=quartiles(us), GBps=round(n_bytes / med / 1e3, 1),
                             share_of_sweep=round(n_bytes / (med * 1e-6) / SWEEP_RATE, 3), calls_per_block=a.calls, blocks=a.blocks)))


def profile(a, emit):
    import torch
    from video_gcp_amd import runtime as rt
    from video_gcp_amd.synthetic import make_inputs_device
    lib = rt.load_library()
    hp, tr = _trainer(a, 1)
    stream = torch.cuda.current_stream()
    has_kernel = any(s[0] == "gcpx_grad_accumulate" for s in rt.SYMBOLS)
    kernel_calls = 0
    if has_kernel:
        call = _kernel_calls(lib, tr.grad.numel(), a.calls, stream)
        call(0)
        call(1)
        kernel_calls = 2 * a.calls
    batches = [make_inputs_device(hp, 1000 + i, "B", "cuda:0") for i in range(4)]
    for i in range(3 + a.profile_steps):
        tr.step(batches[i % len(batches)])
    torch.cuda.synchronize()
    emit(json.dumps(dict(part="profile", root=os.path.relpath(a.root, ROOT), n=tr.grad.numel(), accumulate_kernel_calls=kernel_calls, plain_steps=3 + a.profile_steps,
                         opt_steps=float(tr.opt_state[0]))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2")
    ap.add_argument("--parts", default="steps,kernel")
    ap.add_argument("--steps", type=int, default=50, help="cycles (optimizer steps) timed per trainer")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--n", type=int, default=0, help="kernel part: vector length (default: the model's flat gradient)")
    ap.add_argument("--profile-steps", type=int, default=10)
    ap.add_argument("--root", default=ROOT, help="checkout the package is imported from (profile part: another commit)")
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "accumulate_step.txt"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    lines = []

    def emit(line):
        print(line, flush=True)
        lines.append(line)
    emit("# tools/accumulate_time.py " + " ".join(sys.argv[1:]))
    parts = a.parts.split(",")
    if "steps" in parts:
        steps(a, emit)
    if "kernel" in parts:
        kernel(a, emit)
    if "profile" in parts:
        profile(a, emit)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a" if a.append else "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
