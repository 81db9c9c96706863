"""What a training step costs with the gaussian decoder head next to the mixture head, on the same commit, at c2.

(a) kernel    gcpx_gauss_nll_bwd alone at the c2 training shape (rows = B T = 1280 frames of 64 x 64, C = 3, pitch 16): --blocks blocks of
              --calls calls between two device events after a warm-up block.  Bytes = the two NCHW reads and the gradient rows written;
              the rate is set against the 6.0 TB/s of an in-order sweep of HBM (MI355X_MICROARCH.md).
(b) step      the training step (forward + losses + backward + RAdam) of the tree model, and of the flat model at the shape bench.py
              times it (c2, default widths), each with decoder_distribution = "gaussian" and "discrete_logistic_mixture": the two
              trainers of a model live in one process and are taken in turn step by step (gaussian, dlm, gaussian, ...), --steps steps
              each after --warmup, every step between two device events on the caller's stream.  Median, quartiles, minimum.
Writes --out (default profiles/gauss_train_step.txt) and prints the same lines.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SWEEP_RATE = 6.0e12          # bytes / s: read sweep of HBM3E on the MI355X
HEADS = ("gaussian", "discrete_logistic_mixture")


def quartiles(v):
    q = statistics.quantiles(v, n=4)
    return dict(median=round(statistics.median(v), 4), q1=round(q[0], 4), q3=round(q[2], 4), min=round(min(v), 4), max=round(max(v), 4))


def kernel(a, emit):
    import torch
    import video_gcp_amd as V
    from video_gcp_amd import runtime as rt
    hp = V.config(a.config)
    lib = rt.load_library()
    rows, C, npix, pitch = hp.batch_size * hp.max_seq_len, hp.input_nc, hp.img_sz * hp.img_sz, 16
    g = torch.Generator(device="cuda:0").manual_seed(0)
    mu = torch.tanh(torch.randn(rows, C, npix, generator=g, device="cuda:0"))
    x = torch.rand(rows, C, npix, generator=g, device="cuda:0") * 2 - 1
    w = (torch.rand(rows, generator=g, device="cuda:0") > 0.15).float()            # padded frames weigh 0, as in a ragged batch
    ls = torch.full((1,), -0.7, device="cuda:0")
    dy, colsum = torch.empty(rows, npix, pitch, device="cuda:0"), torch.empty(rows, pitch, device="cuda:0")
    nll, dls = torch.empty(rows, device="cuda:0"), torch.empty(rows, device="cuda:0")
    stream = torch.cuda.current_stream()
    scale = hp.dense_img_rec_weight / (hp.batch_size * float(hp.max_seq_len * C * npix))

    def call():
        rt.check(lib.gcpx_gauss_nll_bwd(mu.data_ptr(), x.data_ptr(), w.data_ptr(), ls.data_ptr(), scale, dy.data_ptr(), colsum.data_ptr(),
                                        nll.data_ptr(), dls.data_ptr(), rows, C, npix, pitch, stream.cuda_stream), "gauss_nll_bwd")
    us = []
    for block in range(a.blocks + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(stream)
        for _ in range(a.calls):
            call()
        e1.record(stream)
        torch.cuda.synchronize()
        if block:                                                # block 0 warms up
            us.append(e0.elapsed_time(e1) * 1e3 / a.calls)
    n_bytes = 4 * (2 * mu.numel() + dy.numel())
    med = statistics.median(us)
    emit(json.dumps(dict(part="kernel", call="gcpx_gauss_nll_bwd", rows=rows, C=C, npix=npix, pitch=pitch, bytes=n_bytes,
                         floor_us=round(n_bytes / SWEEP_RATE * 1e6, 1), us_per_call=quartiles(us), GBps=round(n_bytes / med / 1e3, 1),
                         share_of_sweep=round(n_bytes / (med * 1e-6) / SWEEP_RATE, 3), calls_per_block=a.calls, blocks=a.blocks)))


def steps(a, emit, which):
    import torch
    import video_gcp_amd as V
    from video_gcp_amd.synthetic import make_inputs_device
    trainers = {}
    for head in HEADS:
        hp = V.config(a.config, decoder_distribution=head)
        if which == "tree":
            from video_gcp_amd.model import GCPTreeModel
            from video_gcp_amd.training import GCPTrainStep
            trainers[head] = GCPTrainStep(GCPTreeModel(hp, params=V.init_params(hp, seed=0), device="cuda:0"), lr=1e-3)
        else:
            from video_gcp_amd.sequential import GCPSequentialModel
            from video_gcp_amd.training_sequential import SequentialTrainStep
            trainers[head] = SequentialTrainStep(GCPSequentialModel(hp, device="cuda:0"), lr=1e-3)
    batches = [make_inputs_device(hp, 1000 + i, "B", "cuda:0") for i in range(4)]
    stream = torch.cuda.current_stream()
    ms = {h: [] for h in HEADS}
    for i in range(a.warmup + a.steps):
        for head in HEADS:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record(stream)
            trainers[head].step(batches[i % len(batches)])
            e1.record(stream)
            torch.cuda.synchronize()
            if i >= a.warmup:
                ms[head].append(e0.elapsed_time(e1))
    for head in HEADS:
        emit(json.dumps(dict(part="step", model=which, config=a.config, head=head, steps=a.steps, warmup=a.warmup,
                             ms_per_step=quartiles(ms[head]), opt_steps=float(trainers[head].opt_state[0]))))
    emit(json.dumps(dict(part="step", model=which, gaussian_minus_dlm_ms=round(statistics.median(ms[HEADS[0]]) - statistics.median(ms[HEADS[1]]), 4))))
    trainers.clear()
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2")
    ap.add_argument("--parts", default="kernel,tree,flat")
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gauss_train_step.txt"))
    a = ap.parse_args()
    lines = []

    def emit(line):
        print(line, flush=True)
        lines.append(line)
    emit("# tools/gauss_train_time.py " + " ".join(sys.argv[1:]))
    parts = a.parts.split(",")
    if "kernel" in parts:
        kernel(a, emit)
    for which in ("tree", "flat"):
        if which in parts:
            steps(a, emit, which)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
