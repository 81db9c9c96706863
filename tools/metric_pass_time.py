"""Wall time of one batch of the top-of-N evaluation (`train.py --metric 1`, evaluation.Evaluator.eval) next to N headline forwards.

c2 tree model (B = 16, T = 80, 64x64), one seeded synthetic batch.  Per pruning scheme: Evaluator.eval inside val_mode (N prior-sampled
forwards, each aligned, scored and accumulated on the device, one device-to-host copy at the end), `--reps` times after one warm-up.
Next to it: N prior-sampled forwards alone, and N headline forwards (bench.py's workload: posterior forward with losses).
Prints one JSON line of milliseconds per batch.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2")
    ap.add_argument("--top_of", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--schemes", default="dtw,pruned_dtw,basic")
    a = ap.parse_args()
    import torch
    import video_gcp_amd as V
    from video_gcp_amd.evaluation import Evaluator
    from video_gcp_amd.model import GCPTreeModel
    from video_gcp_amd.synthetic import make_inputs_device
    hp = V.config(a.config)
    model = GCPTreeModel(hp, params=V.init_params(hp, seed=0), device="cuda:0")
    inputs = make_inputs_device(hp, 500000, "B", "cuda:0")
    N = a.top_of

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return min(ts), ts

    res = dict(config=a.config, batch=hp.batch_size, top_of=N)

    def headline():
        for _ in range(N):
            model.loss(inputs, model(inputs))

    def prior():
        with model.val_mode(pred_length=False):
            for _ in range(N):
                model(inputs, "train")

    res["headline_forwards_ms"] = timed(headline)[0]
    res["prior_forwards_ms"] = timed(prior)[0]
    for s in a.schemes.split(","):
        ev = Evaluator(model, pruning_scheme=s, top_of=N)

        def run():
            with model.val_mode(pred_length=False):
                ev.eval(inputs, None, model)
            ev.reset()
        best, all_ = timed(run)
        res[f"eval_{s}_ms"] = best
        res[f"eval_{s}_all_ms"] = [round(t, 1) for t in all_]
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
