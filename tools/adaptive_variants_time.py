"""Time of the c5 training step (configs[4] per GPU: B = 8, T = 200, 64 x 64, L = 8) in the four forms of the adaptive model:

    untied / dtw_image    (the baseline: what bench.py --full's "adaptive_train_step" runs)
    tied   / dtw_image    (untied_layers = False, the reference's default: one tree module, no side lanes in the backward)
    untied / dtw_latent   (matching cost between latents, adaptive.py:45-47; the criterion's image cost still runs)
    tied   / dtw_latent

    python tools/adaptive_variants_time.py [form ...]        form = untied:dtw_image etc.; default: all four, in that order

Each form in turn on one device: WARM warm-up steps, then ROUNDS windows of STEPS steps between two device events on the caller's
stream (the step's lanes are joined onto it).  One JSON line per form and a closing table against the baseline
(profiles/adaptive_tied_latent.txt)."""
import gc
import json
import os
import sys

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
import torch  # noqa: E402
import video_gcp_amd as V  # noqa: E402
from video_gcp_amd.model import GCPTreeModel  # noqa: E402
from video_gcp_amd.training import GCPTrainStep  # noqa: E402
from video_gcp_amd.synthetic import make_inputs  # noqa: E402

WARM, STEPS, ROUNDS = 5, 20, 5
FORMS = sys.argv[1:] or ["untied:dtw_image", "tied:dtw_image", "untied:dtw_latent", "tied:dtw_latent"]
dev = "cuda:0"


def measure(form):
    levels, matching = form.split(":")
    hp = V.config("c5", untied_layers=(levels == "untied"), matching_type=matching)
    m = GCPTreeModel(hp, params=V.init_params(hp, seed=0), device=dev)
    inputs, noise, _ = make_inputs(hp, seed=200, variant="A")
    d = {k: v.to(dev) for k, v in inputs.items()}
    n = noise.to(dev)
    tr = GCPTrainStep(m)
    for _ in range(WARM):
        out = tr.step(d, n)
    torch.cuda.synchronize()
    ms = []
    for _ in range(ROUNDS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(STEPS):
            out = tr.step(d, n)
        e1.record()
        e1.synchronize()
        ms.append(round(e0.elapsed_time(e1) / STEPS, 3))
    fns = [getattr(op[1], "__name__", "") for op in tr.last_bplan.ops]
    res = dict(form=form, ms_per_step=ms, median=sorted(ms)[len(ms) // 2], loss=float(out.raw["losses"][5]),
               side_lanes=bool(tr.side_lanes), backward_launches=sum(1 for f in fns if f),
               parameters=int(m.theta.numel()), steps=WARM + STEPS * ROUNDS)
    print(json.dumps(res), flush=True)
    del tr, m, d, n, out
    gc.collect()
    torch.cuda.empty_cache()
    return res


rows = [measure(f) for f in FORMS]
base = rows[0]["median"]
print(f"\n{'form':<20}{'ms / step (median of ' + str(ROUNDS) + ' x ' + str(STEPS) + ')':>34}{'vs ' + rows[0]['form']:>24}{'side lanes':>12}")
for r in rows:
    print(f"{r['form']:<20}{r['median']:>34.3f}{r['median'] / base:>24.3f}{str(r['side_lanes']):>12}")
