"""Time of the c5-shard adaptive training step (bench.py --full's "adaptive_train_step": configs[4], batch 8) at a given number of
attention heads and layers:  python tools/attention_layers_time.py <tree root> <heads> <layers>
<tree root>: the checkout whose package is measured ("." or an export of another commit built in place), so that two commits can be
run in alternation in one job (profiles/attention_layers.txt).  ROUNDS windows of STEPS steps, host clock around a device
synchronise, after WARM warm-up steps; one JSON line, with a checksum of the parameters after the last step (same seed and inputs
every time: two trees that compute the same print the same)."""
import hashlib
import json
import os
import sys
import time

root, heads, layers = os.path.abspath(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, "tests"))
import torch  # noqa: E402
import video_gcp_amd as V  # noqa: E402
from video_gcp_amd.model import GCPTreeModel  # noqa: E402
from video_gcp_amd.training import GCPTrainStep  # noqa: E402
from video_gcp_amd.synthetic import make_inputs  # noqa: E402

assert os.path.abspath(V.__file__).startswith(root), V.__file__
WARM, STEPS, ROUNDS = 5, 50, 5
dev = "cuda:0"
hp = V.config("c5", n_attention_heads=heads, n_attention_layers=layers)
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
    t0 = time.perf_counter()
    for _ in range(STEPS):
        out = tr.step(d, n)
    torch.cuda.synchronize()
    ms.append(round(1e3 * (time.perf_counter() - t0) / STEPS, 3))
loss = float(out.raw["losses"][5])
digest = hashlib.sha256(m.theta.cpu().numpy().tobytes()).hexdigest()[:16]
print(json.dumps(dict(tree=os.path.basename(root) or "this", heads=heads, layers=layers, ms_per_step=ms, median=sorted(ms)[len(ms) // 2],
                      loss=loss, theta_sha=digest, steps=WARM + STEPS * ROUNDS)), flush=True)
