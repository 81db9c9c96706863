"""Wall time of one picture-logging step (`train.py --log_images 1`, image_log.log_outputs) next to a plain training step.

Per configuration (c2: balanced tree; c5: adaptive binding + attentive inference), one seeded synthetic batch, after a training step:
  device   every panel composed by gcpx_panel_compose into its cached uint8 canvas + the canvas copied to the host (what a logging
           step adds in front of the file encoding), and the launches alone;
  host     the same panels by the numpy restatement (visualization.compose + to_uint8) after copying their f32 sources to the host --
           the reference's way (visualization.py, logger.py), with the copy timed apart;
  files    PNG / APNG encoding and writing of the canvases (zlib, host only; the same for either path);
  step     a plain training step, for scale.
Prints one JSON line of milliseconds per configuration: best of --reps after one warm-up; the host path and the files, which take
seconds at c5 (its match_overview is 3 x 13312 x 16448 pixels), are run --host_reps times without a warm-up.
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c2,c5")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host_reps", type=int, default=1)
    a = ap.parse_args()
    import torch
    import video_gcp_amd as V
    from video_gcp_amd import image_log as IL
    from video_gcp_amd import visualization as VIS
    from video_gcp_amd.model import GCPTreeModel
    from video_gcp_amd.synthetic import make_inputs_device
    from video_gcp_amd.training import GCPTrainStep

    def timed(fn, reps=None):
        if reps is None:
            fn()
            torch.cuda.synchronize()
        ts = []
        for _ in range(reps or a.reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return round(min(ts), 3)

    for name in a.configs.split(","):
        hp = V.config(name)
        model = GCPTreeModel(hp, params=V.init_params(hp, seed=0), device="cuda:0")
        trainer = GCPTrainStep(model, lr=1e-3)
        inputs = make_inputs_device(hp, 1000, "B", "cuda:0")
        res = dict(config=name, batch=hp.batch_size, T=hp.max_seq_len, levels=hp.hierarchy_levels, img_sz=hp.img_sz)
        res["train_step_ms"] = timed(lambda: trainer.step(inputs))
        out = trainer.step(inputs)
        torch.cuda.synchronize()
        stream = torch.cuda.current_stream(model.device).cuda_stream
        panels = [(IL.DevicePanel(build(), model.device), tensors) for _, build, tensors, _ in IL.tree_panels(model, out, inputs, "train")]
        res["panels"] = {dp.panel.name: [dp.panel.n, dp.panel.H, dp.panel.W, len(dp.panel.tiles)] for dp, _ in panels}
        res["canvas_bytes"] = sum(dp.canvas.numel() for dp, _ in panels)

        def launches():
            IL.tree_panels(model, out, inputs, "train")              # (the soft estimates' launch of an adaptive model is part of it)
            for dp, tensors in panels:
                dp.compose(model.lib, tensors, stream)

        def device():
            launches()
            return [dp.canvas.cpu().numpy() for dp, _ in panels]

        def copy_sources():
            return [IL.numpy_sources({k: tensors[k] for k in dp.panel.sources}) for dp, tensors in panels]

        host_src = copy_sources()
        host_out = []

        def host_compose():                                          # one panel at a time: a c5 canvas is 7.9 GB as f32
            host_out.clear()
            for (dp, _), src in zip(panels, host_src):
                host_out.append(VIS.to_uint8(VIS.compose(dp.panel, src)))

        def progress(key, value):
            res[key] = value
            print(f"[{name}] {key} = {value}", file=sys.stderr, flush=True)

        progress("device_launches_ms", timed(launches))
        progress("device_compose_and_copy_ms", timed(device))
        progress("host_copy_f32_sources_ms", timed(copy_sources))
        progress("host_numpy_compose_ms", timed(host_compose, a.host_reps))
        progress("host_total_ms", round(res["host_copy_f32_sources_ms"] + res["host_numpy_compose_ms"], 3))
        launches()
        res["device_equals_host"] = all(bool((h == dp.canvas.cpu().numpy()).all()) for h, (dp, _) in zip(host_out, panels))
        host_out.clear()
        model.log_dir = tempfile.mkdtemp()
        progress("log_outputs_with_files_ms", timed(lambda: model.log_outputs(out, inputs, None, 0, True, "train"), a.host_reps))
        res["files_bytes"] = sum(os.path.getsize(os.path.join(model.log_dir, f)) for f in os.listdir(model.log_dir))
        print(json.dumps(res), flush=True)
        del model, trainer, panels
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
