"""Time of the top-down batch assembly at the c2 shape (B=16, T=80, 64 x 64) with the nav datasets' crop window (cw = 40, 25 rooms).

One seeded batch of the image-less fixture dataset (tests/topdown_fixture.py), three ways:
  topdown  gcpx_topdown_assemble_batch: frames rendered from pixel coordinates out of the device-resident picture, resized 80 -> 64;
  resize   gcpx_resize_assemble_batch on the same frames rendered beforehand by numpy and uploaded as uint8 [B][T][80][80][3] -- the
           yardstick: the recorded-frame path with the same resize and the same output traffic (its upload is not timed);
  host     render_topdown_numpy + resize_frames_numpy + the f32 conversion for the batch on the host (assemble_numpy).
Device figures: device events around --calls back-to-back calls (both launches of an export), alternating topdown / resize for --rounds
rounds after a warm-up of each; microseconds per call, median and range over the rounds.  The outputs of the two exports are compared
before anything is timed.  Prints one JSON line.  For kernel times run it under `rocprofv3 --kernel-trace --stats -- python ...`.
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
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host_reps", type=int, default=2)
    a = ap.parse_args()
    import numpy as np
    import torch
    import video_gcp_amd  # noqa: F401
    from video_gcp_amd import dataset as DS
    from video_gcp_amd import runtime as rt
    import topdown_fixture as TF

    B, T, img, cw = 16, 80, 64, 40
    dev = torch.device("cuda:0")
    lib = rt.load_library()
    with tempfile.TemporaryDirectory() as tmp:
        TF.write_topdown_dataset(tmp, T=T, n_files=2, traj_per_file=B, seed=8, min_len=T, split=(1.0, 0.0, 0.0), n_rooms=25, cw=cw)
        ds = DS.VideoDataset(tmp, DS.load_spec(tmp), "train", img)
        batch = DS.epoch_schedule(len(ds), B, 1, seed=4, epoch=0, shuffle=True)[0]
        items = [ds.item(i, DS.item_rng(4, c, p)) for i, p, c in batch]
    assets = ds.topdown
    host_ms = []
    for _ in range(a.host_reps):
        t0 = time.perf_counter()
        ref = DS.assemble_numpy(items, T, img_sz=img, topdown=assets)
        host_ms.append((time.perf_counter() - t0) * 1e3)
    S, A = 2, items[0][0]["actions"].shape[-1]
    naux = B * T + B * T * S + B * (T - 1) * A
    coords, aux = np.zeros(B * T * 2 + B * 2, dtype=np.int32), np.zeros(naux, dtype=np.float32)
    info = np.zeros((B, DS.N_INFO), dtype=np.int32)
    frames = np.zeros((B, T, 2 * cw, 2 * cw, 3), dtype=np.uint8)
    for j, it in enumerate(items):
        DS.pack_item(it, j, coords, aux, info, B, T, S, A, topdown=assets)
        pix, goal = DS.topdown_item_pixels(it, T, assets)
        frames[j, :pix.shape[0]] = DS.render_topdown_numpy(assets, pix, goal)      # the window's frames, as a recorded dataset stores them
    t = lambda x: torch.from_numpy(x).to(dev)
    d = dict(coords=t(coords), aux=t(aux), info=t(info), frames=t(frames), lut=t(DS.LUT))
    dassets = DS.topdown_device_assets(assets, img, dev)

    def outputs():
        return dict(traj_seq=torch.empty(B, T, 3, img, img, device=dev), I_0=torch.empty(B, 3, img, img, device=dev),
                    I_g=torch.empty(B, 3, img, img, device=dev), pad_mask=torch.empty(B, T, device=dev),
                    end_ind=torch.empty(B, dtype=torch.int64, device=dev), start_ind=torch.empty(B, dtype=torch.int64, device=dev),
                    traj_seq_states=torch.empty(B, T, S, device=dev), actions=torch.empty(B, T - 1, A, device=dev))

    out_t, out_r = outputs(), outputs()
    stream = torch.cuda.current_stream(dev).cuda_stream
    topdown = lambda: DS.topdown_assemble_into(lib, dassets, d["coords"], d["aux"], d["info"], d["lut"], None, None, out_t, S, A, stream)
    resize = lambda: DS.resize_assemble_into(lib, d["frames"], d["aux"], d["info"], d["lut"], dassets["tables"], None, None, out_r, S, A,
                                             stream)
    topdown()
    resize()
    torch.cuda.synchronize()
    equal = all(torch.equal(out_t[k], out_r[k]) for k in out_t) and torch.equal(out_t["traj_seq"].cpu(), torch.from_numpy(ref["traj_seq"]))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.calls

    timed(topdown)
    timed(resize)
    rt_, rr = [], []
    for _ in range(a.rounds):
        rt_.append(timed(topdown))
        rr.append(timed(resize))
    med = lambda v: sorted(v)[len(v) // 2]
    out_bytes = (B * T + 2 * B) * 3 * img * img * 4
    print(json.dumps({"workload": "topdown_assemble_time", "B": B, "T": T, "img_sz": img, "crop_window": cw,
                      "background_bytes": int(assets["background"].nbytes), "frame_slot_bytes": int(frames.nbytes),
                      "coord_slot_bytes": int(coords.nbytes), "output_bytes": out_bytes, "exports_equal": bool(equal),
                      "calls_per_round": a.calls, "topdown_us_per_call": round(med(rt_), 2),
                      "topdown_us_range": [round(min(rt_), 2), round(max(rt_), 2)], "resize_us_per_call": round(med(rr), 2),
                      "resize_us_range": [round(min(rr), 2), round(max(rr), 2)], "topdown_over_resize": round(med(rt_) / med(rr), 4),
                      "host_numpy_batch_ms": round(min(host_ms), 1)}), flush=True)
    if not equal:
        sys.exit("the two exports differ")


if __name__ == "__main__":
    main()
