"""Time of the resident batch assembly against the host-fed one at the c2 shape (B=16, T=80, frames stored at 128 x 128, resized to 64).

One seeded batch of the fixture dataset (tests/dataset_fixture.py), two ways over the same frames:
  resident  gcpx_resize_assemble_batch_resident: windows of a ResidentStore of the whole split, through the index;
  slot      gcpx_resize_assemble_batch on the same windows packed into a [B][T][128][128][3] slot and uploaded beforehand (the upload is
            not timed) -- the yardstick: both read the same bytes and write the same outputs.
Device events around --calls back-to-back calls (both launches of an export), alternating for --rounds rounds after a warm-up of each;
microseconds per call, median and range over the rounds.  The outputs of the two exports are compared before anything is timed.
`--source_size 64` times the forms without a resize.  Prints one JSON line with the store's load time and bytes.
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
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--source_size", type=int, default=128)
    a = ap.parse_args()
    import numpy as np
    import torch
    import video_gcp_amd  # noqa: F401
    from video_gcp_amd import dataset as DS
    from video_gcp_amd import dataset_resident as DR
    from video_gcp_amd import runtime as rt
    import dataset_fixture as FX

    B, T, img, N = 16, 80, 64, a.source_size
    dev = torch.device("cuda:0")
    lib = rt.load_library()
    with tempfile.TemporaryDirectory() as tmp:
        FX.write_random_dataset(tmp, T=T, img=N, n_files=2, traj_per_file=B, phases=("train",), min_len=T // 2)
        ds = DS.VideoDataset(tmp, DS.load_spec(tmp), "train", img, randomize_length=True, resize=N != img)
        t0 = time.perf_counter()
        store = DR.ResidentStore(ds, dev)
        torch.cuda.synchronize()
        t_load = time.perf_counter() - t0
        batch = DS.epoch_schedule(len(ds), B, 1, seed=4, epoch=0, shuffle=True)[0]
        items = [ds.item(i, DS.item_rng(4, c, p)) for i, p, c in batch]
    S, A = store.S, store.A
    frames = np.zeros((B, T, N, N, 3), dtype=np.uint8)
    aux = np.zeros(B * T + B * T * S + B * (T - 1) * A, dtype=np.float32)
    info = np.zeros((B, DS.N_INFO), dtype=np.int32)
    for j, it in enumerate(items):
        DS.pack_item(it, j, frames, aux, info, B, T, S, A)
    rinfo, rpad = DR.resident_batch_info(store, batch, 4)
    slot = np.concatenate([rinfo.reshape(-1).view(np.uint8), rpad.reshape(-1).view(np.uint8)])
    t = lambda x: torch.from_numpy(x).to(dev)
    d = dict(frames=t(frames), aux=t(aux), info=t(info), slot=t(slot), lut=t(DS.LUT))
    tables = tuple(t(x) for x in DS.resize_tables(N, N, img)) if N != img else None

    def outputs():
        return dict(traj_seq=torch.empty(B, T, 3, img, img, device=dev), I_0=torch.empty(B, 3, img, img, device=dev),
                    I_g=torch.empty(B, 3, img, img, device=dev), pad_mask=torch.empty(B, T, device=dev),
                    end_ind=torch.empty(B, dtype=torch.int64, device=dev), start_ind=torch.empty(B, dtype=torch.int64, device=dev),
                    traj_seq_states=torch.empty(B, T, S, device=dev), actions=torch.empty(B, T - 1, A, device=dev))

    out_r, out_s = outputs(), outputs()
    stream = torch.cuda.current_stream(dev).cuda_stream
    resident = lambda: DR.resident_assemble_into(lib, store.frames.data_ptr(), store.frames_bytes, store.states.data_ptr(),
                                                 store.actions.data_ptr(), d["slot"].data_ptr(), B, T, (N, N), d["lut"], tables, None, None,
                                                 out_r, S, A, stream)
    if tables is None:
        slot_fed = lambda: DS.assemble_into(lib, d["frames"], d["aux"], d["info"], d["lut"], None, None, out_s, S, A, stream)
    else:
        slot_fed = lambda: DS.resize_assemble_into(lib, d["frames"], d["aux"], d["info"], d["lut"], tables, None, None, out_s, S, A, stream)
    resident()
    slot_fed()
    torch.cuda.synchronize()
    equal = all(torch.equal(out_r[k], out_s[k]) for k in out_r)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.calls

    timed(resident)
    timed(slot_fed)
    rr, rs = [], []
    for _ in range(a.rounds):
        rr.append(timed(resident))
        rs.append(timed(slot_fed))
    med = lambda v: sorted(v)[len(v) // 2]
    print(json.dumps({"workload": "resident_assemble_time", "B": B, "T": T, "img_sz": img, "source_size": N,
                      "store_bytes": int(store.nbytes), "store_frames": int(store.n_frames_total), "store_load_s": round(t_load, 3),
                      "frame_slot_bytes": int(frames.nbytes), "resident_slot_bytes": int(slot.nbytes), "exports_equal": bool(equal),
                      "calls_per_round": a.calls, "resident_us_per_call": round(med(rr), 2),
                      "resident_us_range": [round(min(rr), 2), round(max(rr), 2)], "slot_us_per_call": round(med(rs), 2),
                      "slot_us_range": [round(min(rs), 2), round(max(rs), 2)], "resident_over_slot": round(med(rr) / med(rs), 4)}),
          flush=True)
    if not equal:
        sys.exit("the two exports differ")


if __name__ == "__main__":
    main()
