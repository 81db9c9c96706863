"""Device-resident datasets: a split uploaded once and kept in HBM as uint8, batches assembled from it through an index.

`HostFedLoader` (dataset.py) reads, slices, packs and uploads every batch's frames again each epoch, and the host work bounds the
training step.  Here the frames of the whole split cross once: `ResidentStore` reads every trajectory through
`VideoDataset.read` (the same checks), and keeps on the device
    frames   uint8, all trajectories back to back in dataset index order, each [n_i, Hs, Ws, 3], no padding between them,
    states   f32 [sum n_i, S],
    actions  f32 [sum (n_i - 1), A]            (S or A is 0 when the files have none),
and on the host one row per trajectory: first frame index, n_i, first state / action row and the pad mask — all that
`VideoDataset.draw` reads, so the reference's draws (dataset.py, tests/golden/ref_dataset.npz) are made without opening a file.

Per batch `ResidentLoader` makes the B draws, writes 8 int64 per sequence (`resident_info`: which window of which trajectory, chop,
zero_from, end_ind) and the pad masks into one pinned slot, copies that slot (B * (64 + 4 T) bytes) and launches
gcpx_assemble_batch_resident / gcpx_resize_assemble_batch_resident (csrc/batch_assemble.hip) into `model.input_buffer(...)`.
No frame, state or action byte crosses per batch.  Schedule, draws and every tensor of every batch are HostFedLoader's bit for bit;
`resident_batch_numpy` is the same indexing over host copies of the three arrays, the kernels' check on the CPU.

A split that does not fit the budget raises; there is no eviction and no fall-back to the host-fed loader.  Under a process group
every rank holds the whole split: the shuffled order is global, so any rank may be handed any trajectory.  Top-rendered datasets
(dataset.topdown) raise: that path reads no frames and uploads 20 KB of coordinates per batch already.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import runtime as rt
from .dataset import LUT, RingLoader, item_rng, opt_ptr, output_args, resize_frames_numpy, table_args

N_INFO_RESIDENT = 8     # int64 per sequence read by gcpx_assemble_batch_resident (include/gcpx.h)
MAX_WORKERS = 16


class ResidentStore:
    """Every trajectory of `dataset` (a VideoDataset of any phase) on `device`, and the host tables the draws and the index need.
    `budget_bytes`: the most the store may take (default: half of the device's memory); more, or more than is free now, raises
    ValueError before anything is uploaded.  On a CPU `device` the arrays are host tensors and only an explicit budget is checked
    (the layout and the mirror are tested there)."""

    def __init__(self, dataset, device, budget_bytes=None, n_workers=4):
        if dataset.topdown is not None:
            raise ValueError("a top-rendered dataset keeps no frames to make resident: its batches are 20 KB of pixel coordinates, "
                             "drawn on the device already (HostFedLoader)")
        self.ds, self.device = dataset, torch.device(device)
        n_items = len(dataset)
        self.pad_masks = [dataset.pad_mask(i) for i in range(n_items)]
        self.n = np.array([pm.shape[0] for pm in self.pad_masks], dtype=np.int64)
        if (self.n < 1).any():
            raise ValueError(f"{dataset.data_dir}: a trajectory without frames")
        raw0 = dataset.read(0)
        self.S = raw0["states"].shape[-1] if "states" in raw0 else 0
        self.A = raw0["actions"].shape[-1] if "actions" in raw0 else 0
        self.Hs, self.Ws = (int(x) for x in raw0["images"].shape[1:3])
        self.frame_bytes = self.Hs * self.Ws * 3
        # one row per trajectory: where its frames, states and actions begin
        self.first_frame = np.concatenate(([0], np.cumsum(self.n)[:-1])).astype(np.int64)
        self.first_state = self.first_frame.copy()
        self.first_action = np.concatenate(([0], np.cumsum(self.n - 1)[:-1])).astype(np.int64)
        self.n_frames_total = int(self.n.sum())
        self.n_action_rows = int((self.n - 1).sum())
        self.frames_bytes = self.n_frames_total * self.frame_bytes
        self.nbytes = self.frames_bytes + 4 * (self.n_frames_total * self.S + self.n_action_rows * self.A)
        self._check_capacity(budget_bytes)
        self._load(max(1, min(int(n_workers), MAX_WORKERS)))

    def _check_capacity(self, budget_bytes):
        on_gpu = self.device.type == "cuda"
        if budget_bytes is None and on_gpu:
            budget_bytes = torch.cuda.get_device_properties(self.device).total_memory // 2
        if budget_bytes is not None and self.nbytes > budget_bytes:
            raise ValueError(f"the {self.ds.phase} split of {self.ds.data_dir} needs {self.nbytes} bytes on the device "
                             f"({self.n_frames_total} frames of {self.Hs}x{self.Ws}), the budget has {int(budget_bytes)} bytes available: "
                             "raise the budget (train.py --device_dataset_gb) or train host-fed (--device_dataset 0)")
        if on_gpu:
            free = torch.cuda.mem_get_info(self.device)[0]
            if self.nbytes > free:
                raise ValueError(f"the {self.ds.phase} split of {self.ds.data_dir} needs {self.nbytes} bytes on the device, "
                                 f"{free} bytes are available (free) now")

    def _load(self, n_workers):
        """every trajectory once through VideoDataset.read, at most n_workers + 2 of them on the host at a time; the frames go up
        through two pinned buffers of the longest trajectory's size"""
        ds, dev, n_items = self.ds, self.device, len(self.n)
        on_gpu = dev.type == "cuda"
        self.frames = torch.empty(self.frames_bytes, dtype=torch.uint8, device=dev)
        assert self.frames.data_ptr() % 16 == 0
        states = np.empty((self.n_frames_total, self.S), dtype=np.float32)
        actions = np.empty((self.n_action_rows, self.A), dtype=np.float32)
        if on_gpu:
            stage = [torch.empty(int(self.n.max()) * self.frame_bytes, dtype=torch.uint8, pin_memory=True) for _ in range(2)]
            done = [torch.cuda.Event() for _ in range(2)]
            copy = torch.cuda.Stream(device=dev)
        with ThreadPoolExecutor(max_workers=n_workers) as pool:
            futs = {i: pool.submit(ds.read, i) for i in range(min(n_workers, n_items))}
            for i in range(n_items):
                raw = futs.pop(i).result()
                if i + n_workers < n_items:
                    futs[i + n_workers] = pool.submit(ds.read, i + n_workers)
                self._check_item(i, raw)
                f0, n = int(self.first_frame[i]), int(self.n[i])
                b0, nb = f0 * self.frame_bytes, n * self.frame_bytes
                im = np.ascontiguousarray(raw["images"]).reshape(-1)
                if on_gpu:
                    k = i % 2
                    done[k].synchronize()                     # the buffer's previous upload has completed
                    stage[k].numpy()[:nb] = im
                    with torch.cuda.stream(copy):
                        self.frames[b0:b0 + nb].copy_(stage[k][:nb], non_blocking=True)
                        done[k].record(copy)
                else:
                    self.frames.numpy()[b0:b0 + nb] = im
                if self.S:
                    states[f0:f0 + n] = raw["states"]
                if self.A:
                    a0 = int(self.first_action[i])
                    actions[a0:a0 + n - 1] = raw["actions"]
        self.states = torch.from_numpy(states).to(dev)
        self.actions = torch.from_numpy(actions).to(dev)
        if on_gpu:
            copy.synchronize()
            torch.cuda.current_stream(dev).synchronize()

    def _check_item(self, i, raw):
        n, want = int(self.n[i]), {"images": int(self.n[i])}
        if self.S:
            want["states"] = n
        if self.A:
            want["actions"] = n - 1
        for k, m in want.items():
            if k not in raw or raw[k].shape[0] != m:
                raise ValueError(f"trajectory {i} of {self.ds.data_dir} ({self.ds.phase}): {k} has "
                                 f"{raw[k].shape[0] if k in raw else 'no'} rows, its pad mask of {n} entries asks for {m}")
        if raw["images"].shape[1:] != (self.Hs, self.Ws, 3):
            raise ValueError(f"trajectory {i} of {self.ds.data_dir} ({self.ds.phase}): frames are {raw['images'].shape[1:3]}, "
                             f"item 0 has {(self.Hs, self.Ws)}: a resident store holds one frame size")
        if (self.S and raw["states"].shape[-1] != self.S) or (self.A and raw["actions"].shape[-1] != self.A):
            raise ValueError(f"trajectory {i} of {self.ds.data_dir} ({self.ds.phase}): state / action width differs from item 0's")

    def __len__(self):
        return len(self.n)

    def draw(self, index, rs):
        """VideoDataset.draw of trajectory `index` from its stored pad mask: no file is opened"""
        return self.ds.draw({"pad_mask": self.pad_masks[index]}, rs)

    def host_arrays(self):
        """host copies (frames uint8 [sum n_i, Hs, Ws, 3], states, actions) for resident_batch_numpy"""
        return (self.frames.cpu().numpy().reshape(-1, self.Hs, self.Ws, 3), self.states.cpu().numpy(), self.actions.cpu().numpy())


def resident_info(store, index, plan, out=None):
    """the 8 int64 of one sequence: the window of trajectory `index` that starts at plan['offset'] (include/gcpx.h)"""
    o, n = int(plan["offset"]), int(store.n[index])
    row = (int(store.first_frame[index]) + o, max(n - o, 0),
           int(store.first_state[index]) + o, max(n - o, 0) if store.S else 0,
           int(store.first_action[index]) + o, max(n - 1 - o, 0) if store.A else 0,
           int(plan["chop"]), int(plan["zero_from"]) | int(plan["end_ind"]) << 32)
    if out is None:
        return np.array(row, dtype=np.int64)
    out[:] = row
    return out


def resident_batch_info(store, batch, seed):
    """one scheduled batch [(dataset index, position, cycle)] -> (info int64 [B, 8], pad_mask f32 [B, T]) by the reference's draws"""
    info = np.empty((len(batch), N_INFO_RESIDENT), dtype=np.int64)
    pad = np.empty((len(batch), store.ds.T), dtype=np.float32)
    for j, (i, p, c) in enumerate(batch):
        plan = store.draw(i, item_rng(seed, c, p))
        resident_info(store, i, plan, info[j])
        pad[j] = plan["pad_mask"]
    return info, pad


def resident_batch_numpy(store_arrays, info, pad_mask, T, states_mean=None, states_den=None, img_sz=None):
    """(frames uint8 [N, Hs, Ws, 3], states f32 [N, S], actions f32 [M, A]), info int64 [B, 8], pad_mask [B, T] -> the model's inputs as
    numpy arrays: what gcpx_assemble_batch_resident (gcpx_resize_assemble_batch_resident when img_sz differs from the stored size)
    computes, indexing the three arrays as the kernels do.  Frames outside a sequence's own window, or outside the arrays, are padding."""
    frames, states, actions = store_arrays
    B, S, A = info.shape[0], states.shape[-1], actions.shape[-1]
    t, ta = np.arange(T), np.arange(T - 1)
    out = dict(traj_seq=[], traj_seq_states=[], actions=[], end_ind=[])
    for b in range(B):
        first, nf, srow, ns, arow, na, chop, packed = (int(x) for x in info[b])
        chop, zero_from, end_ind = max(chop, 0), packed & 0xffffffff, packed >> 32
        s = np.minimum(t + chop, T - 1)
        valid = (t < zero_from) & (s < min(nf, T)) & (first >= 0) & (first + s < frames.shape[0])
        im = np.zeros((T,) + frames.shape[1:], dtype=np.uint8)
        im[valid] = frames[first + s[valid]]
        if img_sz is not None and im.shape[1:3] != (img_sz, img_sz):
            im = resize_frames_numpy(im, img_sz)
        out["traj_seq"].append(LUT[np.transpose(im, (0, 3, 1, 2))])
        out["end_ind"].append(end_ind)
        if S:
            valid = (t < zero_from) & (s < min(ns, T)) & (srow >= 0)
            x = np.zeros((T, S), dtype=np.float32)
            x[valid] = states[srow + s[valid]]
            if states_mean is not None:
                x = (x - states_mean) / states_den
            out["traj_seq_states"].append(x.astype(np.float32))
        if A:
            s = np.minimum(ta + chop, T - 2)
            valid = (ta < zero_from) & (s < min(na, T - 1)) & (arow >= 0)
            x = np.zeros((T - 1, A), dtype=np.float32)
            x[valid] = actions[arow + s[valid]]
            out["actions"].append(x)
    res = {k: np.stack(v) for k, v in out.items() if len(v) and k != "end_ind"}
    res["end_ind"] = np.array(out["end_ind"], dtype=np.int64)
    res["start_ind"] = np.zeros(B, dtype=np.int64)
    res["pad_mask"] = np.asarray(pad_mask, dtype=np.float32).reshape(B, T).copy()
    res["I_0"] = res["traj_seq"][:, 0].copy()
    res["I_g"] = res["traj_seq"][np.arange(B), res["end_ind"]].copy()
    return res


def resident_assemble_into(lib, store_ptr, store_bytes, states_ptr, actions_ptr, slot_ptr, B, T, src, lut, tables, mean, den, out, S, A,
                           stream):
    """the resident assembly of one batch into the device tensors of `out` (the model's input names).  slot_ptr: the device slot
    [info int64 B * 8 | pad_mask f32 B * T]; src = (Hs, Ws) of the store; tables None: frames stored at the model's size."""
    H, W = out["traj_seq"].shape[-2:]
    head = (store_ptr, store_bytes, slot_ptr, lut.data_ptr())
    rows = (slot_ptr + 8 * N_INFO_RESIDENT * B, states_ptr if S else None, actions_ptr if A else None, opt_ptr(mean), opt_ptr(den))
    if tables is None:
        rt.check(lib.gcpx_assemble_batch_resident(*head, *rows, B, T, H, W, S, A, *output_args(out, stream)), "assemble_batch_resident")
    else:
        rt.check(lib.gcpx_resize_assemble_batch_resident(*head, *table_args(tables), *rows, B, T, src[0], src[1], H, W, tables[0].shape[1],
                                                         tables[2].shape[1], S, A, *output_args(out, stream)),
                 "resize_assemble_batch_resident")


class ResidentLoader(RingLoader):
    """HostFedLoader's interface and batches (dataset.RingLoader) over a ResidentStore built at construction.  A slot is
    [info int64 B * 8 | pad_mask f32 B * T]: per batch one worker thread makes the B draws from the store's pad masks and fills it, and
    the resident assembly reads it and the store.
    Under a process group every rank holds the whole split (the shuffled order is one global order; a rank may draw any trajectory)."""

    def __init__(self, dataset, model, batch_size, n_repeat=1, seed=0, rank=None, world=None, n_slots=2, shuffle=None, budget_bytes=None,
                 accumulate=1):
        super().__init__(dataset, model, batch_size, n_repeat, seed, rank, world, n_slots, shuffle, n_workers=1, accumulate=accumulate)
        self.store = ResidentStore(dataset, model.device, budget_bytes=budget_bytes)
        self.S, self.A = self.store.S, self.store.A

    def _alloc_slots(self, dev, n):
        nbytes = 8 * N_INFO_RESIDENT * self.B + 4 * self.B * self.ds.T
        self.pin = {"slot": [torch.zeros(nbytes, dtype=torch.uint8, pin_memory=True) for _ in range(n)]}
        self.dev = {"slot": [torch.empty(nbytes, dtype=torch.uint8, device=dev) for _ in range(n)]}
        return self.store.Hs, self.store.Ws

    def _jobs(self, batch):
        return [(self._fill, batch)]

    def _fill(self, slot, batch):
        B, T = self.B, self.ds.T
        info, pad = resident_batch_info(self.store, batch, self.seed)
        buf = self.pin["slot"][slot].numpy()
        buf[:8 * N_INFO_RESIDENT * B].view(np.int64).reshape(B, N_INFO_RESIDENT)[:] = info
        buf[8 * N_INFO_RESIDENT * B:].view(np.float32).reshape(B, T)[:] = pad

    def _launch(self, slot, out, stream):
        store = self.store
        resident_assemble_into(self.model.lib, store.frames.data_ptr(), store.frames_bytes, store.states.data_ptr(),
                               store.actions.data_ptr(), self.dev["slot"][slot].data_ptr(), self.B, self.ds.T, (store.Hs, store.Ws),
                               self.lut, self.tables, self.mean, self.den, out, self.S, self.A, stream)
