"""Picture logs of the trainer: the panels of the reference's `model.log_outputs(..., log_images=True)` (tree.py:79-108,
sequential.py:116-121), composed on the device and written as PNG / animated PNG.

Every source of a panel is already in device memory (the decoded node images, node_t, the matching distribution, the per-level
attention weights, the input frames), and where a node's tile goes is a device integer, so one launch of gcpx_panel_compose
(csrc/panel.hip) writes a panel's uint8 canvas without a host sync; one device-to-host copy of that canvas follows.  The tile tables
come from visualization.py (which also holds their numpy restatement), are uploaded once per (panel, sizes) and are cached on the model
together with their canvas: a logging step builds no table and allocates nothing.

Files (standard library only: zlib, struct): stills `<log_dir>/<name>_<phase>_<step>.png`, videos `..._<step>.apng` — animated PNG
(acTL / fcTL / fdAT chunks) at the reference logger's 4 frames per second, whose first frame is a plain IDAT, so any PNG reader shows
frame 0 and every browser plays the rest.  All rows use filter type 0.

Not built: pruned_pred (this build's tree has no dense-rec module, and its action row needs cv2), pixel_copy_masks, pruned_tree,
draw_frame's colour borders, log_prior_images (hard-wired off in the reference), scalars.
"""
import ctypes as C
import os
import struct
import zlib

import numpy as np

from . import runtime as rt
from . import visualization as V


# ---- PNG / APNG ---------------------------------------------------------------------------------------------------------------------
def _chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def _rows(frame):
    """zlib stream of an [H, W, 3] uint8 frame, every row with filter type 0"""
    H, W, _ = frame.shape
    raw = np.zeros((H, 1 + W * 3), np.uint8)
    raw[:, 1:] = frame.reshape(H, W * 3)
    return zlib.compress(raw.tobytes(), 6)


def encode_png(frames, fps=V.FPS):
    """bytes of a PNG (one frame) or APNG (several) of uint8 frames [n, H, W, 3] (or [H, W, 3])"""
    frames = np.ascontiguousarray(frames, dtype=np.uint8)
    if frames.ndim == 3:
        frames = frames[None]
    n, H, W, ch = frames.shape
    assert ch == 3 and n >= 1 and H >= 1 and W >= 1, frames.shape
    out = [b"\x89PNG\r\n\x1a\n", _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0))]
    if n > 1:
        out.append(_chunk(b"acTL", struct.pack(">II", n, 0)))                 # n frames, loop forever
    seq = 0
    for i in range(n):
        if n > 1:                                                             # delay = 1 / fps s, dispose none, blend source
            out.append(_chunk(b"fcTL", struct.pack(">IIIIIHHBB", seq, W, H, 0, 0, 1, int(fps), 0, 0)))
            seq += 1
        data = _rows(frames[i])
        if i == 0:
            out.append(_chunk(b"IDAT", data))
        else:
            out.append(_chunk(b"fdAT", struct.pack(">I", seq) + data))
            seq += 1
    out.append(_chunk(b"IEND", b""))
    return b"".join(out)


def write_png(path, frames, fps=V.FPS):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as f:
        f.write(encode_png(frames, fps))
    return path


# ---- the device composer ------------------------------------------------------------------------------------------------------------
_FIELDS = [name for name, _ in rt.PanelTile._fields_ if name != "_pad"]


def tile_table(panel):
    """(ctypes array of gcpx_panel_tile, slot names) of a visualization.Panel"""
    names = panel.sources
    assert len(names) <= rt.PANEL_MAX_SRCS, names
    tab = (rt.PanelTile * max(len(panel.tiles), 1))()
    for d, t in zip(tab, panel.tiles):
        for k in _FIELDS:
            v = t[k]
            if k in ("src", "index", "length"):
                v = -1 if v is None else names.index(v)
            setattr(d, k, v)
    return tab, names


def launch_panel(lib, table_ptr, n_tiles, names, tensors, panel, canvas_f32, canvas_u8, stream):
    """one gcpx_panel_compose over the device tensors `tensors[name]` (contiguous; f32 sources, int32 / int64 indices as the tiles say)"""
    ptrs, elems = (C.c_void_p * rt.PANEL_MAX_SRCS)(), (C.c_int64 * rt.PANEL_MAX_SRCS)()
    for i, name in enumerate(names):
        t = tensors[name]
        assert t.is_contiguous(), name
        ptrs[i], elems[i] = t.data_ptr(), t.numel()
    rt.check(lib.gcpx_panel_compose(table_ptr, n_tiles, ptrs, elems, len(names), panel.n, panel.H, panel.W, C.c_float(panel.background),
                                    int(panel.post_rescale), rt.ptr(canvas_f32), rt.ptr(canvas_u8), stream), "panel_compose")


class DevicePanel:
    """a panel's tile table on the device and its uint8 canvas, built once"""

    def __init__(self, panel, device):
        import torch
        self.panel = panel
        tab, self.names = tile_table(panel)
        self.n_tiles = len(panel.tiles)
        host = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8)
        self.table = host.to(device)
        self.canvas = torch.empty((panel.n, panel.H, panel.W, 3), dtype=torch.uint8, device=device)

    def compose(self, lib, tensors, stream, f32=None):
        launch_panel(lib, self.table.data_ptr(), self.n_tiles, self.names, tensors, self.panel, f32, self.canvas, stream)
        return self.canvas


def numpy_sources(tensors):
    """the same sources on the host, for visualization.compose"""
    return {k: v.detach().cpu().numpy() for k, v in tensors.items()}


# ---- which panels a model's outputs give (tree.py:85-108, sequential.py:119-121) -------------------------------------------------------
def _frames_on(model, inputs, name="traj_seq"):
    import torch
    if name not in inputs:
        raise ValueError(f"picture logs need inputs['{name}']")
    return torch.as_tensor(inputs[name]).to(device=model.device, dtype=torch.float32).contiguous()


def _node_steps(model, outputs, matching):
    """int32 [B, N], depth-first: the time step each node is drawn at in hierarchical_splits (`subgoal.ind`, logger.py:145).
    Balanced binding: node_t, the matched time steps.  Adaptive binding with a matching: best_t, the argmax of the matching
    distribution (adaptive.py:121; "gets overwritten w/ argmax of matching at training time", tree_module.py:113).  Adaptive binding
    without one (a prior-sampled prediction): the midpoints (start_ind + end_ind) / 2 of tree_module.py:113 themselves, which for
    node j of level l are end_ind * (2 j + 1) / 2^(l + 1), truncated as logger.py:145 truncates them -- three small elementwise
    launches on a logging step, the fractions cached."""
    import torch
    hp, o = model._hp, outputs.raw
    if not hp.adaptive:
        return o["node_t"]
    if matching:
        return o["best_t"]
    cache = model.__dict__.setdefault("_image_log_panels", {})
    L = hp.hierarchy_levels
    frac = cache.get(("midpoints", L))
    if frac is None:
        lj = [V.node_level(i, L) for i in range(2 ** L - 1)]
        frac = cache[("midpoints", L)] = torch.tensor([(2 * j + 1) / 2 ** (l + 1) for l, j in lj], dtype=torch.float32,
                                                      device=model.device)
    return (outputs.end_ind.to(torch.float32)[:, None] * frac[None]).to(torch.int32)


def tree_panels(model, outputs, inputs, phase):
    """[(cache key, builder of the visualization.Panel, {source name: device tensor}, trim)] for a GCPTreeModel's outputs; trim: None,
    or the int32 device tensor of sequence lengths whose maximum is the number of frames of the video (pad_sequence,
    visualization.py:487).  The builder runs once per key: the tables are not rebuilt on a logging step."""
    hp, o = model._hp, outputs.raw
    L, res, T, B = hp.hierarchy_levels, hp.img_sz, hp.max_seq_len, outputs.end_ind.shape[0]
    n, ns = V.N_LOGGED_SAMPLES, min(V.N_LOGGED_SEQS, B)
    assert B >= n, f"picture logs show {n} samples: the batch holds {B} (logger.py:119)"
    if o.get("images_df") is None:
        return []                                            # val_mode(decode=False): nothing was decoded
    traj = _frames_on(model, inputs)
    matching = "match_dist_df" in o
    src = dict(traj_seq=traj, images_df=o["images_df"], node_t=_node_steps(model, outputs, matching), end_ind=outputs.end_ind)
    gamma = model._plans_rec(o).get("gamma")
    attentive = gamma is not None
    if attentive:
        src.update({f"gamma{l}": g for l, g in gamma.items()})
    if matching:
        src["match_dist_df"] = o["match_dist_df"]
        src["soft"] = model.soft_matched_estimates(outputs)
    sizes = (L, res, T, B)
    res_list = [(("hierarchical_splits", sizes, attentive, matching),
                 lambda: V.hierarchical_splits(L, res, T, n, attentive=attentive, soft=matching), src, None)]
    if "pruned_padded" in o:
        lens = o["pruned_len" if "pruned_len" in o else "seq_len"]
        F = o["pruned_padded"].shape[1]
        res_list.append((("pruned_seq_gif", sizes, F),
                         lambda: V.rows_gif("pruned_seq_gif", res, [("pruned_padded", F, "pruned_len")], ns, F),
                         dict(pruned_padded=o["pruned_padded"], pruned_len=lens), lens))
    if matching:
        res_list.append((("match_overview", sizes), lambda: V.match_overview("match_overview", L, res, T, n, "match_dist", soft=True),
                         src, None))
        rows = [("traj_seq", T, None), ("soft", T, None)] if phase == "train" else [("soft", T, None)]
        res_list.append((("gt_target_gif", sizes, phase), lambda: V.rows_gif("gt_target_gif", res, rows, ns, T), src, None))
    if phase == "val":
        res_list.append((("output_tree", sizes), lambda: V.output_tree(L, res, T, n), src, None))
    if attentive:
        res_list.append((("attention_masks", sizes, matching),
                         lambda: V.match_overview("attention_masks", L, res, T, n, "gamma", soft=matching), src, None))
    return res_list


def sequential_panels(model, outputs, inputs, phase):
    hp = model._hp
    res, B = hp.img_sz, outputs.end_ind.shape[0]
    images = outputs.dense_rec.images
    F = images.shape[1]
    src = dict(dense_rec=images)
    rows = [("dense_rec", F, None)]
    if phase == "train":                                     # log_dense_gif (logger.py:214-221): the input sequence on top
        src["traj_seq"] = _frames_on(model, inputs)
        rows = [("traj_seq", src["traj_seq"].shape[1], None)] + rows
    return [(("dense_rec", res, B, F, phase), lambda: V.rows_gif("dense_rec", res, rows, min(V.N_LOGGED_SEQS, B), F), src, None)]


def log_outputs(model, panels_fn, outputs, inputs, losses, step, log_images, phase):
    """the body of `model.log_outputs`: composes every panel of `outputs` on the device, copies the uint8 canvases to the host and
    writes them under model.log_dir (stills: the logged samples one below the other).  Returns the files written; model.last_panels
    keeps {name: uint8 canvas [n, H, W, 3]} of this call.  With log_images false it returns at once: no launch, no copy, no file."""
    if not log_images:
        return []
    import torch
    if not getattr(model, "log_dir", None):
        raise ValueError("model.log_dir is not set: picture logs need a directory (the trainer uses <exp>/images)")
    cache = model.__dict__.setdefault("_image_log_panels", {})
    stream = torch.cuda.current_stream(model.device).cuda_stream
    done = []
    for key, build, tensors, trim in panels_fn(model, outputs, inputs, phase):
        dp = cache.get(key)
        if dp is None:
            dp = cache[key] = DevicePanel(build(), model.device)
        dp.compose(model.lib, tensors, stream)
        done.append((dp, trim))
    files, model.last_panels = [], {}
    for dp, trim in done:
        canvas = dp.canvas.cpu().numpy()                     # the one device-to-host copy of the panel (it waits for the launch)
        if trim is not None:
            canvas = canvas[:max(int(trim.max().item()), 1)]
        name = dp.panel.name
        model.last_panels[name] = canvas
        if dp.panel.video:
            files.append(write_png(os.path.join(model.log_dir, f"{name}_{phase}_{step}.apng"), canvas))
        else:
            files.append(write_png(os.path.join(model.log_dir, f"{name}_{phase}_{step}.png"), canvas.reshape(-1, *canvas.shape[2:])))
    return files
