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

A model that was handed a nav dataset's top-down assets (model.topdown_assets) also logs `regressed_state_topdown` and
`action_traj_topdown`: the maze with the state trajectories drawn on it by gcpx_topdown_trajectories (csrc/topdown_traj.hip; the spec
and its numpy mirror are visualization.render_trajectories_numpy), from the states, the regressed states and the matching distribution
where they already are, on the device.

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
    gamma = model._plan_of(o).rec.get("gamma")
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


# ---- state trajectories on the nav datasets' top-down map (base_gcp.py:311-327, nav_9rooms.py:11-54) --------------------------------
class TrajectoryRenderer:
    """the picture and the stamps of a nav dataset's `topdown_assets.npz` on the device, and the uint8 canvases [n, S, S, 3] that
    gcpx_topdown_trajectories (csrc/topdown_traj.hip) draws into, one per key, allocated once"""

    def __init__(self, assets, device):
        import torch
        self.assets, self.device = assets, torch.device(device)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
        rgb = lambda c: int(c[0]) | int(c[1]) << 8 | int(c[2]) << 16
        self.background, self.agent_stamp, self.goal_stamp = (t(assets["background"]), t(assets["agent_stamp"].astype(np.uint8)),
                                                              t(assets["goal_stamp"].astype(np.uint8)))
        self.S, self.cw, self.k = int(assets["S"]), int(assets["cw"]), int(assets["agent_stamp"].shape[0])
        self.agent_rgb, self.goal_rgb = rgb(assets["agent_color"]), rgb(assets["goal_color"])
        self.canvases = {}

    def render(self, lib, layers, n, stream, key=None):
        """layers: [dict(states f32 device tensor [>= n, P, 2] (any strides), length int32 / int64 device tensor [>= n] (end_ind + 1),
        color (three floats), dim_t int32 device tensor [n, K] or None)] -> the uint8 device canvas [n, S, S, 3] of `key`.  One call of
        the export on `stream`; nothing is copied to the host."""
        import torch
        canvas = self.canvases.get((key, n))
        if canvas is None:
            canvas = self.canvases[(key, n)] = torch.empty((n, self.S, self.S, 3), dtype=torch.uint8, device=self.device)
        tab = (rt.TrajLayer * max(len(layers), 1))()
        dims = {2}
        for d, L in zip(tab, layers):
            st, ln, dt = L["states"], L["length"], L.get("dim_t")
            assert st.dtype == torch.float32 and st.dim() == 3 and st.shape[0] >= n and ln.shape[0] >= n, (st.shape, ln.shape)
            assert ln.dtype in (torch.int32, torch.int64) and ln.is_contiguous(), ln.dtype
            dims.add(int(st.shape[2]))
            d.states, (d.s_n, d.s_p, d.s_d), d.P = st.data_ptr(), st.stride(), st.shape[1]
            d.len, d.len_i64 = ln.data_ptr(), int(ln.dtype == torch.int64)
            d.color = (C.c_float * 3)(*[float(c) for c in L["color"]])
            if dt is not None:
                assert dt.dtype == torch.int32 and dt.is_contiguous() and dt.dim() == 2 and dt.shape[0] >= n, (dt.dtype, dt.shape)
                d.dim_t, d.K = dt.data_ptr(), dt.shape[1]
        a = self.assets
        rt.check(lib.gcpx_topdown_trajectories(self.background.data_ptr(), self.S, self.cw, self.agent_stamp.data_ptr(),
                                               self.goal_stamp.data_ptr(), self.k, self.agent_rgb, self.goal_rgb, tab, len(layers), n,
                                               max(dims), int(a["n_rooms"]), int(a["scale"]), canvas.data_ptr(), stream),
                 "topdown_trajectories")
        return canvas


def trajectory_renderer(model):
    """the model's TrajectoryRenderer, or None when the model was given no top-down assets (model.topdown_assets: the trainer sets it
    for a top-rendered dataset class)"""
    assets = getattr(model, "topdown_assets", None)
    if assets is None:
        return None
    cache = model.__dict__.setdefault("_image_log_panels", {})
    r = cache.get("topdown_renderer")
    if r is None or r.assets is not assets:
        r = cache["topdown_renderer"] = TrajectoryRenderer(assets, model.device)
    return r


def bottleneck_frames(model, match_dist_df, n, stream, K=7):
    """int32 device tensor [n, min(K, N)]: `tree.bf.match_dist.argmax(2)[:, :7]` (nav_9rooms.py:42) of the depth-first matching
    distribution [B, N, T], one small launch, cached output"""
    import torch
    B, N, T = match_dist_df.shape
    K = min(K, N)
    cache = model.__dict__.setdefault("_image_log_panels", {})
    out = cache.get(("bottlenecks", n, K))
    if out is None:
        out = cache[("bottlenecks", n, K)] = torch.empty((n, K), dtype=torch.int32, device=match_dist_df.device)
    assert match_dist_df.is_contiguous() and match_dist_df.dtype == torch.float32
    rt.check(model.lib.gcpx_topdown_bottlenecks(match_dist_df.data_ptr(), B, N, T, (N + 1).bit_length() - 1, n, K, out.data_ptr(), stream),
             "topdown_bottlenecks")
    return out


def trajectory_layers(model, outputs, inputs, stream, n=V.N_LOGGED_SAMPLES):
    """{panel name: layers} of log_dataset_specific_trajectory for a model's outputs: `regressed_state_topdown` (ground truth green,
    regressed states red, the segments around the matched frames of the top three tree levels darkened when the tree has a matching)
    and `action_traj_topdown` (the cumulated full-sequence actions from the first regressed state; only where the forward produced
    them: the reference re-runs the inverse model on a training step, this build does not).  The first min(n, B) samples are drawn.
    Empty without regressed states or ground-truth states, and when the regressed states are not (x, y) pairs (state_dim != 2: the
    reference's renderer takes two columns)."""
    import torch
    o = outputs.raw
    rs = o.get("regressed_state_padded")
    if rs is None or "traj_seq_states" not in inputs:
        return {}
    n = min(n, rs.shape[0])
    gt = torch.as_tensor(inputs["traj_seq_states"]).to(device=model.device, dtype=torch.float32)
    if gt.shape[-1] < 2 or rs.shape[-1] != 2:
        return {}
    length = outputs.end_ind + 1                             # int64 [B], on the device
    dim_t = bottleneck_frames(model, o["match_dist_df"], n, stream) if "match_dist_df" in o else None
    truth = dict(states=gt[..., :2], length=length, color=V.GREEN)
    res = {"regressed_state_topdown": [truth, dict(states=rs, length=length, color=V.RED, dim_t=dim_t)]}
    act = o.get("actions_padded")
    if act is not None and act.dim() == 3 and act.shape[-1] == 2:
        cum = torch.cat((rs[:, :1], act), dim=1).cumsum(1)
        res["action_traj_topdown"] = [truth, dict(states=cum, length=length, color=V.RED, dim_t=dim_t)]
    return res


def numpy_layers(layers):
    """the same layers on the host, for visualization.render_trajectories_numpy"""
    h = lambda t: None if t is None else t.detach().cpu().numpy()
    return [dict(states=h(L["states"]), length=h(L["length"]), color=L["color"], dim_t=h(L.get("dim_t"))) for L in layers]


def write_trajectory_png(path, assets, states, device, lib=None, color=V.RED):
    """one red polyline of `states` [m, >= 2] on the map, drawn on the device and written as a PNG (the `metrics/trajectories` pictures
    and the planner's `inferStateTraj`)"""
    import torch
    st = torch.as_tensor(np.asarray(states, dtype=np.float32)[None, :, :2]).to(device).contiguous()
    r = TrajectoryRenderer(assets, device) if not isinstance(assets, TrajectoryRenderer) else assets
    ln = torch.full((1,), st.shape[1], dtype=torch.int64, device=st.device)
    canvas = r.render(lib or rt.lib(), [dict(states=st, length=ln, color=color)], 1, torch.cuda.current_stream(st.device).cuda_stream,
                      key="single")
    return write_png(path, canvas.cpu().numpy()[0])


def write_metric_trajectories(model, inputs, exp_path, step, n=V.N_PLOTTED_ELEMENTS):
    """dump_traj_overview (compute_metrics.py:253-261): `<exp>/metrics/trajectories/it_<step>/trajectories_<b>.png` for the first n
    sequences of a batch, one red polyline of traj_seq_states[b, :end_ind + 1] each.  One launch, one copy.  Returns the files."""
    import torch
    renderer = trajectory_renderer(model)
    if renderer is None or "traj_seq_states" not in inputs:
        return []
    st = torch.as_tensor(inputs["traj_seq_states"]).to(device=model.device, dtype=torch.float32)
    end = torch.as_tensor(inputs["end_ind"]).to(device=model.device)
    n = min(n, st.shape[0])
    stream = torch.cuda.current_stream(model.device).cuda_stream
    canvas = renderer.render(model.lib, [dict(states=st[..., :2], length=(end + 1).to(torch.int64), color=V.RED)], n, stream,
                             key="metric").cpu().numpy()
    folder = os.path.join(exp_path, "metrics", "trajectories", f"it_{step}")
    return [write_png(os.path.join(folder, f"trajectories_{b}.png"), canvas[b]) for b in range(n)]


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
    renderer = trajectory_renderer(model)
    drawn = []
    if renderer is not None:                                 # a nav dataset: the maze with the state trajectories, one launch each
        n = min(V.N_LOGGED_SAMPLES, int(outputs.end_ind.shape[0]))
        for name, layers in trajectory_layers(model, outputs, inputs, stream, n).items():
            drawn.append((name, renderer.render(model.lib, layers, n, stream, key=name)))
    files, model.last_panels = [], {}
    for name, canvas in drawn:
        canvas = canvas.cpu().numpy()
        model.last_panels[name] = canvas
        files.append(write_png(os.path.join(model.log_dir, f"{name}_{phase}_{step}.png"), canvas.reshape(-1, *canvas.shape[2:])))
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


# ---- the planner's verbose pictures (ImageCEMPlanner.log_verbose, cem_planner.py:222-254) ---------------------------------------------
def _elite_images(model, entry, start_state):
    """per elite [len, 3, H, W] on the device.  Elites that were scored on latents only are decoded here, all of them in one batch
    (the decoder takes its skip activations from the start image); the rows that stand for the raw goal image take it."""
    import torch
    from .planning import env2planner
    if entry.elite_images is not None:
        return [torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x).to(device=model.device, dtype=torch.float32)
                for x in entry.elite_images]
    lat = entry.elite_latents
    lens = [int(x.shape[0]) for x in lat]
    I0 = env2planner(np.asarray(start_state)).to(model.device)[:1]
    img = model.decoder.decode_seq({"I_0": I0}, torch.cat(lat)[None]).images[0]
    out = list(torch.split(img, lens))
    goal = env2planner(entry.goal_state).to(model.device)[0]
    for x, rows in zip(out, entry.goal_rows or [[]] * len(out)):
        for k in rows:
            x[k] = goal
    return out


def planner_pictures(model, logs, start_state, horizon, renderer=None):
    """The pictures of ONE planner call's verbose log (planner.verbose_logs[r]): [{name: uint8 canvas}] per iteration, names `overview`
    (always), `goal`, and with a TrajectoryRenderer and 2-D elite states `inferStateTraj` (first elite) / `inferStateTrajDist`.
    Composed on the device -- one gcpx_panel_compose per overview, one gcpx_topdown_trajectories per trajectory picture -- and each
    copied to the host once.  `sources` of every entry: the host copies the numpy mirrors take (visualization.plan_overview_numpy,
    render_trajectory_dist_numpy)."""
    import torch
    res_all = []
    stream = torch.cuda.current_stream(model.device).cuda_stream
    cache = model.__dict__.setdefault("_image_log_panels", {})
    for entry in logs:
        elites = _elite_images(model, entry, start_state)
        E, res = len(elites), int(elites[0].shape[-1])
        padded = torch.ones((E, horizon) + tuple(elites[0].shape[1:]), dtype=torch.float32, device=model.device)
        for e, x in enumerate(elites):
            padded[e, :min(x.shape[0], horizon)] = x[:horizon]
        key = ("plan_overview", res, horizon, E)
        dp = cache.get(key)
        if dp is None:
            dp = cache[key] = DevicePanel(V.plan_overview(res, horizon, E), model.device)
        pics = {"overview": dp.compose(model.lib, dict(elites=padded), stream).cpu().numpy()[0].copy()}
        sources = {"elites": [x.cpu().numpy() for x in elites]}
        g = np.asarray(entry.goal_state)
        g = g[0] if g.ndim == 4 else g
        pics["goal"] = g if g.dtype == np.uint8 else V.to_uint8(g.astype(np.float32) / (np.float32(255) if g.max() > 1.0 else np.float32(1)))
        st = entry.elite_states
        if renderer is not None and st is not None and len(st) and int(st[0].shape[-1]) == 2:
            st = [torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x).to(device=model.device, dtype=torch.float32)
                  for x in st if len(x)][:V.TRAJ_MAX_LAYERS]
            if st:
                P = max(int(x.shape[0]) for x in st)
                pad = torch.zeros((len(st), P, 2), dtype=torch.float32, device=model.device)
                for e, x in enumerate(st):
                    pad[e, :x.shape[0]] = x
                ln = torch.tensor([int(x.shape[0]) for x in st], dtype=torch.int64, device=model.device)
                layers = [dict(states=pad[e:e + 1], length=ln[e:e + 1], color=V.RED) for e in range(len(st))]
                pics["inferStateTraj"] = renderer.render(model.lib, layers[:1], 1, stream, key="plan_single").cpu().numpy()[0].copy()
                pics["inferStateTrajDist"] = renderer.render(model.lib, layers, 1, stream, key="plan_dist").cpu().numpy()[0].copy()
                sources["states"] = [x.cpu().numpy() for x in st]
        res_all.append(dict(pictures=pics, sources=sources))
    return res_all


def write_planner_pictures(out_dir, pair, replan, pictures):
    """`plan_{pair}_r{replan}_iter{i}_{name}.png` for what planner_pictures returned; the files written"""
    files = []
    for i, p in enumerate(pictures):
        for name, canvas in p["pictures"].items():
            files.append(write_png(os.path.join(out_dir, f"plan_{pair}_r{replan}_iter{i}_{name}.png"), canvas))
    return files
