"""Picture-log panels as tables of tile descriptors, and their numpy restatement.

A panel is what one `log_*` call of the reference's HierarchyLogger draws (gcp/prediction/utils/logger.py, visualization.py): a
canvas [n, H, W, 3] with a background value and a list of tiles, each a rectangle copied (or expanded, or added) from a named f32
source tensor.  The panel functions below only do the layout arithmetic of the reference, once per (panel, sizes); `compose` applies a
panel to numpy arrays on the host and is the CPU oracle of the device composer (csrc/panel.hip, image_log.DevicePanel), which reads
the same tiles as a gcpx_panel_tile table.  The semantics of a tile are stated at gcpx_panel_compose in include/gcpx.h.

Deviations from the reference as executed:
  * hierarchical_splits draws every node of every logged sample at its matched time step.  The reference's test
    `'done_mask' in segment` (logger.py:144) iterates the tree's layers and is never true, so its tree rows stay empty.
  * the balanced trees of match_overview / attention_masks / output_tree are plain tiles, without draw_frame's matplotlib colour border.
  * uint8 = trunc(clip(x, 0, 1) * 255): this build's own conversion (the reference leaves it to tensorboardX).

State trajectories on the nav datasets' top-down map (Multiroom3dEnv.render_top_down, multiroom3d_env.py:151-183) are not tiles:
`render_trajectories_numpy` below is the definition of gcpx_topdown_trajectories (csrc/topdown_traj.hip, spec in include/gcpx.h).
  * a segment is the set of pixels within thickness / 2 of it, by an exact integer test: the shape of OpenCV's non-antialiased thick
    line (a rectangle with round ends), not pinned to OpenCV pixel for pixel.
  * a point whose pixel is not finite is skipped and pixels are clamped to +-TRAJ_COORD_LIMIT, where the reference raises.
"""
import math

import numpy as np

IMAGE, GREY, GREY_ADD, FILL = 0, 1, 2, 3
RESCALE, LENGTH_STRICT, INDEX_FRAME, INDEX_I64, LENGTH_I64 = 1, 2, 4, 8, 16

N_LOGGED_SAMPLES = 3          # HierarchyLogger(n_logged_samples=3), visualization.Params.n_logged_samples
N_LOGGED_SEQS = 5             # make_gif(n_seqs_logged=5), log_loss_gif's plot_imgs[:5]
GAMMA_WIDTH = 4               # HierarchyLogger._gamma_width
FPS = 4                       # Logger(fps=4)

_TILE_DEFAULTS = dict(kind=IMAGE, src=None, index=None, length=None, flags=0, nb=1, nf=1, h=0, w=0, tile_w=1, n0=0, n_b=0, n_f=0,
                      r0=0, r_b=0, r_f=0, c0=0, c_b=0, c_f=0, index_off=0, index_stride=0, index_count=0, fill=0.0,
                      off=0, s_b=0, s_f=0, s_c=0, s_y=0)


def tile(**kw):
    t = dict(_TILE_DEFAULTS)
    assert set(kw) <= set(t), set(kw) - set(t)
    t.update(kw)
    return t


class Panel:
    def __init__(self, name, n, H, W, background, post_rescale=False, video=False):
        self.name, self.n, self.H, self.W = name, int(n), int(H), int(W)
        self.background, self.post_rescale, self.video = float(background), bool(post_rescale), bool(video)
        self.tiles = []

    def add(self, **kw):
        self.tiles.append(tile(**kw))

    @property
    def sources(self):
        """the names the tiles read, in first-use order: the slots of the device table"""
        names = []
        for t in self.tiles:
            for k in ("src", "index", "length"):
                if t[k] is not None and t[k] not in names:
                    names.append(t[k])
        return names


def node_level(i, L):
    """(level from the root, position in the level) of depth-first node i of a tree with L levels (tree_utils.py:79-88)"""
    k = i + 1
    tz = (k & -k).bit_length() - 1
    return L - 1 - tz, k >> (tz + 1)


def _frames(src, res, n_frames, **kw):
    """an IMAGE tile over a contiguous [B, n_frames, 3, res, res] tensor"""
    px = res * res
    return dict(kind=IMAGE, src=src, h=res, w=res, s_b=n_frames * 3 * px, s_f=3 * px, s_c=px, s_y=res, **kw)


def _balanced_tree(p, L, res, r0, c0, nb):
    """plot_balanced_tree (visualization.py:232-262) without draw_frame: node n of the depth-first order in column n, row = its level"""
    N = 2 ** L - 1
    for i in range(N):
        level, _ = node_level(i, L)
        p.add(**_frames("images_df", res, N, nb=nb, n_b=1, r0=r0 + level * res, c0=c0 + i * res, off=i * 3 * res * res, flags=RESCALE))


def hierarchical_splits(L, res, T, n=N_LOGGED_SAMPLES, attentive=False, dense=False, soft=False):
    """HierarchyLogger.log_hierarchy_image (logger.py:114-182).  Sources: traj_seq [B, T, 3, res, res], images_df [B, N, 3, res, res],
    node_t int32 [B, N], gamma<l> [B * 2^l, T] per level l (attentive), dense_rec / soft [B, T, 3, res, res], end_ind int64 [B]."""
    N = 2 ** L - 1
    gw = GAMMA_WIDTH if attentive else 0
    lh = res + gw
    rows = res + L * lh + (res if dense else 0) + (res if soft else 0)
    p = Panel("hierarchical_splits", n, rows, T * res, 0.7, post_rescale=True)
    p.add(**_frames("traj_seq", res, T, nb=n, nf=T, n_b=1, c_f=res))                                  # flatten_seq(traj_seq_images)
    for level in range(L if gw else 0):                                                                # strips start at 0 (:130-132)
        p.add(kind=FILL, nb=n, n_b=1, h=gw, w=T * res, r0=res + level * lh, fill=0.0)
    for i in range(N):                                                                                 # depth_first_iter (:138-154)
        level, j = node_level(i, L)
        if gw:
            p.add(kind=GREY_ADD, src=f"gamma{level}", nb=n, n_b=1, h=gw, w=T * res, tile_w=res, r0=res + level * lh,
                  off=j * T, s_b=2 ** level * T, s_c=1)
        p.add(**_frames("images_df", res, N, nb=n, n_b=1, r0=res + level * lh + gw, off=i * 3 * res * res,
                        index="node_t", index_off=i, index_stride=N, index_count=T))
    r = res + L * lh
    for name, on in (("dense_rec", dense), ("soft", soft)):                                            # mask_extra + flatten_seq (:156-178)
        if on:
            p.add(**_frames(name, res, T, nb=n, nf=T, n_b=1, c_f=res, r0=r, length="end_ind", flags=LENGTH_I64))
            r += res
    return p


def rows_gif(name, res, rows, nb, n_frames, gap_zero=True):
    """make_gif (visualization.py:485-497) / log_loss_gif (logger.py:236-253): the first nb sequences side by side, the rows stacked
    with a 2-pixel gap of zeros, one canvas per time step.  rows: [(source, frames of the source, length source or None)]; with a
    length (int32 [B]) the frames from it on are pad_sequence's zeros."""
    p = Panel(name, n_frames, len(rows) * res + 2 * (len(rows) - 1), nb * res, 0.0, video=True)
    for k, (src, F, length) in enumerate(rows):
        p.add(**_frames(src, res, F, nb=nb, nf=min(F, n_frames), n_f=1, c_b=res, r0=k * (res + 2), length=length,
                        flags=RESCALE | (LENGTH_STRICT if length else 0)))
    return p


def match_overview(name, L, res, T, n=N_LOGGED_SAMPLES, attr="match_dist", soft=True):
    """plot_gt_matching_overview (visualization.py:365-400) with PLOT_BINARY_DISTS tiles.  attr 'match_dist': match_dist_df [B, N, T];
    attr 'gamma': gamma<l> [B * 2^l, T] per level."""
    N = 2 ** L - 1
    p = Panel(name, n, (T + L) * res, (N + 2) * res, 0.7)
    p.add(**_frames("traj_seq", res, T, nb=n, nf=T, n_b=1, r_f=res, flags=RESCALE))
    if soft:
        p.add(**_frames("soft", res, T, nb=n, nf=T, n_b=1, r_f=res, c0=res, flags=RESCALE))
    _balanced_tree(p, L, res, T * res, 2 * res, n)
    for i in range(N):                                   # plot_greyscale_dist of match_dists[b, :, t]: node i's value in column i, row t
        if attr == "gamma":
            level, j = node_level(i, L)
            p.add(kind=GREY, src=f"gamma{level}", nb=n, nf=T, n_b=1, h=res, w=res, tile_w=res, r_f=res, c0=(2 + i) * res,
                  off=j * T, s_b=2 ** level * T, s_f=1)
        else:
            p.add(kind=GREY, src="match_dist_df", nb=n, nf=T, n_b=1, h=res, w=res, tile_w=res, r_f=res, c0=(2 + i) * res,
                  off=i * T, s_b=N * T, s_f=1)
    return p


def output_tree(L, res, T, n=N_LOGGED_SAMPLES):
    """plot_val_tree (visualization.py:327-362) on the path without p_n_hat / actions: the balanced tree, start and goal frame"""
    N = 2 ** L - 1
    p = Panel("output_tree", n, L * res + 2 * res, (N + 2) * res, 0.7)
    _balanced_tree(p, L, res, 2 * res, res, n)
    p.add(**_frames("traj_seq", res, T, nb=n, n_b=1, flags=RESCALE))
    p.add(**_frames("traj_seq", res, T, nb=n, n_b=1, c0=(N + 1) * res, flags=RESCALE | INDEX_FRAME | INDEX_I64,
                    index="end_ind", index_stride=1, index_count=T))
    return p


# ---- the numpy restatement ----------------------------------------------------------------------------------------------------------
def compose(panel, sources):
    """f32 canvas [n, H, W, 3] of `panel` over numpy arrays `sources[name]`"""
    one, two = np.float32(1), np.float32(2)
    n, H, W = panel.n, panel.H, panel.W
    canvas = np.full((n, H, W, 3), np.float32(panel.background), np.float32)
    ch = np.arange(3)
    for t in panel.tiles:
        a = None if t["src"] is None else np.asarray(sources[t["src"]], np.float32).reshape(-1)
        idx = None if t["index"] is None else np.asarray(sources[t["index"]]).reshape(-1)
        lens = None if t["length"] is None else np.asarray(sources[t["length"]]).reshape(-1)
        for b in range(t["nb"]):
            iv = 0
            if idx is not None:
                iv = int(idx[t["index_off"] + b * t["index_stride"]])
                if not 0 <= iv < t["index_count"]:
                    continue
            ln = None
            if lens is not None:
                ln = int(lens[b]) - (1 if t["flags"] & LENGTH_STRICT else 0)
            as_frame = idx is not None and t["flags"] & INDEX_FRAME
            for f in range(t["nf"]):
                ni = t["n0"] + b * t["n_b"] + f * t["n_f"]
                if not 0 <= ni < n:
                    continue
                r = t["r0"] + b * t["r_b"] + f * t["r_f"]
                c = t["c0"] + b * t["c_b"] + f * t["c_f"] + (iv * t["w"] if idx is not None and not as_frame else 0)
                y0, y1, x0, x1 = max(r, 0), min(r + t["h"], H), max(c, 0), min(c + t["w"], W)
                if y0 >= y1 or x0 >= x1:
                    continue
                dst = canvas[ni, y0:y1, x0:x1]
                if t["kind"] == FILL:
                    dst[...] = np.float32(t["fill"])
                    continue
                base = t["off"] + b * t["s_b"] + (iv if as_frame else f) * t["s_f"]
                yy, xx = np.arange(y0 - r, y1 - r), np.arange(x0 - c, x1 - c)
                if t["kind"] == IMAGE:
                    v = a[base + ch[None, None, :] * t["s_c"] + yy[:, None, None] * t["s_y"] + xx[None, :, None]]
                else:
                    v = a[base + (xx // max(t["tile_w"], 1)) * t["s_c"]][None, :, None]
                if t["kind"] == GREY_ADD:
                    dst += v
                    continue
                if ln is not None:
                    v = v * np.float32(1.0 if f <= ln else 0.0)
                if t["flags"] & RESCALE:
                    v = (v + one) / two
                dst[...] = v
    if panel.post_rescale:
        canvas = (canvas + one) / two
    return canvas


def to_uint8(canvas):
    """this build's conversion of a [0, 1] f32 canvas to bytes: trunc(clip(x, 0, 1) * 255)"""
    return (np.clip(canvas, np.float32(0), np.float32(1)) * np.float32(255)).astype(np.uint8)


# ---- state trajectories on the top-down map ----------------------------------------------------------------------------------------
TRAJ_THICKNESS = 4            # render_top_down(line_thickness=4); GCPX_TRAJ_THICKNESS (tests/test_topdown_traj_cpu.py compares both
TRAJ_COORD_LIMIT = 16384      # GCPX_TRAJ_COORD_LIMIT                                    with include/gcpx.h)
N_PLOTTED_ELEMENTS = 5        # compute_metrics.py: the sequences whose trajectories --metric plots
GREEN, RED = (0.0, 1.0, 0.0), (1.0, 0.0, 0.0)


def trajectory_pixels(states, n_rooms, scale, S):
    """float32 states [m, 2] -> (int64 pixels [m, 2] of the unpadded S x S picture, bool [m]: the pixel is finite).  The reference's
    float32 expressions (multiroom3d_env.py:163-170): y *= -1; everything / 27 when max > 1 or min < -1 (numpy's max / min return a NaN
    that is there, and then neither holds); + 0.5 * table_size; int(x * scale), S - int(y * scale)."""
    t = np.array(states, dtype=np.float32).reshape(-1, 2)
    t[:, 1] *= np.float32(-1)
    with np.errstate(all="ignore"):
        if t.size and (t.max() > 1.0 or t.min() < -1.0):
            t = t / np.float32(27.0)
        t = t + np.float32(0.5 * ((1 / 3) * int(math.sqrt(n_rooms))))
        f = t * np.float32(scale)
        ok = np.isfinite(f).all(axis=1)
        v = np.clip(np.trunc(np.where(np.isfinite(f), f, np.float32(0))), -2.0 ** 30, 2.0 ** 30).astype(np.int64)
    pix = np.stack([v[:, 0], S - v[:, 1]], axis=1)
    return np.clip(pix, -TRAJ_COORD_LIMIT, TRAJ_COORD_LIMIT), ok


def segment_colors(color, m, length, dim_t=None):
    """uint8 [max(m - 1, 0), 3]: trunc(c * 255) of the base colour, halved once per hit of `color_seq[t] *= 0.5` and
    `color_seq[t - 1] *= 0.5` (nav_9rooms.py:46-49) over the distinct t = min(dim_t, length - 1); negative dim_t are ignored"""
    f = np.ones(max(m - 1, 0), dtype=np.float32)
    if dim_t is not None:
        D = {min(int(t), int(length) - 1) for t in np.asarray(dim_t).reshape(-1) if int(t) >= 0}
        for j in range(f.shape[0]):
            f[j] = np.float32(0.5) ** ((j in D) + (j + 1 in D))
    with np.errstate(all="ignore"):
        c = np.trunc((np.asarray(color, dtype=np.float32)[None] * f[:, None]) * np.float32(255))
    return np.clip(np.nan_to_num(c, nan=0.0), 0, 255).astype(np.uint8)


def _paint_segment(img, a, b, color, thickness=TRAJ_THICKNESS):
    """the pixels of img [S, S, 3] within thickness / 2 of the segment a -> b (integer pixels), in Python integers"""
    S, g = img.shape[0], (thickness + 1) // 2
    ax, ay, bx, by = int(a[0]), int(a[1]), int(b[0]), int(b[1])
    xs, xe, ys, ye = max(min(ax, bx) - g, 0), min(max(ax, bx) + g + 1, S), max(min(ay, by) - g, 0), min(max(ay, by) + g + 1, S)
    if xs >= xe or ys >= ye:
        return
    qx, qy = np.arange(xs, xe, dtype=np.int64)[None, :], np.arange(ys, ye, dtype=np.int64)[:, None]
    dx, dy, wx, wy = bx - ax, by - ay, qx - ax, qy - ay
    dd, t, th2 = dx * dx + dy * dy, wx * dx + wy * dy, thickness * thickness
    near_a = 4 * (wx * wx + wy * wy) <= th2
    near_b = 4 * ((qx - bx) ** 2 + (qy - by) ** 2) <= th2
    cross = dx * wy - dy * wx
    cover = np.where(t <= 0, near_a, np.where(t >= dd, near_b, 4 * cross * cross <= th2 * dd))
    img[ys:ye, xs:xe][cover] = color


def _paint_stamp(img, stamp, color, px, py):
    k, S = stamp.shape[0], img.shape[0]
    x0, y0 = int(px) - k // 2, int(py) - k // 2
    xs, xe, ys, ye = max(x0, 0), min(x0 + k, S), max(y0, 0), min(y0 + k, S)
    if xs < xe and ys < ye:
        img[ys:ye, xs:xe][stamp[ys - y0:ye - y0, xs - x0:xe - x0]] = color


def render_trajectories_numpy(assets, layers):
    """uint8 [n, S, S, 3]: the definition of gcpx_topdown_trajectories.  assets: dataset.load_topdown_assets' dict.  layers: a list of
    dicts(states [n, P, 2], length [n] (= end_ind + 1), color (three floats), dim_t [n, K] or None).  Per canvas: the unpadded
    picture; then per layer the segments 0 .. m - 2 in order, the agent stamp on point 0, the goal stamp on point m - 1."""
    S, cw = assets["S"], assets["cw"]
    n = len(layers[0]["length"])
    out = np.repeat(assets["background"][None, cw:cw + S, cw:cw + S], n, axis=0).copy()
    for L in layers:
        states = np.asarray(L["states"], dtype=np.float32)
        for i in range(n):
            length = int(np.asarray(L["length"]).reshape(-1)[i])
            m = min(length, states.shape[1])
            if m < 1:
                continue
            pix, ok = trajectory_pixels(states[i, :m, :2], assets["n_rooms"], assets["scale"], S)
            dim_t = None if L.get("dim_t") is None else np.asarray(L["dim_t"])[i]
            col = segment_colors(L["color"], m, length, dim_t)
            for j in range(m - 1):
                if ok[j] and ok[j + 1]:
                    _paint_segment(out[i], pix[j], pix[j + 1], col[j])
            if ok[0]:
                _paint_stamp(out[i], assets["agent_stamp"], assets["agent_color"], *pix[0])
            if ok[m - 1]:
                _paint_stamp(out[i], assets["goal_stamp"], assets["goal_color"], *pix[m - 1])
    return out


# ---- the planner's verbose pictures (cem_planner.py:222-254) ---------------------------------------------------------------------------
TRAJ_MAX_LAYERS = 64          # GCPX_TRAJ_MAX_LAYERS: the trajectories one call of gcpx_topdown_trajectories draws onto a canvas


def plan_overview(res, horizon, n_elites):
    """ImageCEMPlanner.log_verbose's `plan_r{r}_iter{i}_overview` (cem_planner.py:228-242): the elites stacked top to bottom, each a
    row of `horizon` frames, values clip((x + 1) / 2, 0, 1).  Source: elites [n_elites, horizon, 3, res, res], every plan padded to
    `horizon` frames with ones (which the rescale leaves white) -- `pad_elites_numpy`."""
    p = Panel("plan_overview", 1, n_elites * res, horizon * res, 1.0)
    p.add(**_frames("elites", res, horizon, nb=n_elites, nf=horizon, r_b=res, c_f=res, flags=RESCALE))
    return p


def pad_elites_numpy(elites, horizon):
    """list of [len_e, 3, res, res] -> f32 [E, horizon, 3, res, res]: ones behind a shorter plan (cem_planner.py:232-233); a plan longer
    than `horizon` (a hierarchical plan of max_seq_len frames with the goal image appended) shows its first `horizon` frames, where
    the reference's reshape fails"""
    first = np.asarray(elites[0])
    out = np.ones((len(elites), horizon) + first.shape[1:], np.float32)
    for e, x in enumerate(elites):
        x = np.asarray(x, np.float32)[:horizon]
        out[e, :x.shape[0]] = x
    return out


def plan_overview_numpy(elites, horizon):
    """uint8 [E * res, horizon * res, 3]: the numpy mirror of the overview canvas"""
    padded = pad_elites_numpy(elites, horizon)
    panel = plan_overview(padded.shape[-1], horizon, padded.shape[0])
    return to_uint8(compose(panel, dict(elites=padded)))[0]


def trajectory_dist_layers(trajectories, color=RED):
    """log_multiple_topdown_trajs (logger.py:262-269) as layers of ONE canvas: every trajectory [len, >= 2] drawn in turn, its lines
    then its two stamps, onto what the previous one left -- which is the paint order of gcpx_topdown_trajectories' layers.  The first
    TRAJ_MAX_LAYERS trajectories are drawn."""
    return [dict(states=np.asarray(t, np.float32)[None, :, :2], length=np.array([len(t)]), color=color)
            for t in trajectories[:TRAJ_MAX_LAYERS] if len(t)]


def render_trajectory_dist_numpy(assets, trajectories, color=RED):
    """uint8 [S, S, 3]: the numpy mirror of `inferStateTrajDist`"""
    return render_trajectories_numpy(assets, trajectory_dist_layers(trajectories, color))[0]
