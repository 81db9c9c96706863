"""Nav dataset generator: the reference's data collection for the multiroom maze ("Generating navigation data with new layout",
README.md:145-152; experiments/data_gen/nav_16rooms/mod_hyper.py) -- a PrmPolicy expert walking a TopdownMultiroom3dEnv -- with the
probabilistic road map built on the device for a batch of independent trajectories (csrc/prm.hip, gcpx_prm_*).

Per trajectory, as PrmPolicy does it (prm_policy.py:130-190): start and goal from RoomSampler2d.sample(); one of the simple room paths
between their rooms, drawn uniformly (plan_room_seq_multimodal); sample points in the rooms and doors of that path; the road map and
the shortest path under cost d ** cost_power, with up to max_planning_retries fresh point sets; n_steps = min(int(length * 20), T)
with `length` from compute_shortest_path; the cubic spline through the path's vertices evaluated at linspace(0, 1, n_steps).  The
episode is recorded as Multiroom3dEnv.step and the HDF5 saver would: states [x, y, heading, goal_x, goal_y] in the environment's units
27 * (x, -y), actions = state differences and the zero action of the `done` step, pad_mask = get_pad_mask.

Three deviations:
  1. execution is ideal: the recorded states are the planned ones (MiniWorld's dynamics and heading smoothing are absent; heading is the
     direction of the step taken from a state);
  2. a trajectory whose planning fails in every retry, whose path has fewer than 4 vertices (splprep raises) or more than
     GCPX_PRM_MAX_PATH, or whose n_steps is below 2, is redrawn with a new start and goal (the reference records its one-step
     fallback episode, prm_policy.py:192-196);
  3. the random numbers are this build's own counter-based generator keyed (seed, trajectory index, draw index): np.random is not
     mirrored, and a trajectory does not depend on its batch-mates.

The numpy restatements below are the kernels' documentation and checkers (like dataset.assemble_numpy): sample_points_numpy,
prm_numpy (road map and path), spline_numpy, episode_numpy.  There is no host fallback: NavGenerator runs the kernels.
"""
import heapq
import math
import os

import numpy as np

from . import nav_layout as NL

PRM_MAX_NODES, PRM_MAX_KNN, PRM_MAX_PATH = 2048, 32, 1024      # include/gcpx.h
VAR_SAMPLING_RATES = (30, 300)                                  # PrmPolicy.VAR_SAMPLING_RATES
GRID_CELL_FACTOR = 1.25                                         # obstacle grid cell = 1.25 rr (> rr: the 3 x 3 cells cover radius rr)

# ---- the key table of PrmPolicy._default_hparams (prm_policy.py:44-64), with conf_loader.KEY_TABLE's discipline -----------------------
#   mapped   a NavGenerator parameter;  inert   cannot change what is generated;  unbuilt  {key: the reference's default}: any other
#   value raises.  A key in none of the three raises as unknown.
KEY_TABLE = {
    "mapped": {"n_samples_per_room": 50, "n_samples_per_door": 3, "n_knn": 10, "max_edge_len": 0.1, "max_planning_retries": 2,
               "cost_power": 2, "bottleneck_sampling": True, "use_var_sampling": False, "sample_door_center": False,
               "max_traj_length": None, "n_rooms": None},
    "inert": {"replan_eps": "execution is ideal: the agent never deviates from its plan, so nothing is replanned",
              "subsample_factor": "unused by the reference's _plan (prm_policy.py:173)",
              "use_fallback_plan": "a failed trajectory is redrawn instead (deviation 2)",
              "logger": "dummy variable", "type": "the policy class of a conf: PrmPolicy", "ncam": "no camera: frames are drawn top-down"},
    "unbuilt": {"use_scripted_path": False, "straight_through_door": False, "smooth_trajectory": False},
}


def screen_prm_params(params, where="NavGenerator"):
    """policy parameters -> the mapped ones over their defaults; raises on an unknown key or an unbuilt key off its default"""
    out = dict(KEY_TABLE["mapped"])
    for k, v in params.items():
        if k in KEY_TABLE["mapped"]:
            out[k] = v
        elif k in KEY_TABLE["unbuilt"]:
            if v != KEY_TABLE["unbuilt"][k]:
                raise ValueError(f"{where}: {k} = {v!r} is not built (only the reference's default {KEY_TABLE['unbuilt'][k]!r})")
        elif k not in KEY_TABLE["inert"]:
            raise ValueError(f"{where}: unknown PrmPolicy parameter {k!r}")
    return out


# ---- the counter-based generator ------------------------------------------------------------------------------------------------------
def mix64(z):
    """the splitmix64 output function on uint64 arrays (wrapping arithmetic)"""
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def uniform01(seed, key, ctr):
    """float64 in [0, 1): 53 bits of mix64(mix64(mix64(seed) ^ key) ^ ctr); key and ctr broadcast"""
    s = mix64(np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF))
    k = np.asarray(key).astype(np.int64).astype(np.uint64)
    c = np.asarray(ctr).astype(np.int64).astype(np.uint64)
    return (mix64(mix64(s ^ k) ^ c) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


HOST_CTR = 1 << 40          # the host's draws (start, goal, room path, sampling rates) use counters from here: the device's stay below


def sample_points_numpy(boxes, pt_box, key, draw0, seed):
    """gcpx_prm_sample_points for one trajectory: points (px, py) of the boxes pt_box, draws draw0, draw0 + 1, ..."""
    pt_box = np.asarray(pt_box, dtype=np.int64)
    draw = int(draw0) + np.arange(pt_box.shape[0], dtype=np.int64)
    b = np.asarray(boxes, dtype=np.float64)[pt_box]
    px = (uniform01(seed, key, 2 * draw) - 0.5) * b[:, 2] + b[:, 0]
    py = (uniform01(seed, key, 2 * draw + 1) - 0.5) * b[:, 3] + b[:, 1]
    return px, py


# ---- the obstacle grid ----------------------------------------------------------------------------------------------------------------
def obstacle_grid(ox, oy, rr):
    """the uniform grid gcpx_prm_roadmap reads: the cloud sorted by cell (row-major, cell = cy * gx + cx), cell_start int32
    [gx * gy + 1]; cell side GRID_CELL_FACTOR * rr"""
    ox, oy = np.asarray(ox, dtype=np.float64), np.asarray(oy, dtype=np.float64)
    cell = GRID_CELL_FACTOR * float(rr)
    x0, y0 = float(ox.min()), float(oy.min())
    cx, cy = np.floor((ox - x0) / cell).astype(np.int64), np.floor((oy - y0) / cell).astype(np.int64)
    gx, gy = int(cx.max()) + 1, int(cy.max()) + 1
    c = cy * gx + cx
    order = np.argsort(c, kind="stable")
    start = np.zeros(gx * gy + 1, dtype=np.int32)
    start[1:] = np.cumsum(np.bincount(c, minlength=gx * gy))
    return dict(ox=np.ascontiguousarray(ox[order]), oy=np.ascontiguousarray(oy[order]), cell_start=start, n_obs=int(ox.shape[0]),
                gx=gx, gy=gy, x0=x0, y0=y0, cell=cell)


def nearest_obstacle_grid_numpy(grid, x, y):
    """the kernel's nearest_obstacle for one query: the minimum over the 3 x 3 cells around it (inf when they are empty)"""
    fx, fy = math.floor((x - grid["x0"]) / grid["cell"]), math.floor((y - grid["y0"]) / grid["cell"])
    gx, gy = grid["gx"], grid["gy"]
    if not (-1 <= fx <= gx and -1 <= fy <= gy):
        return math.inf
    xa, xb = max(fx - 1, 0), min(fx + 1, gx - 1)
    best = math.inf
    if xb < xa:
        return best
    for yy in range(max(fy - 1, 0), min(fy + 1, gy - 1) + 1):
        s, e = grid["cell_start"][yy * gx + xa], grid["cell_start"][yy * gx + xb + 1]
        if e > s:
            dx, dy = grid["ox"][s:e] - x, grid["oy"][s:e] - y
            best = min(best, float((dx * dx + dy * dy).min()))
    return math.sqrt(best)


# ---- the road map and the path: prm.py in numpy -----------------------------------------------------------------------------------------
def nearest_obstacle_numpy(ox, oy, x, y):
    """distance from each query (x, y) to its nearest obstacle point: a brute-force scan"""
    x, y = np.atleast_1d(np.asarray(x, dtype=np.float64)), np.atleast_1d(np.asarray(y, dtype=np.float64))
    dx, dy = ox[None, :] - x[:, None], oy[None, :] - y[:, None]
    return np.sqrt((dx * dx + dy * dy).min(axis=1)) if ox.shape[0] else np.full(x.shape, np.inf)


def edges_collide_numpy(ox, oy, sx, sy, gx, gy, rr, max_edge_len):
    """is_collision (prm.py:96-122) from (sx, sy) to every (gx[k], gy[k]) -> bool [K]"""
    gx, gy = np.asarray(gx, dtype=np.float64), np.asarray(gy, dtype=np.float64)
    dx, dy = gx - sx, gy - sy
    d = np.sqrt(dx * dx + dy * dy)
    hit = d >= max_edge_len
    live = ~hit
    if not live.any():
        return hit
    # only obstacle points near the start can be within rr of a walk point or an end point
    reach = max_edge_len + 3 * rr
    near = (np.abs(ox - sx) <= reach) & (np.abs(oy - sy) <= reach)
    nox, noy = ox[near], oy[near]
    yaw = np.arctan2(dy, dx)
    nstep = np.rint(d / rr).astype(np.int64)                # Python's round: half to even
    ax, ay = rr * np.cos(yaw), rr * np.sin(yaw)
    x, y = np.full(d.shape, float(sx)), np.full(d.shape, float(sy))
    for i in range(int(nstep[live].max()) if live.any() else 0):
        walk = live & (i < nstep)
        if walk.any():
            hit[walk] |= nearest_obstacle_numpy(nox, noy, x[walk], y[walk]) <= rr
        x, y = x + ax, y + ay                               # accumulated, as the reference does it
    hit[live] |= nearest_obstacle_numpy(nox, noy, gx[live], gy[live]) <= rr
    return hit


def prm_numpy(px, py, sx, sy, gx, gy, ox, oy, rr, n_knn=10, max_edge_len=0.1, cost_power=2):
    """PRM_planning with `sampled_points` given (prm.py:82-93) -> dict: kept bool [n_pts]; x, y the node coordinates (kept samples in
    order, start, goal); road_map int32 [n, n_knn] (-1 past a list); success; path (vertex indices start .. goal, empty on failure);
    cost (inf on failure).  What gcpx_prm_roadmap and gcpx_prm_shortest_path compute."""
    px, py = np.asarray(px, dtype=np.float64), np.asarray(py, dtype=np.float64)
    ox, oy = np.asarray(ox, dtype=np.float64), np.asarray(oy, dtype=np.float64)
    kept = np.zeros(px.shape[0], dtype=bool)
    for s in range(0, px.shape[0], 256):
        kept[s:s + 256] = nearest_obstacle_numpy(ox, oy, px[s:s + 256], py[s:s + 256]) >= rr
    x = np.concatenate([px[kept], [sx, gx]])
    y = np.concatenate([py[kept], [sy, gy]])
    n = x.shape[0]
    road = np.full((n, n_knn), -1, dtype=np.int32)
    for i in range(n):
        dx, dy = x - x[i], y - y[i]
        d = np.sqrt(dx * dx + dy * dy)
        cand = np.flatnonzero((d < max_edge_len) & (np.arange(n) != i))
        cand = cand[np.lexsort((cand, d[cand]))]            # ascending distance, ties by index
        free = cand[~edges_collide_numpy(ox, oy, x[i], y[i], x[cand], y[cand], rr, max_edge_len)][:n_knn]
        road[i, :free.shape[0]] = free
    # dijkstra_planning (prm.py:162-226): node n - 2 -> node n - 1, costs summed from the start; equal cost: the lower predecessor
    cost = np.full(n, np.inf)
    pred = np.full(n, -1, dtype=np.int64)
    cost[n - 2] = 0.0
    heap, done = [(0.0, n - 2)], np.zeros(n, dtype=bool)
    while heap:
        c, i = heapq.heappop(heap)
        if done[i] or c > cost[i]:
            continue
        done[i] = True
        for j in road[i]:
            if j < 0:
                continue
            ddx, ddy = x[j] - x[i], y[j] - y[i]
            dd = math.sqrt(ddx * ddx + ddy * ddy)
            nc = c + (dd * dd if cost_power == 2 else dd ** cost_power)
            if nc < cost[j] or (nc == cost[j] and j != n - 2 and i < pred[j]):
                cost[j], pred[j] = nc, i
                heapq.heappush(heap, (nc, int(j)))
    success = bool(np.isfinite(cost[n - 1]))
    path = []
    if success:
        v = n - 1
        while v != -1:
            path.append(int(v))
            v = pred[v]
        path = path[::-1]
    return dict(kept=kept, x=x, y=y, road_map=road, success=success, path=np.array(path, dtype=np.int32),
                cost=float(cost[n - 1]))


def path_is_free_numpy(vx, vy, ox, oy, rr, max_edge_len):
    """every edge of the vertex path passes is_collision"""
    ox, oy = np.asarray(ox, dtype=np.float64), np.asarray(oy, dtype=np.float64)
    return not any(edges_collide_numpy(ox, oy, vx[k], vy[k], vx[k + 1:k + 2], vy[k + 1:k + 2], rr, max_edge_len)[0]
                   for k in range(len(vx) - 1))


# ---- resampling -------------------------------------------------------------------------------------------------------------------------
def spline_numpy(vx, vy, n_steps):
    """splprep([vx, vy], s=0) / splev(linspace(0, 1, n_steps)) (prm_policy.py:176-177) -> float64 [n_steps, 2]: the cubic spline that
    interpolates every vertex over the normalised cumulative chord length with not-a-knot ends (interior knots u[2:-2]); that spline
    is unique, so the second derivatives M of one tridiagonal solve per coordinate reproduce it.  What gcpx_prm_resample computes, in
    its order of operations.  Raises for fewer than 4 vertices or a repeated vertex, as splprep does."""
    v = np.stack([np.asarray(vx, dtype=np.float64), np.asarray(vy, dtype=np.float64)])
    m = v.shape[1]
    if m < 4:
        raise TypeError(f"m > k must hold: {m} vertices")
    h = np.sqrt(((v[:, 1:] - v[:, :-1]) ** 2).sum(axis=0))
    u = np.zeros(m)
    for k in range(1, m):
        u[k] = u[k - 1] + h[k - 1]
    if not (h > 0).all():
        raise ValueError("a repeated vertex")
    u[1:] = u[1:] / u[m - 1]
    M = np.zeros((2, m))
    for c in range(2):
        y = v[c]
        cp, prev_cp, prev_dp = np.zeros(m), 0.0, 0.0
        for i in range(1, m - 1):
            hl, hr = u[i] - u[i - 1], u[i + 1] - u[i]
            a, b, cc = hl, 2.0 * (hl + hr), hr
            if i == 1:
                a, b, cc = 0.0, 3.0 * hl + 2.0 * hr + hl * hl / hr, hr - hl * hl / hr
            if i == m - 2:
                a, b, cc = hl - hr * hr / hl, 3.0 * hr + 2.0 * hl + hr * hr / hl, 0.0
            r = 6.0 * ((y[i + 1] - y[i]) / hr - (y[i] - y[i - 1]) / hl)
            den = b - a * prev_cp
            prev_cp, prev_dp = cc / den, (r - a * prev_dp) / den
            cp[i], M[c, i] = prev_cp, prev_dp
        for i in range(m - 3, 0, -1):
            M[c, i] = M[c, i] - cp[i] * M[c, i + 1]
        h0, h1, hL, hp = u[1] - u[0], u[2] - u[1], u[m - 1] - u[m - 2], u[m - 2] - u[m - 3]
        M[c, 0] = (1.0 + h0 / h1) * M[c, 1] - (h0 / h1) * M[c, 2]
        M[c, m - 1] = (1.0 + hL / hp) * M[c, m - 2] - (hL / hp) * M[c, m - 3]
    t = np.linspace(0, 1, n_steps)
    lo = np.clip(np.searchsorted(u, t, side="right") - 1, 0, m - 2)
    hh, A, B = u[lo + 1] - u[lo], u[lo + 1] - t, t - u[lo]
    out = np.empty((n_steps, 2))
    for c in range(2):
        Ml, Mr, yl, yr = M[c, lo], M[c, lo + 1], v[c, lo], v[c, lo + 1]
        out[:, c] = Ml * (A * A * A) / (6.0 * hh) + Mr * (B * B * B) / (6.0 * hh) + (yl / hh - Ml * hh / 6.0) * A + (yr / hh - Mr * hh / 6.0) * B
    return out


def n_steps_for(length, T):
    """prm_policy.py:173: min(int(length * 20), max_traj_length - t) at t = 0"""
    return min(int(length * 20), int(T))


def get_pad_mask(action_len, max_num_actions):
    """hdf5_saver.py:39-53"""
    if action_len > max_num_actions:
        raise ValueError
    return np.concatenate([np.ones(action_len + 1), np.zeros(max_num_actions - action_len)])


def episode_numpy(plan, goal, T):
    """the recorded episode of an ideally executed plan (float64 [ns, 2], planner's units; goal (gx, gy)) -> states f32 [T + 1, 5],
    actions f32 [T, 2], pad_mask f32 [T + 1]: what gcpx_prm_resample writes beside the plan"""
    plan = np.asarray(plan, dtype=np.float64)
    ns = plan.shape[0]
    assert 2 <= ns <= T
    env = np.stack([plan[:, 0] * 27.0, (plan[:, 1] * -1.0) * 27.0], axis=1)          # prm2env: 27 (x, -y)
    diff = env[1:] - env[:-1]                                                         # transform_plan, multiroom3d_env.py:141-144
    states, actions = np.zeros((T + 1, 5), dtype=np.float32), np.zeros((T, 2), dtype=np.float32)
    actions[:ns - 1] = diff                                                           # then the zero action of the `done` step
    states[:ns, :2] = env
    states[ns, :2] = env[-1]
    head = np.arctan2(diff[:, 1], diff[:, 0])
    states[:ns - 1, 2] = head
    states[ns - 1:ns + 1, 2] = head[-1]
    states[:ns + 1, 3] = np.float32(goal[0] * 27.0)
    states[:ns + 1, 4] = np.float32((goal[1] * -1.0) * 27.0)
    return states, actions, get_pad_mask(ns, T).astype(np.float32)


# ---- the top-down assets without textures ---------------------------------------------------------------------------------------------
# a flat colour per room (this build's own palette: light, so that the black walls and the blue / green dots stay visible)
PALETTE = np.array([(255, 224, 224), (224, 255, 224), (224, 224, 255), (255, 255, 208), (255, 224, 255), (208, 255, 255),
                    (255, 236, 208), (224, 240, 224), (236, 224, 255), (240, 240, 240), (255, 208, 224), (208, 236, 255),
                    (236, 255, 208)], dtype=np.uint8)
RENDER_SCALE = 256            # Multiroom3dEnv._topdown_render_scale
STAMP_K, STAMP_RADIUS = 11, 5
AGENT_COLOR, GOAL_COLOR = (0, 0, 255), (0, 255, 0)


def _thick_line(img, p, q, half=1):
    """an axis-parallel black line of thickness 2 * half + 1 from pixel p to pixel q (x, y), with one cap pixel past each end on the
    centre line; clipped to the picture.  The footprint of cv2.line(..., thickness=3) is inferred, not pinned (OpenCV is absent)."""
    S = img.shape[0]
    (x0, y0), (x1, y1) = p, q
    xa, xb, ya, yb = min(x0, x1), max(x0, x1), min(y0, y1), max(y0, y1)
    horizontal = ya == yb
    rx0, rx1 = (xa, xb) if horizontal else (xa - half, xb + half)
    ry0, ry1 = (ya - half, yb + half) if horizontal else (ya, yb)
    img[max(ry0, 0):max(min(ry1 + 1, S), 0), max(rx0, 0):max(min(rx1 + 1, S), 0)] = 0
    caps = ((xa - 1, ya), (xb + 1, ya)) if horizontal else ((xa, ya - 1), (xa, yb + 1))
    for cx, cy in caps:
        if 0 <= cx < S and 0 <= cy < S:
            img[cy, cx] = 0


def draw_layout_picture(n_rooms, crop_window=40, plain=False, render_scale=RENDER_SCALE):
    """draw_layout_overview(add_textures=False) (multiroom2d_layout.py:265-294) padded by crop_window (multiroom3d_env.py:33-38), as uint8:
    a white int(table_size * render_scale)-square with the walls as black 3-pixel lines at the reference's pixel positions, on a zero
    border.  Unless `plain`, every room is first filled with a flat colour of PALETTE (where the reference pastes its texture)."""
    rps = NL.rooms_per_side_of(n_rooms)
    table = NL.ROOM_SIZE * rps
    res = int(table * render_scale)
    room = int(res / rps)
    img = np.full((res, res, 3), 255, dtype=np.uint8)
    if not plain:
        for x in range(rps):
            for y in range(rps):
                img[y * room:(y + 1) * room, x * room:(x + 1) * room] = PALETTE[(x * rps + y) % len(PALETTE)]
    for kind, (lo, hi), at in NL.wall_segments(rps):
        if kind == "h":
            yy = res - int(at * render_scale - 1)
            _thick_line(img, (int(lo * render_scale), yy), (int(hi * render_scale), yy))
        else:
            xx = int(at * render_scale)
            _thick_line(img, (xx, res - int(lo * render_scale - 1)), (xx, res - int(hi * render_scale - 1)))
    cw = int(crop_window)
    out = np.zeros((res + 2 * cw, res + 2 * cw, 3), dtype=np.uint8)
    out[cw:cw + res, cw:cw + res] = img
    return out


def disc_stamp(k=STAMP_K, radius=STAMP_RADIUS):
    """a filled disc: what the renderer's degenerate line cv2.line(img, p, p, colour, 10) leaves (inferred, not pinned)"""
    c = np.arange(k) - k // 2
    return (c[:, None] ** 2 + c[None, :] ** 2) <= radius * radius


def topdown_assets(n_rooms, crop_window=40, plain=False):
    """the arrays of `topdown_assets.npz` ('Top-down assets')"""
    stamp = disc_stamp()
    return dict(background=draw_layout_picture(n_rooms, crop_window, plain), crop_window=np.int64(crop_window), n_rooms=np.int64(n_rooms),
                render_scale=np.int64(RENDER_SCALE), agent_stamp=stamp, goal_stamp=stamp.copy(),
                agent_color=np.array(AGENT_COLOR, dtype=np.uint8), goal_color=np.array(GOAL_COLOR, dtype=np.uint8))


# ---- the generator ----------------------------------------------------------------------------------------------------------------------
class NavGenerator:
    """NavGenerator(n_rooms, T=100, seed=0, **prm_params): prm_params are PrmPolicy's (KEY_TABLE).  generate(n) -> device tensors."""

    CHUNK = 512               # trajectories per launch: bounds the adjacency buffer (CHUNK * cap * n_knn int32)
    MAX_REDRAWS = 64

    def __init__(self, n_rooms, T=100, seed=0, device="cuda:0", start_index=0, **prm_params):
        import torch
        from . import runtime as rt
        hp = screen_prm_params(dict(prm_params, n_rooms=n_rooms))
        self.n_rooms, self.T, self.seed, self.start_index = int(n_rooms), int(T), int(seed), int(start_index)
        if hp["max_traj_length"] not in (None, self.T):
            raise ValueError(f"max_traj_length = {hp['max_traj_length']}: the data collection plans for the agent's T = {self.T}")
        self.rps = NL.rooms_per_side_of(self.n_rooms)
        self.layout, self.boxes = NL.layout(self.rps), NL.RoomBoxes(self.rps, sample_wide=False)
        self.hp = hp
        self.n_knn, self.max_edge_len, self.cost_power = int(hp["n_knn"]), float(hp["max_edge_len"]), float(hp["cost_power"])
        self.retries = int(hp["max_planning_retries"])
        if not 1 <= self.n_knn <= PRM_MAX_KNN or self.retries < 1 or not 2 <= self.T <= PRM_MAX_PATH:
            raise ValueError("n_knn: 1 .. 32, max_planning_retries >= 1, T: 2 .. 1024")
        self.device, self.lib, self.rt, self.torch = torch.device(device), rt.load_library(), rt, torch
        self.box_table = self.boxes.box_table(self.layout.doors)
        self._door_box = {tuple(d): self.n_rooms + k for k, d in enumerate(self.layout.doors)}
        self.grid = obstacle_grid(self.layout.ox, self.layout.oy, self.layout.robot_size)
        self._tables = None

    @property
    def _dev(self):
        """the layout's tables on the device (the sorted cloud, the grid, the boxes): uploaded once, at the first launch"""
        if self._tables is None:
            g = self.grid
            dev = lambda a: self.torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
            self._tables = dict(ox=dev(g["ox"]), oy=dev(g["oy"]), cell_start=dev(g["cell_start"]), boxes=dev(self.box_table))
        return self._tables

    # -- host bookkeeping: the draws that pick rooms, and the point tables --
    def _u(self, key, k):
        return float(uniform01(self.seed, key, HOST_CTR + k))

    def draw_task(self, index, redraw):
        """start, goal, room path and n_steps of trajectory `index` at its `redraw`-th drawing (host draws 0 .. 5)"""
        key = index * 256 + redraw
        rooms = [min(int(self._u(key, 3 * e) * self.n_rooms), self.n_rooms - 1) for e in range(2)]      # np.random.randint(n_rooms)
        pts = []
        for e, room in enumerate(rooms):                    # RoomSampler2d.sample(): _rand(2) * width + centre
            c = self.box_table[room]
            pts += [(self._u(key, 3 * e + 1) - 0.5) * c[2] + c[0], (self._u(key, 3 * e + 2) - 0.5) * c[3] + c[1]]
        paths = NL.room_paths(self.rps, rooms[0], rooms[1])
        path = paths[min(int(self._u(key, 6) * len(paths)), len(paths) - 1)]                             # np.random.choice(goal_nodes)
        length, _ = NL.compute_shortest_path(self.rps, pts[:2], pts[2:])
        return dict(index=index, key=key, start_goal=pts, room_path=path, n_steps=n_steps_for(length, self.T))

    def point_boxes(self, task, retry):
        """the box of every sample point of one planning attempt (PrmPolicy._sample_points with the room path)"""
        hp, path = self.hp, task["room_path"]
        out = []
        for k, room in enumerate(path):
            n = hp["n_samples_per_room"]
            if hp["use_var_sampling"]:                      # np.random.choice(VAR_SAMPLING_RATES) per room and attempt
                n = VAR_SAMPLING_RATES[min(int(self._u(task["key"], 16 + retry * 64 + k) * 2), 1)]
            out += [room] * int(n)
        if hp["bottleneck_sampling"]:
            off = len(self.layout.doors) if hp["sample_door_center"] else 0
            for a, b in zip(path[:-1], path[1:]):
                out += [self._door_box[(min(a, b), max(a, b))] + off] * int(hp["n_samples_per_door"])
        if len(out) + 2 > PRM_MAX_NODES:
            raise ValueError(f"{len(out)} sample points for one trajectory: at most {PRM_MAX_NODES - 2} nodes fit the kernel")
        return out

    # -- the device pipeline --
    def plan_batch(self, tasks, retry):
        """one planning attempt for a list of tasks -> dict of device tensors (points, kept, n_nodes, node_xy, adj, success, n_vert,
        path, cost) and the sizes; four launches, no synchronisation"""
        torch, rt, lib, d = self.torch, self.rt, self.lib, self._dev
        B = len(tasks)
        tabs = [self.point_boxes(t, retry) for t in tasks]
        off = np.zeros(B + 1, dtype=np.int32)
        off[1:] = np.cumsum([len(t) for t in tabs])
        total, max_pts = int(off[-1]), max(len(t) for t in tabs)
        cap = max_pts + 2
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
        pt_box, pt_off = dev(np.concatenate(tabs).astype(np.int32)), dev(off)
        key = dev(np.array([t["key"] for t in tasks], dtype=np.int64))
        draw0 = dev(np.full(B, retry * PRM_MAX_NODES, dtype=np.int32))
        sg = dev(np.array([t["start_goal"] for t in tasks], dtype=np.float64))
        o = dict(B=B, cap=cap, total=total, max_pts=max_pts, pt_off=pt_off, start_goal=sg)
        f64 = dict(dtype=torch.float64, device=self.device)
        i32 = dict(dtype=torch.int32, device=self.device)
        o["px"], o["py"] = torch.empty(total, **f64), torch.empty(total, **f64)
        s = rt.current_stream()
        rt.check(lib.gcpx_prm_sample_points(d["boxes"].data_ptr(), self.box_table.shape[0], pt_box.data_ptr(), pt_off.data_ptr(),
                                            key.data_ptr(), draw0.data_ptr(), B, total, max_pts, self.seed, o["px"].data_ptr(),
                                            o["py"].data_ptr(), s), "prm_sample_points")
        self.roadmap_into(o, s)
        self.path_into(o, s)
        return o

    def roadmap_into(self, o, stream):
        torch, g, d = self.torch, self.grid, self._dev
        B, cap = o["B"], o["cap"]
        o["kept"] = torch.zeros(o["total"], dtype=torch.uint8, device=self.device)
        o["n_nodes"] = torch.zeros(B, dtype=torch.int32, device=self.device)
        o["node_xy"] = torch.zeros(B, 2, cap, dtype=torch.float64, device=self.device)
        o["adj"] = torch.full((B, cap, self.n_knn), -1, dtype=torch.int32, device=self.device)
        self.rt.check(self.lib.gcpx_prm_roadmap(d["ox"].data_ptr(), d["oy"].data_ptr(), d["cell_start"].data_ptr(), g["n_obs"], g["gx"],
                                                g["gy"], g["x0"], g["y0"], g["cell"], o["px"].data_ptr(), o["py"].data_ptr(),
                                                o["pt_off"].data_ptr(), o["start_goal"].data_ptr(), B, o["total"], o["max_pts"], cap,
                                                self.n_knn, self.layout.robot_size, self.max_edge_len, o["kept"].data_ptr(),
                                                o["n_nodes"].data_ptr(), o["node_xy"].data_ptr(), o["adj"].data_ptr(), stream),
                      "prm_roadmap")

    def path_into(self, o, stream):
        torch = self.torch
        B, cap = o["B"], o["cap"]
        o["success"] = torch.zeros(B, dtype=torch.int32, device=self.device)
        o["n_vert"] = torch.zeros(B, dtype=torch.int32, device=self.device)
        o["path"] = torch.full((B, cap), -1, dtype=torch.int32, device=self.device)
        o["cost"] = torch.full((B,), float("inf"), dtype=torch.float64, device=self.device)
        self.rt.check(self.lib.gcpx_prm_shortest_path(o["node_xy"].data_ptr(), o["n_nodes"].data_ptr(), o["adj"].data_ptr(), B, cap,
                                                      self.n_knn, self.cost_power, o["success"].data_ptr(), o["n_vert"].data_ptr(),
                                                      o["path"].data_ptr(), o["cost"].data_ptr(), stream), "prm_shortest_path")

    def resample_into(self, o, n_steps, stream):
        torch, T = self.torch, self.T
        B, cap = o["B"], o["cap"]
        o["n_steps"] = torch.from_numpy(np.asarray(n_steps, dtype=np.int32)).to(self.device)
        o["plan"] = torch.zeros(B, T, 2, dtype=torch.float64, device=self.device)
        o["ok"] = torch.zeros(B, dtype=torch.int32, device=self.device)
        o["states"] = torch.zeros(B, T + 1, 5, dtype=torch.float32, device=self.device)
        o["actions"] = torch.zeros(B, T, 2, dtype=torch.float32, device=self.device)
        o["pad_mask"] = torch.zeros(B, T + 1, dtype=torch.float32, device=self.device)
        self.rt.check(self.lib.gcpx_prm_resample(o["node_xy"].data_ptr(), o["n_nodes"].data_ptr(), o["path"].data_ptr(),
                                                 o["n_vert"].data_ptr(), o["n_steps"].data_ptr(), o["start_goal"].data_ptr(), B, cap, T,
                                                 o["plan"].data_ptr(), o["ok"].data_ptr(), o["states"].data_ptr(),
                                                 o["actions"].data_ptr(), o["pad_mask"].data_ptr(), stream), "prm_resample")

    def generate(self, n, keep_paths=False):
        """n trajectories (indices start_index .. start_index + n - 1) -> dict of device tensors: states f32 [n, T + 1, 5], actions f32
        [n, T, 2], pad_mask f32 [n, T + 1], n_steps int32 [n], start_goal f64 [n, 4] (planner's units), redraws int32 [n]; with
        keep_paths also path_xy f64 [n, PRM_MAX_PATH, 2] and n_vert int32 [n] (the road-map vertices behind each plan)."""
        torch, T = self.torch, self.T
        res = dict(states=torch.zeros(n, T + 1, 5, dtype=torch.float32, device=self.device),
                   actions=torch.zeros(n, T, 2, dtype=torch.float32, device=self.device),
                   pad_mask=torch.zeros(n, T + 1, dtype=torch.float32, device=self.device),
                   n_steps=torch.zeros(n, dtype=torch.int32, device=self.device),
                   start_goal=torch.zeros(n, 4, dtype=torch.float64, device=self.device),
                   redraws=torch.zeros(n, dtype=torch.int32, device=self.device))
        if keep_paths:
            res["path_xy"] = torch.zeros(n, PRM_MAX_PATH, 2, dtype=torch.float64, device=self.device)
            res["n_vert"] = torch.zeros(n, dtype=torch.int32, device=self.device)
        redraw = np.zeros(n, dtype=np.int64)
        todo = list(range(n))

        def draw_again(slot):
            redraw[slot] += 1
            if redraw[slot] >= self.MAX_REDRAWS:
                raise RuntimeError(f"trajectory {self.start_index + slot}: no plan in {self.MAX_REDRAWS} drawings of start and goal")

        while todo:
            chunk, todo = todo[:self.CHUNK], todo[self.CHUNK:]
            tasks = []
            for slot in chunk:
                t = self.draw_task(self.start_index + slot, int(redraw[slot]))
                while t["n_steps"] < 2:                      # a plan of fewer than 2 states: drawn again at once
                    draw_again(slot)
                    t = self.draw_task(self.start_index + slot, int(redraw[slot]))
                t["slot"] = slot
                tasks.append(t)
            for retry in range(self.retries):
                if not tasks:
                    break
                o = self.plan_batch(tasks, retry)
                self.resample_into(o, [t["n_steps"] for t in tasks], self.rt.current_stream())
                found, good = o["success"].bool(), o["success"].bool() & o["ok"].bool()
                idx = torch.nonzero(good).flatten()
                slots = np.array([t["slot"] for t in tasks], dtype=np.int64)
                dst = torch.from_numpy(slots).to(self.device)[idx]
                for k in ("states", "actions", "pad_mask", "n_steps", "start_goal"):
                    res[k][dst] = o[k][idx]
                res["redraws"][dst] = torch.from_numpy(redraw[slots].astype(np.int32)).to(self.device)[idx]
                if keep_paths:
                    m = min(o["cap"], PRM_MAX_PATH)
                    pidx = o["path"][idx, :m].clamp(min=0).long()
                    xy = torch.stack([torch.gather(o["node_xy"][idx, 0], 1, pidx), torch.gather(o["node_xy"][idx, 1], 1, pidx)], dim=2)
                    live = (torch.arange(m, device=self.device)[None, :] < o["n_vert"][idx, None]).unsqueeze(2)
                    res["path_xy"][dst, :m] = xy * live
                    res["n_vert"][dst] = o["n_vert"][idx]
                state = torch.stack([found, good]).cpu().numpy()          # the one synchronisation of an attempt: who needs another
                again = []
                for t, f, g_ in zip(tasks, state[0], state[1]):
                    if not f:
                        again.append(t)                     # no path: fresh points for the same start and goal
                    elif not g_:                            # a path that cannot be resampled (fewer than 4 vertices): new start and goal
                        draw_again(t["slot"])
                        todo.append(t["slot"])
                tasks = again
            for t in tasks:                                 # no path in any retry
                draw_again(t["slot"])
                todo.append(t["slot"])
        return res


# ---- writing a dataset ------------------------------------------------------------------------------------------------------------------
_SPEC_CLASS = {9: ("gcp.datasets.configs.nav_9rooms", "Nav9Rooms"), 25: ("gcp.datasets.configs.nav_25rooms", "Nav25Rooms")}
_SPEC_DEFAULT = ("gcp.datasets.data_loader", "MazeTopRenderedGlobalSplitVarLenVideoDataset")
_SPEC_TEMPLATE = """from blox import AttrDict
from {module} import {cls}

dataset_spec = AttrDict(
    max_seq_len={T},
    dataset_class={cls},
    split=AttrDict(train={train}, val={val}, test={test}),
)
"""


def write_dataset(root, n, n_rooms=9, T=100, seed=0, traj_per_file=1, split=(0.9, 0.05, 0.05), crop_window=40, plain=False, start_index=0,
                  device="cuda:0", generator=None, **prm_params):
    """Write the GlobalSplit `.npz` tree dataset.py reads (no `images`: the nav datasets draw their frames from the states), its
    `dataset_spec.py` and `topdown_assets.npz` into `root`.  File f holds trajectories [f * traj_per_file, (f + 1) * traj_per_file) as
    traj{i}/states f32 [n_steps + 1, 5], traj{i}/actions f32 [T, 2], traj{i}/pad_mask f32 [T + 1] (as the reference's saver pads
    them).  Returns the generator's result (device tensors)."""
    if n % traj_per_file:
        raise ValueError(f"n = {n} is not a multiple of traj_per_file = {traj_per_file}")
    gen = generator or NavGenerator(n_rooms, T=T, seed=seed, device=device, start_index=start_index, **prm_params)
    res = gen.generate(n)
    st, ac, pm, ns = (res[k].cpu().numpy() for k in ("states", "actions", "pad_mask", "n_steps"))
    os.makedirs(os.path.join(root, "hdf5"), exist_ok=True)
    for f in range(n // traj_per_file):
        arrays = {"traj_per_file": np.int64(traj_per_file)}
        for i in range(traj_per_file):
            j = f * traj_per_file + i
            arrays[f"traj{i}/states"] = st[j, :ns[j] + 1]
            arrays[f"traj{i}/actions"] = ac[j]
            arrays[f"traj{i}/pad_mask"] = pm[j]
        np.savez(os.path.join(root, "hdf5", f"traj_{start_index + f * traj_per_file:06d}_to_{start_index + (f + 1) * traj_per_file - 1:06d}.npz"),
                 **arrays)
    write_spec_and_assets(root, gen.n_rooms, gen.T, split, crop_window, plain)
    return res


def write_spec_and_assets(root, n_rooms, T, split=(0.9, 0.05, 0.05), crop_window=40, plain=False):
    os.makedirs(root, exist_ok=True)
    module, cls = _SPEC_CLASS.get(int(n_rooms), _SPEC_DEFAULT)
    with open(os.path.join(root, "dataset_spec.py"), "w") as f:
        f.write(_SPEC_TEMPLATE.format(module=module, cls=cls, T=int(T), train=split[0], val=split[1], test=split[2]))
    np.savez(os.path.join(root, "topdown_assets.npz"), **topdown_assets(n_rooms, crop_window, plain))


def experiment_settings(conf):
    """the values gen_nav --experiment reads from a data-collection conf (`config` of a mod_hyper.py, as a plain dict): n_rooms,
    crop_window, T, start_index / end_index, traj_per_file and the policy's parameters"""
    agent = conf["agent"]
    env_params = agent["env"][1] if isinstance(agent["env"], (list, tuple)) else agent["env"]
    policy = {k: v for k, v in dict(conf["policy"]).items() if k != "type"}
    return dict(n_rooms=int(env_params.get("n_rooms", 9)), crop_window=int(env_params.get("crop_window") or 40), T=int(agent["T"]),
                start_index=int(conf.get("start_index", 0)), end_index=int(conf["end_index"]),
                traj_per_file=int(conf.get("traj_per_file", 1)), policy=policy)
