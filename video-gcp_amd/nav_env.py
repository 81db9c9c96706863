"""The maze environment of the control experiments, batched: E independent episodes advanced together on the device, one launch per
step (csrc/nav_env.hip, gcpx_nav_env_*), observed through the nav datasets' top-down renderer (gcpx_topdown_assemble_batch, one frame per
episode).  The batched counterpart of TopdownMultiroom3dEnv as BenchmarkAgent drives it (gcp/planning/infra/agent/general_agent.py:
`env.step`, a render, `policy.act`, one episode at a time on the host) and of BaseMiniworldEnv.eval (base_miniworld_env.py:29-40).

gym-miniworld is absent, so the dynamics are this build's own ('Control experiments'):
  state      (x, y, heading) float32 in the environment's units, 27 * (x, -y) of the layout's table coordinates
  proposal   p' = p + a, one float32 add per coordinate
  blocked    iff the closed segment [p, p'] comes within ROBOT_SIZE of a wall segment (float64, table coordinates); a blocked move is
             rejected whole: position and heading stay
  free       heading = atan2 of the step (the generator's convention, nav_gen.episode_numpy); a zero action is free and keeps the heading
  goal dist  PrmPolicy.compute_shortest_path (nav_layout.compute_shortest_path) from a per-episode table built at reset

The numpy restatements are the kernels' documentation and the tests' reference (like nav_gen.prm_numpy): wall_table, goal_table,
goal_dist_numpy, step_numpy.  There is no host fallback: NavEnvBatch runs the kernels."""
import math

import numpy as np

from . import nav_layout as NL

UNITS = 27.0                  # environment units per table unit (multiroom3d_env.py:196-199)


def env2table(xy):
    """environment units -> table coordinates, float64: (x / 27, -(y / 27))"""
    xy = np.asarray(xy, dtype=np.float64)
    return np.stack([xy[..., 0] / UNITS, (xy[..., 1] / UNITS) * -1.0], axis=-1)


def table2env(xy):
    """table coordinates -> environment units, float32: 27 * (x, -y) as nav_gen.episode_numpy has it"""
    xy = np.asarray(xy, dtype=np.float64)
    return np.stack([xy[..., 0] * UNITS, (xy[..., 1] * -1.0) * UNITS], axis=-1).astype(np.float32)


def wall_table(rooms_per_side):
    """float64 [n_walls, 4] = (x0, y0, x1, y1): nav_layout.wall_segments centred on (0, 0), as Layout centres its cloud"""
    off = 0.5 * rooms_per_side * NL.ROOM_SIZE
    rows = [(lo - off, at - off, hi - off, at - off) if kind == "h" else (at - off, lo - off, at - off, hi - off)
            for kind, (lo, hi), at in NL.wall_segments(rooms_per_side)]
    return np.ascontiguousarray(np.array(rows, dtype=np.float64))


def _room_of(rooms_per_side, x, y):
    """Layout.coords2ridx with the room coordinates clamped into the layout"""
    table = NL.ROOM_SIZE * rooms_per_side
    xr = min(max(math.floor((x + table / 2) / NL.ROOM_SIZE), 0), rooms_per_side - 1)
    yr = min(max(math.floor((y + table / 2) / NL.ROOM_SIZE), 0), rooms_per_side - 1)
    return int(xr) * rooms_per_side + (rooms_per_side - 1) - int(yr)


def goal_table(rooms_per_side, goal):
    """float64 [n_rooms, 3] for one goal (table coordinates): row r = (x, y of the first door centre of plan_room_seq(r, goal room), the
    length from that door over the remaining door centres to the goal); the goal room's row = (goal x, goal y, -1); every third entry
    is NaN when a coordinate of the goal lies outside [-0.5, 0.5] (compute_shortest_path then answers 10 whatever the position)"""
    g = np.asarray(goal, dtype=np.float64)
    n_rooms = rooms_per_side * rooms_per_side
    tab = np.zeros((n_rooms, 3), dtype=np.float64)
    if (g < -0.5).any() or (g > 0.5).any():
        tab[:, 2] = np.nan
        return tab
    L, boxes = NL.layout(rooms_per_side), NL.RoomBoxes(rooms_per_side)
    groom = _room_of(rooms_per_side, g[0], g[1])
    for r in range(n_rooms):
        if r == groom:
            tab[r] = (g[0], g[1], -1.0)
            continue
        rooms = NL.plan_room_seq(r, groom, L.doors)
        way = np.array([boxes.get_door_pos(min(a, b), max(a, b)) for a, b in zip(rooms[:-1], rooms[1:])] + [g])
        rest = 0.0
        for k in range(len(way) - 1):
            dx, dy = way[k + 1, 0] - way[k, 0], way[k + 1, 1] - way[k, 1]
            rest += math.sqrt(dx * dx + dy * dy)
        tab[r] = (way[0, 0], way[0, 1], rest)
    return tab


def goal_dist_numpy(rooms_per_side, p, table):
    """the kernels' goal distance of one position p (table coordinates) under a goal_table: 10 outside [-0.5, 0.5] (position or goal),
    else |p - (row x, y)| + max(row rest, 0) of the position's room"""
    x, y = float(p[0]), float(p[1])
    if not (-0.5 <= x <= 0.5 and -0.5 <= y <= 0.5):
        return 10.0
    row = table[_room_of(rooms_per_side, x, y)]
    if row[2] != row[2]:
        return 10.0
    dx, dy = x - row[0], y - row[1]
    d = math.sqrt(dx * dx + dy * dy)
    return d if row[2] < 0 else d + row[2]


def _point_segment_d2(qx, qy, ax, ay, bx, by):
    dx, dy = bx - ax, by - ay
    l2 = dx * dx + dy * dy
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(l2 > 0, np.minimum(np.maximum(((qx - ax) * dx + (qy - ay) * dy) / l2, 0.0), 1.0), 0.0)
    ex, ey = qx - (ax + t * dx), qy - (ay + t * dy)
    return ex * ex + ey * ey


def segment_walls_d2(p, q, walls):
    """squared distance from the closed segment [p, q] to every wall segment, float64 [n_walls]: 0 where they cross properly (both
    orientation tests strictly of opposite sign), else the least of the four end-point-to-segment distances; in the kernel's order of
    operations"""
    px, py, qx, qy = float(p[0]), float(p[1]), float(q[0]), float(q[1])
    ax, ay, bx, by = (np.asarray(walls, dtype=np.float64)[:, k] for k in range(4))
    ux, uy, vx, vy = qx - px, qy - py, bx - ax, by - ay
    o1, o2 = ux * (ay - py) - uy * (ax - px), ux * (by - py) - uy * (bx - px)
    o3, o4 = vx * (py - ay) - vy * (px - ax), vx * (qy - ay) - vy * (qx - ax)
    cross = (((o1 > 0) & (o2 < 0)) | ((o1 < 0) & (o2 > 0))) & (((o3 > 0) & (o4 < 0)) | ((o3 < 0) & (o4 > 0)))
    d = np.minimum(np.minimum(_point_segment_d2(px, py, ax, ay, bx, by), _point_segment_d2(qx, qy, ax, ay, bx, by)),
                   np.minimum(_point_segment_d2(ax, ay, px, py, qx, qy), _point_segment_d2(bx, by, px, py, qx, qy)))
    return np.where(cross, 0.0, d)


def step_numpy(state, action, walls, radius=NL.ROBOT_SIZE):
    """gcpx_nav_env_step for one episode: state float32 [3], action float32 [2] -> dict(state float32 [3], blocked bool, step_len
    float64 (environment units, 0 when blocked), clearance float64: the least distance from [p, p'] to a wall, inf for a zero action)"""
    s, a = np.asarray(state, dtype=np.float32), np.asarray(action, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        new = (s[:2] + a).astype(np.float32)                  # one float32 add per coordinate
    if a[0] == 0 and a[1] == 0:
        return dict(state=s.copy(), blocked=False, step_len=0.0, clearance=math.inf)
    blocked, clearance = not np.isfinite(new).all(), math.nan
    if not blocked:
        d2 = segment_walls_d2(env2table(s[:2]), env2table(new), walls)
        blocked = bool((~(d2 > radius * radius)).any())
        clearance = float(np.sqrt(d2.min()))
    if blocked:
        return dict(state=s.copy(), blocked=True, step_len=0.0, clearance=clearance)
    dx, dy = float(new[0]) - float(s[0]), float(new[1]) - float(s[1])
    out = np.array([new[0], new[1], np.float32(math.atan2(dy, dx))], dtype=np.float32)
    return dict(state=out, blocked=False, step_len=math.sqrt(dx * dx + dy * dy), clearance=clearance)


def rollout_numpy(n_rooms, start, goal, actions):
    """one episode through step_numpy: start float32 [3], goal [2] (environment units), actions [T, 2] -> dict(full_traj float32
    [T + 1, 3], blocked bool [T], path_len, goal_dist float64 [T + 1], clearance float64 [T])"""
    rps = NL.rooms_per_side_of(n_rooms)
    walls, tab = wall_table(rps), goal_table(rps, env2table(np.asarray(goal, dtype=np.float32)))
    T = len(actions)
    traj, blocked, clear = np.zeros((T + 1, 3), dtype=np.float32), np.zeros(T, dtype=bool), np.zeros(T)
    dist, path_len = np.zeros(T + 1), 0.0
    traj[0] = np.asarray(start, dtype=np.float32)
    dist[0] = goal_dist_numpy(rps, env2table(traj[0, :2]), tab)
    for t in range(T):
        r = step_numpy(traj[t], actions[t], walls)
        traj[t + 1], blocked[t], clear[t] = r["state"], r["blocked"], r["clearance"]
        path_len += r["step_len"]
        dist[t + 1] = goal_dist_numpy(rps, env2table(traj[t + 1, :2]), tab)
    return dict(full_traj=traj, blocked=blocked, path_len=path_len, goal_dist=dist, clearance=clear)


# ---- tasks ------------------------------------------------------------------------------------------------------------------------------
START_ANGLE_DRAW = 7          # NavGenerator.draw_task uses the host draws 0 .. 6 of a key


def draw_tasks(n_rooms, seed, indices):
    """tasks (index, seed): start and goal of NavGenerator.draw_task (its first drawing), and a start angle in [-pi, pi) from one more
    keyed draw -> dict(start float32 [K, 3], goal float32 [K, 2]) in the environment's units.  Host only: nothing is launched."""
    from .nav_gen import NavGenerator
    gen = NavGenerator(n_rooms, seed=seed, device="cpu")
    start, goal = [], []
    for i in indices:
        t = gen.draw_task(int(i), 0)
        sg = np.asarray(t["start_goal"], dtype=np.float64)
        angle = (gen._u(t["key"], START_ANGLE_DRAW) * 2.0 - 1.0) * math.pi
        start.append(np.concatenate([table2env(sg[:2]), [np.float32(angle)]]))
        goal.append(table2env(sg[2:]))
    return dict(start=np.array(start, dtype=np.float32).reshape(-1, 3), goal=np.array(goal, dtype=np.float32).reshape(-1, 2))


def load_tasks(path):
    """an `.npz` with `start` [K, 3] and `goal` [K, 2] in the environment's units"""
    with np.load(path) as z:
        start, goal = np.asarray(z["start"], dtype=np.float32), np.asarray(z["goal"], dtype=np.float32)
    if start.ndim != 2 or start.shape[1] != 3 or goal.shape != (start.shape[0], 2):
        raise ValueError(f"{path}: start {start.shape} and goal {goal.shape}, expected [K, 3] and [K, 2]")
    return dict(start=start, goal=goal)


def default_assets(n_rooms, crop_window):
    """the untextured top-down assets of nav_gen.topdown_assets in the form dataset.load_topdown_assets returns"""
    from .dataset import topdown_table_size
    from .nav_gen import topdown_assets
    z = topdown_assets(n_rooms, crop_window)
    a = dict(background=np.ascontiguousarray(z["background"]), cw=int(z["crop_window"]), n_rooms=int(z["n_rooms"]),
             scale=int(z["render_scale"]), agent_stamp=z["agent_stamp"].astype(bool), goal_stamp=z["goal_stamp"].astype(bool),
             agent_color=z["agent_color"].astype(np.uint8).reshape(3), goal_color=z["goal_color"].astype(np.uint8).reshape(3))
    a["S"] = int(topdown_table_size(a["n_rooms"]) * a["scale"])
    return a


# ---- the batched environment --------------------------------------------------------------------------------------------------------------
class NavEnvBatch:
    """NavEnvBatch(n_rooms, crop_window, T, img_sz, device, assets=None): reset(tasks), step(actions_dev), observe(), eval().
    `assets`: a nav dataset's top-down assets (dataset.load_topdown_assets) when the model was trained on its pictures; default: the
    generator's untextured picture.  The record stays on the device until eval():
      state f32 [E, 3], full_traj f32 [E, T + 1, 3], goal_dist f64 [E, T + 1], path_len f64 [E], blocked u8 [E, T], actions f32 [E, T, 2],
      frames u8 [E, T + 1, H, W, 3], goal_frames u8 [E, H, W, 3]"""

    def __init__(self, n_rooms, crop_window, T, img_sz, device, assets=None):
        import torch
        from . import dataset as DS
        from . import runtime as rt
        self.torch, self.rt, self.lib, self.DS = torch, rt, rt.load_library(), DS
        self.n_rooms, self.rps = int(n_rooms), NL.rooms_per_side_of(int(n_rooms))
        self.T, self.img_sz, self.device = int(T), int(img_sz), torch.device(device)
        self.assets = assets if assets is not None else default_assets(self.n_rooms, int(crop_window))
        if self.assets["n_rooms"] != self.n_rooms or self.assets["cw"] != int(crop_window):
            raise ValueError(f"top-down assets for n_rooms = {self.assets['n_rooms']}, crop_window = {self.assets['cw']}; the environment "
                             f"has n_rooms = {self.n_rooms}, crop_window = {crop_window}")
        if self.T < 1:
            raise ValueError("T >= 1")
        self.cw, self.S, self.scale = self.assets["cw"], self.assets["S"], self.assets["scale"]
        self.table_size = NL.ROOM_SIZE * self.rps
        self.half_table = float(np.float32(0.5 * DS.topdown_table_size(self.n_rooms)))
        self.walls_np = wall_table(self.rps)
        self.walls = torch.from_numpy(self.walls_np).to(self.device)
        self.dev_assets = DS.topdown_device_assets(self.assets, self.img_sz, self.device)
        # the renderer converts a byte through a table: the identity here (the frames are kept as bytes), and the planner's format of a
        # byte, planning.env2planner, for the tensor the policy reads
        from .planning import env2planner
        self._lut_id = torch.arange(256, dtype=torch.float32, device=self.device)
        self._lut_planner = env2planner(np.arange(256, dtype=np.uint8).reshape(1, 1, 256, 1)).reshape(256).to(self.device)
        self.E = 0

    # -- reset --
    def reset(self, tasks):
        """tasks: dict(start [E, 3], goal [E, 2]) in the environment's units (draw_tasks / load_tasks).  Returns the first observation."""
        torch, dev = self.torch, self.device
        start = np.ascontiguousarray(np.asarray(tasks["start"], dtype=np.float32).reshape(-1, 3))
        goal = np.ascontiguousarray(np.asarray(tasks["goal"], dtype=np.float32).reshape(-1, 2))
        E, T, H = start.shape[0], self.T, self.img_sz
        if E < 1 or goal.shape[0] != E:
            raise ValueError(f"start {start.shape}, goal {goal.shape}: E >= 1 tasks")
        self.E, self.t = E, 0
        self.start_np, self.goal_np = start, goal
        tabs = np.stack([goal_table(self.rps, env2table(g)) for g in goal])
        goal_pix = self.DS.topdown_pixels(goal, self.n_rooms, self.scale, self.S, self.cw)
        fits = self.DS.topdown_fits(self.assets, goal_pix) & self.DS.topdown_fits(
            self.assets, self.DS.topdown_pixels(start, self.n_rooms, self.scale, self.S, self.cw))
        if not fits.all():
            raise ValueError(f"tasks {np.flatnonzero(~fits).tolist()}: start or goal lies outside the padded top-down picture")
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.goal_table, self.goal_pix = t(tabs), t(goal_pix)
        self.state = t(start)
        self.full_traj = torch.zeros(E, T + 1, 3, dtype=torch.float32, device=dev)
        self.goal_dist = torch.zeros(E, T + 1, dtype=torch.float64, device=dev)
        self.path_len = torch.zeros(E, dtype=torch.float64, device=dev)
        self.blocked = torch.zeros(E, T, dtype=torch.uint8, device=dev)
        self.actions = torch.zeros(E, T, 2, dtype=torch.float32, device=dev)
        self.pix = torch.zeros(E, 2, dtype=torch.int32, device=dev)
        self.frames = torch.zeros(E, T + 1, H, H, 3, dtype=torch.uint8, device=dev)
        # the renderer's staging: one frame per episode as a two-frame sequence whose second frame lies past end_ind
        self._coords = torch.zeros(E * 2 * 2 + E * 2, dtype=torch.int32, device=dev)      # [E][2 frames][2] agent pixels | [E][2] goal pixels
        self._coords[E * 4:] = self.goal_pix.reshape(-1)
        self._info = torch.tensor([[1, 0, 0, 0, 1, 0, 0, 0]] * E, dtype=torch.int32, device=dev)
        self._pad_in = torch.zeros(E * 2, dtype=torch.float32, device=dev)
        self._out = dict(traj_seq=torch.empty(E, 2, 3, H, H, dtype=torch.float32, device=dev),
                         I_0=torch.empty(E, 3, H, H, dtype=torch.float32, device=dev),
                         I_g=torch.empty(E, 3, H, H, dtype=torch.float32, device=dev),
                         pad_mask=torch.empty(E, 2, dtype=torch.float32, device=dev),
                         end_ind=torch.empty(E, dtype=torch.int64, device=dev), start_ind=torch.empty(E, dtype=torch.int64, device=dev))
        self.rt.check(self.lib.gcpx_nav_env_reset(self.state.data_ptr(), self.goal_table.data_ptr(), self.rps, self.table_size, E, T,
                                                  self.half_table, float(self.scale), self.S, self.cw, self.full_traj.data_ptr(),
                                                  self.path_len.data_ptr(), self.goal_dist.data_ptr(), self.pix.data_ptr(),
                                                  self.rt.current_stream()), "nav_env_reset")
        # the goal image of a task: the observation with the agent at the goal
        self.goal_frames = self._render(self.goal_pix)[1].clone()
        return self.observe()

    # -- one step --
    def step(self, actions_dev):
        """actions_dev: float32 device tensor [E, 2]; advances every episode by one step (one launch, nothing crosses to the host)"""
        if self.t >= self.T:
            raise ValueError(f"step {self.t} of an episode of T = {self.T} steps")
        a = actions_dev.to(device=self.device, dtype=self.torch.float32).reshape(self.E, 2).contiguous()
        self.actions[:, self.t] = a
        self.rt.check(self.lib.gcpx_nav_env_step(self.state.data_ptr(), a.data_ptr(), self.walls.data_ptr(), self.walls.shape[0],
                                                 NL.ROBOT_SIZE, self.goal_table.data_ptr(), self.rps, self.table_size, self.E, self.T,
                                                 self.t, self.half_table, float(self.scale), self.S, self.cw, self.full_traj.data_ptr(),
                                                 self.path_len.data_ptr(), self.goal_dist.data_ptr(), self.blocked.data_ptr(),
                                                 self.pix.data_ptr(), self.rt.current_stream()), "nav_env_step")
        self.t += 1

    # -- observation --
    def _render(self, pix):
        """agent pixels int32 [E, 2] -> (planner-format float32 [E, 3, H, W], uint8 [E, H, W, 3]): the dataset's renderer, one frame
        per episode"""
        self._coords[:self.E * 4].view(self.E, 2, 2)[:, 0] = pix
        self.DS.topdown_assemble_into(self.lib, self.dev_assets, self._coords, self._pad_in, self._info, self._lut_id, None, None,
                                      self._out, 0, 0, self.rt.current_stream())
        byte = self._out["I_0"].to(self.torch.int64)
        return self._lut_planner[byte], byte.to(self.torch.uint8).permute(0, 2, 3, 1).contiguous()

    def observe(self):
        """the frame the model was trained on, for the current state of every episode -> planner-format float32 [E, 3, H, W] (what
        planning.env2planner makes of the uint8 frame); the uint8 frame is recorded as frames[:, t]"""
        planner, u8 = self._render(self.pix)
        self.frames[:, self.t] = u8
        return planner

    # -- evaluation --
    def eval(self):
        """BaseMiniworldEnv.eval per episode, as arrays over E: improvement, initial_dist, final_dist, all_goal_distances [E, T + 1],
        full_traj [E, T + 1, 3], goal [E, 2]; and path_len [E], blocked [E, T].  Rows past the steps taken so far are zero."""
        d = self.goal_dist.cpu().numpy()
        return dict(improvement=d[:, 0] - d[:, self.t], initial_dist=d[:, 0].copy(), final_dist=d[:, self.t].copy(), all_goal_distances=d,
                    full_traj=self.full_traj.cpu().numpy(), goal=self.goal_np.copy(), path_len=self.path_len.cpu().numpy(),
                    blocked=self.blocked.cpu().numpy())
