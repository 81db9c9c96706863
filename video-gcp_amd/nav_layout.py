"""The nav datasets' maze as data (host, numpy): this build's restatement of the reference's layout and room bookkeeping.

  layout(rooms_per_side)     define_layout_raw / define_layout (multiroom2d_layout.py:11-182) with MULTIMODAL = True and
                             NON_SYMMETRIC = False as the reference ships them, for 3, 4 and 5 rooms per side: the obstacle point
                             cloud `ox`, `oy` (float64, the same linspace expressions, so bit-identical: 3 828 points for 9 rooms,
                             9 304 for 25), robot_size, table_size, the doors as pairs of room indices (lower index first, in the
                             order the reference's recursion opens them) and coords2ridx
  RoomBoxes                  RoomSampler2d's boxes (sampling_fcns.py:12-79): room centre and sampling width, get_door_pos, the door
                             sampling widths of horizontal and vertical connections
  plan_room_seq              the breadth-first room search of prm_policy.py:228-254
  room_paths                 plan_room_seq_multimodal (:257-289) without its draw: every simple room path from start to goal in the
                             reference's breadth-first order (the reference returns one of them, drawn uniformly); cached per pair
  compute_shortest_path      prm_policy.py:198-216: the length over the door centres of plan_room_seq; (10., []) outside [-0.5, 0.5]
  wall_segments              the wall and closed-door segments in table coordinates, in the order the cloud is built: what
                             draw_layout_overview (:265-294) turns into lines
"""
import functools
import math
from collections import deque

import numpy as np

ROBOT_SIZE = 0.02
ROOM_SIZE = 1 / 3
DOOR_SIZE = 1.5 * 0.0667
_NEIGHBORS = ((0, 1), (1, 0), (-1, 0), (0, -1))
# the doors gen_doors_multimodal closes again (pairs of room coordinates; a pair that names no door is skipped, as maybe_remove does)
_CLOSED = {
    3: (((1, 1), (1, 2)), ((1, 1), (1, 0))),
    4: (((0, 3), (1, 3)), ((1, 0), (2, 0)), ((2, 1), (3, 1)), ((2, 2), (3, 2)), ((2, 3), (3, 3)), ((1, 3), (1, 4))),
    5: (((0, 3), (1, 3)), ((1, 0), (2, 0)), ((2, 1), (3, 1)), ((2, 2), (3, 2)), ((2, 3), (3, 3)), ((1, 3), (1, 4)), ((1, 1), (1, 2)),
        ((2, 1), (2, 2)), ((3, 1), (3, 2)), ((4, 2), (4, 3))),
}


def door_coords(rooms_per_side):
    """gen_doors_multimodal (multiroom2d_layout.py:106-154): every door between neighbouring rooms, in the order a depth-first walk from
    room (0, 0) meets them, minus the closed ones; pairs of room coordinates"""
    if rooms_per_side not in _CLOSED:
        raise NotImplementedError(f"rooms_per_side = {rooms_per_side}: the reference defines the multimodal layout for 3, 4 and 5")
    n = rooms_per_side
    doors, known = [], set()
    stack = [((0, 0), 0)]                                   # the reference recurses; the same walk with an explicit stack
    while stack:
        (x, y), k = stack.pop()
        while k < 4:
            dx, dy = _NEIGHBORS[k]
            k += 1
            nx, ny = x + dx, y + dy
            if not (0 <= nx < n and 0 <= ny < n) or frozenset(((x, y), (nx, ny))) in known:
                continue
            known.add(frozenset(((x, y), (nx, ny))))
            doors.append(((x, y), (nx, ny)))
            stack.append(((x, y), k))
            stack.append(((nx, ny), 0))
            break
    for r1, r2 in _CLOSED[n]:
        if (r1, r2) in doors:
            doors.remove((r1, r2))
        elif (r2, r1) in doors:
            doors.remove((r2, r1))
    return doors


def wall_segments(rooms_per_side):
    """[(kind, (lo, hi), at)] in the order define_layout_raw adds them: kind 'h' is a horizontal line x in [lo, hi] at y = at, 'v' a
    vertical line y in [lo, hi] at x = at; table coordinates in [0, table_size] (multiroom2d_layout.py:35-69)"""
    n = rooms_per_side
    table = ROOM_SIZE * n
    segs = [("h", (0, table), 0), ("h", (0, table), table), ("v", (0, table), 0), ("v", (0, table), table)]
    for kind in ("h", "v"):
        for r in range(n):
            at = (r + 1) * ROOM_SIZE
            segs.append((kind, (0, 1 * ROOM_SIZE / 2 - DOOR_SIZE / 2), at))
            for s in range(n - 1):
                segs.append((kind, ((2 * s + 1) * ROOM_SIZE / 2 + DOOR_SIZE / 2, (2 * (s + 1) + 1) * ROOM_SIZE / 2 - DOOR_SIZE / 2), at))
            segs.append((kind, ((n - 0.5) * ROOM_SIZE + DOOR_SIZE / 2, n * ROOM_SIZE), at))
    doors = door_coords(n)
    for rx in range(n):
        for ry in range(n):
            if rx + 1 < n and ((rx, ry), (rx + 1, ry)) not in doors and ((rx + 1, ry), (rx, ry)) not in doors:
                c = ROOM_SIZE / 2 + ry * ROOM_SIZE
                segs.append(("v", (c - DOOR_SIZE / 2, c + DOOR_SIZE / 2), (rx + 1) * ROOM_SIZE))
            if ry + 1 < n and ((rx, ry), (rx, ry + 1)) not in doors and ((rx, ry + 1), (rx, ry)) not in doors:
                c = ROOM_SIZE / 2 + rx * ROOM_SIZE
                segs.append(("h", (c - DOOR_SIZE / 2, c + DOOR_SIZE / 2), (ry + 1) * ROOM_SIZE))
    return segs


class Layout:
    """what define_layout returns, without textures"""

    def __init__(self, rooms_per_side):
        n = self.rooms_per_side = int(rooms_per_side)
        self.n_rooms = n * n
        self.robot_size, self.room_size, self.door_size = ROBOT_SIZE, ROOM_SIZE, DOOR_SIZE
        self.table_size = ROOM_SIZE * n
        offset = 0.5 * n * ROOM_SIZE                         # centred on (0, 0)
        parts = []
        for kind, (lo, hi), at in wall_segments(n):
            along = np.linspace(lo, hi, int((hi - lo + 1) * 100))
            across = at * np.ones_like(along)
            parts.append(np.stack([along, across] if kind == "h" else [across, along], axis=0) - offset)
        o = np.concatenate(parts, axis=1)
        self.ox, self.oy = np.ascontiguousarray(o[0]), np.ascontiguousarray(o[1])
        ridx = lambda c: c[0] * n + (n - 1) - c[1]
        self.doors = [sorted((ridx(a), ridx(b))) for a, b in door_coords(n)]

    def coords2ridx(self, x, y):
        """float coordinates -> room index (define_layout's coords2ridx)"""
        xr, yr = (np.floor((c + self.table_size / 2) / ROOM_SIZE) for c in (x, y))
        r = xr * self.rooms_per_side + (self.rooms_per_side - 1) - yr
        return int(r) if np.ndim(r) == 0 else np.asarray(r, dtype=int)


@functools.lru_cache(maxsize=None)
def layout(rooms_per_side):
    return Layout(rooms_per_side)


class RoomBoxes:
    """RoomSampler2d (sampling_fcns.py:12-79) as boxes: a draw is (u - 0.5) * width + centre with u uniform in [0, 1)^2"""

    def __init__(self, rooms_per_side, sample_wide=False):
        self.n = int(rooms_per_side)
        self.agent_size = 0.02
        self.sampling_width = 1 / 3 - (not sample_wide) * 3 * self.agent_size
        self.room_offset = 1 / 3
        self.door_sampling_width = 1.5 * 0.0667 - 3 * self.agent_size
        self.hor_door_sampling_width = np.array([2 * self.agent_size, self.door_sampling_width])
        self.vert_door_sampling_width = np.array([self.door_sampling_width, 2 * self.agent_size])

    def ridx2coords(self, room):
        return int(np.floor(room / self.n)), int(self.n - 1 - room % self.n)

    def room_center(self, room):
        return np.array([self.room_offset / 2 + i * self.room_offset - self.n / 2 * self.room_offset for i in self.ridx2coords(room)])

    def get_door_pos(self, room1, room2):
        assert room1 < room2
        c1, c2 = self.ridx2coords(room1), self.ridx2coords(room2)
        assert abs(c1[0] - c2[0] + c1[1] - c2[1]) == 1
        return np.array([self.room_offset / 2 + (i + j) / 2 * self.room_offset - self.n / 2 * self.room_offset for i, j in zip(c1, c2)])

    def door_width(self, room1, room2):
        """the sampling widths of the door between two rooms: a horizontal connection (the rooms differ in x) or a vertical one"""
        c1, c2 = self.ridx2coords(room1), self.ridx2coords(room2)
        if c1[0] != c2[0] and c1[1] == c2[1]:
            return self.hor_door_sampling_width
        if c1[0] == c2[0] and c1[1] != c2[1]:
            return self.vert_door_sampling_width
        raise ValueError("Rooms don't have connection for door.")

    def box_table(self, doors):
        """float64 [n_rooms + 2 * len(doors), 4] = (centre x, centre y, width x, width y): the rooms, then the doors of `doors` in its
        order, then the same doors with zero widths (sample_door_center)"""
        rows = [np.concatenate([self.room_center(r), [self.sampling_width] * 2]) for r in range(self.n * self.n)]
        rows += [np.concatenate([self.get_door_pos(a, b), self.door_width(a, b)]) for a, b in doors]
        rows += [np.concatenate([self.get_door_pos(a, b), [0., 0.]]) for a, b in doors]
        return np.ascontiguousarray(np.stack(rows), dtype=np.float64)


def _neighbours(room, doors, seen):
    out = []
    for d in doors:
        if d[0] == room and d[1] not in seen:
            out.append(d[1])
        elif d[1] == room and d[0] not in seen:
            out.append(d[0])
    return out


def plan_room_seq(start, goal, doors):
    """breadth-first room search (prm_policy.py:228-254): a room counts as visited once it is expanded, so it can be queued twice"""
    frontier, visited = deque(), []
    node = (start, None)
    while node[0] != goal:
        visited.append(node[0])
        for nb in _neighbours(node[0], doors, visited):
            frontier.append((nb, node))
        node = frontier.popleft()
    path = []
    while node is not None:
        path.append(node[0])
        node = node[1]
    return path[::-1]


def _room_paths(start, goal, doors):
    frontier, found = deque(), []
    path = (start,)
    while True:
        if path[-1] == goal:
            found.append(list(path))
        else:
            for nb in _neighbours(path[-1], doors, path):
                frontier.append(path + (nb,))
        if not frontier:
            return found
        path = frontier.popleft()


@functools.lru_cache(maxsize=None)
def room_paths(rooms_per_side, start, goal):
    """every simple room path start -> goal of the layout in the order plan_room_seq_multimodal collects them (short to long)"""
    return _room_paths(start, goal, layout(rooms_per_side).doors)


@functools.lru_cache(maxsize=None)
def _bfs_cached(rooms_per_side, start, goal):
    return plan_room_seq(start, goal, layout(rooms_per_side).doors)


def compute_shortest_path(rooms_per_side, p1, p2):
    """(length, waypoints) over the door centres of the breadth-first room sequence (prm_policy.py:198-216, transform_pose=False,
    straight_through_door=False); (10., []) when a coordinate lies outside [-0.5, 0.5] -- as the reference has it, whatever the table's
    size"""
    p1, p2 = np.asarray(p1, dtype=np.float64), np.asarray(p2, dtype=np.float64)
    both = np.stack((p1, p2))
    if (both < -0.5).any() or (both > 0.5).any():
        return 10., []
    L, boxes = layout(rooms_per_side), RoomBoxes(rooms_per_side)
    rooms = _bfs_cached(rooms_per_side, L.coords2ridx(p1[0], p1[1]), L.coords2ridx(p2[0], p2[1]))
    way = [p1] + [boxes.get_door_pos(min(a, b), max(a, b)) for a, b in zip(rooms[:-1], rooms[1:])] + [p2]
    way = np.array(way)
    return np.linalg.norm(way[1:] - way[:-1], axis=1).sum(), way


def rooms_per_side_of(n_rooms):
    n = int(math.sqrt(n_rooms))
    if n * n != n_rooms or n not in _CLOSED:
        raise ValueError(f"n_rooms = {n_rooms}: the layouts are 9, 16 and 25 rooms")
    return n
