"""Golden data for the nav data generator from the REFERENCE's own code, executed (build container only: needs scipy and matplotlib).

It loads the reference's prm.py, multiroom2d_layout.py, sampling_fcns.py (and prm_policy.py for the room searches) by path, with two
stubs: `blox.AttrDict` and an empty `cv2` module (plus a `Policy` base class and the three module names prm_policy.py imports).

Run from the repo root:  python tests/golden/make_ref_prm_goldens.py <reference checkout>
Writes tests/golden/ref_prm.npz (data only) and tests/golden/ref_nav_16rooms_mod_hyper.json (the settings of
experiments/data_gen/nav_16rooms/mod_hyper.py).

PRM cases a-e: the inputs are drawn here (numpy RandomState) and handed to PRM_planning through `sampled_points`; recorded are the input
points, the kept mask, the full road map (padded with -1), the path indices, success and the cost, and the smallest margins seen:
  |dist - rr| over every obstacle query of the filter and of every collision walk, |d - max_edge_len| over all node pairs,
  |frac(d / rr) - 0.5| over all tested edges (round's half-way point), the gaps between a node's sorted neighbour distances below
  max_edge_len (its own 0 included), and the gap between the best and the second-best path cost.
A seed is kept only if every margin exceeds 1e-9: then float64 arithmetic in another order of operations takes the same decisions.
"""
import hashlib
import heapq
import importlib.util
import json
import math
import os
import sys
import threading
import time
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
OUT = os.path.join(HERE, "ref_prm.npz")
OUT_CONF = os.path.join(HERE, "ref_nav_16rooms_mod_hyper.json")
MARGIN = 1e-9
INFRA = os.path.join("gcp", "planning", "infra")


class AttrDict(dict):
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


def load_reference(ref):
    blox = types.ModuleType("blox")
    blox.AttrDict = AttrDict
    sys.modules["blox"] = blox
    sys.modules["cv2"] = types.ModuleType("cv2")

    def load(name, rel):
        spec = importlib.util.spec_from_file_location(name, os.path.join(ref, rel))
        m = importlib.util.module_from_spec(spec)
        sys.modules[name] = m
        spec.loader.exec_module(m)
        return m

    for pkg in ("gcp", "gcp.planning", "gcp.planning.infra", "gcp.planning.infra.envs", "gcp.planning.infra.envs.miniworld_env",
                "gcp.planning.infra.envs.miniworld_env.utils", "gcp.planning.infra.policy", "gcp.planning.infra.policy.prm_policy"):
        sys.modules.setdefault(pkg, types.ModuleType(pkg))
    lay = load("gcp.planning.infra.envs.miniworld_env.utils.multiroom2d_layout",
               os.path.join(INFRA, "envs", "miniworld_env", "utils", "multiroom2d_layout.py"))
    smp = load("gcp.planning.infra.envs.miniworld_env.utils.sampling_fcns", os.path.join(INFRA, "envs", "miniworld_env", "utils", "sampling_fcns.py"))
    prm = load("gcp.planning.infra.policy.prm_policy.prm", os.path.join(INFRA, "policy", "prm_policy", "prm.py"))
    pol = types.ModuleType("gcp.planning.infra.policy.policy")
    pol.Policy = type("Policy", (), {})
    sys.modules["gcp.planning.infra.policy.policy"] = pol
    pp = load("gcp.planning.infra.policy.prm_policy.prm_policy", os.path.join(INFRA, "policy", "prm_policy", "prm_policy.py"))
    return lay, smp, prm, pp


def all_room_paths(pp, start, goal, doors):
    """plan_room_seq_multimodal's ordered list: its np.random.choice is replaced for the call by a function that records the list"""
    seen = {}

    def choice(nodes):
        seen["nodes"] = list(nodes)
        return nodes[0]

    saved = pp.np.random.choice
    pp.np.random.choice = choice
    try:
        pp.plan_room_seq_multimodal(start, goal, doors)
    finally:
        pp.np.random.choice = saved
    out = []
    for node in seen["nodes"]:
        path = []
        while node is not None:
            path.append(node.room)
            node = node.parent
        out.append(path[::-1])
    return out


def ragged(lists):
    flat = np.array([x for l in lists for x in l], dtype=np.int32)
    off = np.zeros(len(lists) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(l) for l in lists])
    return flat, off


def margins(prm, px, py, sx, sy, gx, gy, ox, oy, rr, max_len, n_knn, cost_power, x, y, road, path, cost):
    """the smallest distances of the reference's decisions from their thresholds (own code over scipy's cKDTree, the reference's tree)"""
    import scipy.spatial
    tree = scipy.spatial.cKDTree(np.vstack((ox, oy)).T)
    m = dict(obst=np.inf, edge=np.inf, half=np.inf, gap=np.inf, cost=np.inf)
    d0, _ = tree.query(np.stack([px, py], axis=1))
    m["obst"] = min(m["obst"], np.abs(d0 - rr).min())
    n = len(x)
    X, Y = np.asarray(x), np.asarray(y)
    for i in range(n):
        dx, dy = X - X[i], Y - Y[i]
        d = np.sqrt(dx ** 2 + dy ** 2)
        m["edge"] = min(m["edge"], np.abs(d - max_len).min())
        near = np.sort(d[d < max_len])                      # the node's own 0 first
        if near.shape[0] > 1:
            m["gap"] = min(m["gap"], np.diff(near).min())
        for j in np.flatnonzero((d < max_len) & (np.arange(n) != i)):
            q = d[j] / rr
            m["half"] = min(m["half"], abs(q - math.floor(q) - 0.5))
            yaw = math.atan2(dy[j], dx[j])
            wx, wy = X[i], Y[i]
            pts = []
            for _ in range(round(q)):
                pts.append((wx, wy))
                wx += rr * math.cos(yaw)
                wy += rr * math.sin(yaw)
            pts.append((X[j], Y[j]))
            dd, _ = tree.query(np.array(pts))
            hit = np.flatnonzero(dd <= rr)
            dd = dd[:hit[0] + 1] if hit.shape[0] else dd    # the reference stops at the first collision
            m["obst"] = min(m["obst"], np.abs(dd - rr).min())
    if len(path):                                           # second-best path: through some edge off the best one
        w = lambda a, b: math.sqrt((X[b] - X[a]) ** 2 + (Y[b] - Y[a]) ** 2) ** cost_power
        fwd, rev = {i: [(int(j), w(i, j)) for j in road[i] if j >= 0] for i in range(n)}, {i: [] for i in range(n)}
        for i in range(n):
            for j, c in fwd[i]:
                rev[j].append((i, c))

        def dijkstra(src, graph):
            dist = np.full(n, np.inf)
            dist[src] = 0.0
            heap = [(0.0, src)]
            while heap:
                c, i = heapq.heappop(heap)
                if c > dist[i]:
                    continue
                for j, ww in graph[i]:
                    if c + ww < dist[j]:
                        dist[j] = c + ww
                        heapq.heappush(heap, (c + ww, j))
            return dist

        ds, dt = dijkstra(n - 2, fwd), dijkstra(n - 1, rev)
        on = set(zip(path[:-1], path[1:]))
        second = min([ds[i] + c + dt[j] for i in range(n) for j, c in fwd[i] if (i, j) not in on] or [np.inf])
        m["cost"] = second - cost
    return m


def run_case(lay, smp, prm, name, rooms_per_side, room_path, per_room, per_door, seed0, expect_success, n_knn=10, max_len=0.1, power=2):
    layout = lay.define_layout_raw(rooms_per_side)
    ox, oy = list(layout[0][0]), list(layout[0][1])
    rr = layout[1]
    params = AttrDict(n_knn=n_knn, max_edge_len=max_len, cost_fcn=lambda d: d ** power)
    for seed in range(seed0, seed0 + 200):
        np.random.seed(seed)
        sampler = smp.RoomSampler2d(rooms_per_side)
        s, g = sampler.sample(room_path[0]), sampler.sample(room_path[-1])
        px, py = [], []
        for room in room_path:
            for _ in range(per_room):
                p = sampler.sample(room)
                px.append(p[0])
                py.append(p[1])
        for a, b in zip(room_path[:-1], room_path[1:]):
            for _ in range(per_door):
                p = sampler.sample_door(min(a, b), max(a, b))
                px.append(p[0])
                py.append(p[1])
        px, py = np.array(px), np.array(py)
        tree = prm.KDTree(np.vstack((ox, oy)).T)
        x, y = prm.sample_points(s[0], s[1], g[0], g[1], rr, ox, oy, tree, 0, [px, py])
        kept = np.array([tree.search(np.array([a, b]).reshape(2, 1))[1][0] >= rr for a, b in zip(px, py)])
        assert kept.sum() + 2 == len(x)
        t0 = time.time()
        road = prm.generate_roadmap(x, y, rr, tree, params)
        rx, ry, success = prm.dijkstra_planning(s[0], s[1], g[0], g[1], ox, oy, rr, road, x, y, params.cost_fcn)
        seconds = time.time() - t0
        if success != expect_success:
            continue
        rx, ry = rx[::-1], ry[::-1]
        xy = {(a, b): i for i, (a, b) in enumerate(zip(x, y))}
        path = [xy[(a, b)] for a, b in zip(rx, ry)] if success else []
        pad = np.full((len(x), n_knn), -1, dtype=np.int32)
        for i, e in enumerate(road):
            pad[i, :len(e)] = e
        cost = 0.0
        for a, b in zip(path[:-1], path[1:]):
            cost = cost + params.cost_fcn(math.sqrt((x[b] - x[a]) ** 2 + (y[b] - y[a]) ** 2))
        mg = margins(prm, px, py, s[0], s[1], g[0], g[1], np.array(ox), np.array(oy), rr, max_len, n_knn, power, x, y, pad, path, cost)
        if min(mg.values()) <= MARGIN or (success and len(path) < 4):
            print(f"case {name}: seed {seed} rejected, margins {mg}")
            continue
        print(f"case {name}: seed {seed}, {len(x)} nodes, success {success}, {len(path)} vertices, {seconds:.2f} s, margins {mg}")
        out = {f"case_{name}/{k}": v for k, v in dict(
            rooms_per_side=np.int64(rooms_per_side), px=px, py=py, start_goal=np.array([s[0], s[1], g[0], g[1]]), kept=kept,
            road_map=pad, path=np.array(path, dtype=np.int32), success=np.int64(success), cost=np.float64(cost if success else np.inf),
            n_knn=np.int64(n_knn), max_edge_len=np.float64(max_len), cost_power=np.float64(power), seed=np.int64(seed),
            margins=np.array([mg[k] for k in ("obst", "edge", "half", "gap", "cost")]), ref_seconds=np.float64(seconds)).items()}
        if success:
            from scipy import interpolate
            vx, vy = [x[i] for i in path], [y[i] for i in path]
            tck, u = interpolate.splprep([vx, vy], s=0.0)
            bs = interpolate.make_interp_spline(u, np.stack([vx, vy], axis=1), k=3)
            diff = 0.0
            for ns in (4, 5, 60, 100):
                t = np.linspace(0, 1, ns)
                a = np.stack(interpolate.splev(t, tck), axis=1)
                out[f"case_{name}/spline_{ns}"] = a
                diff = max(diff, float(np.abs(a - bs(t)).max()))
            out[f"case_{name}/spline_route_diff"] = np.float64(diff)
        return out
    raise RuntimeError(f"case {name}: no seed with margins above {MARGIN}")


def main():
    ref = sys.argv[1]
    lay, smp, prm, pp = load_reference(ref)
    out = {}
    for n in (3, 4, 5):
        o, robot, table, doors = lay.define_layout_raw(n)
        out[f"layout{n}/doors"] = np.array(doors, dtype=np.int32)
        out[f"layout{n}/table_size"] = np.float64(table)
        out[f"layout{n}/robot_size"] = np.float64(robot)
        out[f"layout{n}/n_points"] = np.int64(o.shape[1])
        out[f"layout{n}/sha256"] = np.array([hashlib.sha256(np.ascontiguousarray(o[k]).tobytes()).hexdigest() for k in range(2)])
        if n == 3:
            out["layout3/ox"], out["layout3/oy"] = o[0], o[1]
        sampler = smp.RoomSampler2d(n)
        out[f"layout{n}/door_pos"] = np.stack([sampler.get_door_pos(a, b) for a, b in doors])
        out[f"layout{n}/room_box"] = np.array([sampler._sampling_width, sampler._door_sampling_width, *sampler._hor_door_sampling_width,
                                               *sampler._vert_door_sampling_width])
        lay.load_textures = lambda texture_dir: None          # no textures here; define_layout is called for its coords2ridx
        L = lay.define_layout(n, texture_dir="none")
        rs = np.random.RandomState(n)
        q = rs.uniform(-table / 2, table / 2, size=(40, 2))
        out[f"layout{n}/ridx_query"] = q
        out[f"layout{n}/ridx"] = np.array([L.coords2ridx(a, b) for a, b in q], dtype=np.int64)
        if n in (3, 5):
            bfs, multi = [], []
            for a in range(n * n):
                for b in range(n * n):
                    bfs.append(pp.plan_room_seq(a, b, doors))
                    multi.append(all_room_paths(pp, a, b, doors))
            out[f"layout{n}/bfs"], out[f"layout{n}/bfs_off"] = ragged(bfs)
            out[f"layout{n}/multi_count"] = np.array([len(m) for m in multi], dtype=np.int32)
            out[f"layout{n}/multi"], out[f"layout{n}/multi_off"] = ragged([p for m in multi for p in m])
            print(f"{n} rooms per side: at most {max(len(m) for m in multi)} simple paths per pair")
            self = types.SimpleNamespace(convert=None, layout=L, state_sampler=sampler)
            pts = np.random.RandomState(100 + n).uniform(-0.6 if n == 5 else -0.5, 0.6 if n == 5 else 0.5, size=(20, 2, 2))
            out[f"layout{n}/sp_points"] = pts
            out[f"layout{n}/sp_length"] = np.array([pp.PrmPolicy.compute_shortest_path(self, p[0], p[1], transform_pose=False)[0] for p in pts])
            if n == 5:
                longest = max((p for m in multi for p in m), key=len)
    # the PRM cases
    d3 = lay.define_layout_raw(3)[3]
    seq5 = next(p for p in all_room_paths(pp, 0, 8, d3) if len(p) == 5)
    out.update(run_case(lay, smp, prm, "a", 3, [0, 3], 8, 3, 0, True))
    out.update(run_case(lay, smp, prm, "b", 3, seq5, 50, 3, 0, True))
    out.update(run_case(lay, smp, prm, "c", 3, [0, 3], 300, 3, 0, True))
    out.update(run_case(lay, smp, prm, "d", 5, longest, 50, 3, 0, True))
    out.update(run_case(lay, smp, prm, "e", 3, seq5, 2, 0, 0, False))
    # the reference's seconds per plan at the default (case b: generate_roadmap + dijkstra_planning on this machine's CPU)
    out["ref_seconds_per_plan_9rooms"] = out["case_b/ref_seconds"]
    out["ref_seconds_per_plan_25rooms"] = out["case_d/ref_seconds"]
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")
    # the data-collection conf, as settings
    from video_gcp_amd import conf_loader as CL
    os.environ.setdefault("GCP_DATA_DIR", "GCP_DATA_DIR")
    ns = CL._exec_with_placeholders(os.path.join(ref, "experiments", "data_gen", "nav_16rooms", "mod_hyper.py"), "mod_hyper")

    def plain(v):
        if isinstance(v, dict):
            return {k: plain(x) for k, x in v.items()}
        if isinstance(v, (list, tuple)):
            return [plain(x) for x in v]
        if v is None or isinstance(v, (bool, int, float, str)):
            return v
        return getattr(v, "__name__", repr(v))

    conf = plain(dict(ns["config"]))
    conf.pop("current_dir", None)
    with open(OUT_CONF, "w") as f:
        json.dump({"source": "experiments/data_gen/nav_16rooms/mod_hyper.py", "config": conf}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", OUT_CONF)


if __name__ == "__main__":
    sys.setrecursionlimit(1000000)
    threading.stack_size(1 << 29)
    t = threading.Thread(target=main)
    t.start()
    t.join()
