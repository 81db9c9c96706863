"""The nav data generator's kernels (csrc/prm.hip) against tests/golden/ref_prm.npz -- the reference's own PRM_planning, executed, on
recorded sample points -- and the generator end to end.  Bounds and the exactness condition: tests/test_nav_gen_cpu.py (the golden seeds
keep every decision further than 1e-9 from its threshold, so the integers must be equal; the spline may differ from splev by 100 x the
difference of scipy's two routes, at least 1e-12; the path cost is a float64 sum in another order: 1e-12 relative)."""
import os

import numpy as np
import pytest
import torch

from video_gcp_amd import nav_gen as NG
from video_gcp_amd import nav_layout as NL
from video_gcp_amd import runtime as rt

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ("a", "b", "c", "d", "e")
DEV = "cuda:0"


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(HERE, "golden", "ref_prm.npz")) as z:
        return {k: z[k] for k in z.files}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run_cases(lib, gold, cases):
    """the roadmap and shortest-path kernels on the golden points of `cases` (one layout) as one ragged batch"""
    g = lambda c, k: gold[f"case_{c}/{k}"]
    rps = int(g(cases[0], "rooms_per_side"))
    assert all(int(g(c, "rooms_per_side")) == rps for c in cases)
    L = NL.layout(rps)
    grid = NG.obstacle_grid(L.ox, L.oy, L.robot_size)
    n_knn = int(g(cases[0], "n_knn"))
    off = np.zeros(len(cases) + 1, dtype=np.int32)
    off[1:] = np.cumsum([g(c, "px").shape[0] for c in cases])
    total, max_pts, B = int(off[-1]), int(np.diff(off).max()), len(cases)
    cap = max_pts + 2
    o = dict(px=dev(np.concatenate([g(c, "px") for c in cases])), py=dev(np.concatenate([g(c, "py") for c in cases])),
             sg=dev(np.stack([g(c, "start_goal") for c in cases])), off=dev(off), ox=dev(grid["ox"]), oy=dev(grid["oy"]),
             cs=dev(grid["cell_start"]), kept=torch.full((total,), 7, dtype=torch.uint8, device=DEV),
             n_nodes=torch.zeros(B, dtype=torch.int32, device=DEV), node_xy=torch.full((B, 2, cap), -9., dtype=torch.float64, device=DEV),
             adj=torch.full((B, cap, n_knn), -5, dtype=torch.int32, device=DEV), success=torch.full((B,), -3, dtype=torch.int32, device=DEV),
             n_vert=torch.full((B,), -3, dtype=torch.int32, device=DEV), path=torch.full((B, cap), -3, dtype=torch.int32, device=DEV),
             cost=torch.full((B,), -3., dtype=torch.float64, device=DEV))
    s = rt.current_stream()
    rt.check(lib.gcpx_prm_roadmap(o["ox"].data_ptr(), o["oy"].data_ptr(), o["cs"].data_ptr(), grid["n_obs"], grid["gx"], grid["gy"],
                                  grid["x0"], grid["y0"], grid["cell"], o["px"].data_ptr(), o["py"].data_ptr(), o["off"].data_ptr(),
                                  o["sg"].data_ptr(), B, total, max_pts, cap, n_knn, L.robot_size, float(g(cases[0], "max_edge_len")),
                                  o["kept"].data_ptr(), o["n_nodes"].data_ptr(), o["node_xy"].data_ptr(), o["adj"].data_ptr(), s), "roadmap")
    rt.check(lib.gcpx_prm_shortest_path(o["node_xy"].data_ptr(), o["n_nodes"].data_ptr(), o["adj"].data_ptr(), B, cap, n_knn,
                                        float(g(cases[0], "cost_power")), o["success"].data_ptr(), o["n_vert"].data_ptr(),
                                        o["path"].data_ptr(), o["cost"].data_ptr(), s), "shortest_path")
    torch.cuda.synchronize()
    o.update(cases=cases, pt_off=off, cap=cap, B=B)
    return o


@pytest.fixture(scope="module")
def planned(gcpx_lib, gold):
    """cases a, b, c, e (9 rooms) in one launch, case d (25 rooms) in another: computed once, shared, left unchanged"""
    return {c: (o, i) for cases in (("a", "b", "c", "e"), ("d",)) for o in [run_cases(gcpx_lib, gold, cases)] for i, c in enumerate(cases)}


@pytest.mark.parametrize("case", CASES)
def test_roadmap_equals_the_reference(planned, gold, case):
    o, i = planned[case]
    g = lambda k: gold[f"case_{case}/{k}"]
    assert float(g("margins").min()) > 1e-9
    kept = o["kept"][o["pt_off"][i]:o["pt_off"][i + 1]].cpu().numpy()
    assert np.array_equal(kept, g("kept").astype(np.uint8))
    n = int(g("kept").sum()) + 2
    assert int(o["n_nodes"][i]) == n
    x = np.concatenate([g("px")[g("kept")], g("start_goal")[[0, 2]]]), np.concatenate([g("py")[g("kept")], g("start_goal")[[1, 3]]])
    xy = o["node_xy"][i].cpu().numpy()
    assert np.array_equal(xy[0, :n], x[0]) and np.array_equal(xy[1, :n], x[1]) and (xy[:, n:] == 0).all()
    adj = o["adj"][i].cpu().numpy()
    assert np.array_equal(adj[:n], g("road_map"))
    assert (adj[n:] == -1).all()


@pytest.mark.parametrize("case", CASES)
def test_shortest_path_equals_the_reference(planned, gold, case):
    o, i = planned[case]
    g = lambda k: gold[f"case_{case}/{k}"]
    assert int(o["success"][i]) == int(g("success"))
    if case == "e":                                          # no path: a normal result, the outputs keep their fill values
        assert int(o["n_vert"][i]) == -3 and float(o["cost"][i]) == -3. and (o["path"][i] == -3).all()
        return
    m = g("path").shape[0]
    assert int(o["n_vert"][i]) == m
    path = o["path"][i].cpu().numpy()
    assert np.array_equal(path[:m], g("path")) and (path[m:] == -3).all()
    assert abs(float(o["cost"][i]) - float(g("cost"))) <= 1e-12 * float(g("cost"))


@pytest.mark.parametrize("ns", [4, 5, 60, 100])
def test_resample_against_scipy(gcpx_lib, planned, gold, ns):
    T = 100
    for cases in (("a", "b", "c", "e"), ("d",)):
        o = planned[cases[0]][0]
        B, cap = o["B"], o["cap"]
        plan = torch.full((B, T, 2), 5., dtype=torch.float64, device=DEV)
        ok = torch.full((B,), -1, dtype=torch.int32, device=DEV)
        st = torch.full((B, T + 1, 5), 5., dtype=torch.float32, device=DEV)
        ac = torch.full((B, T, 2), 5., dtype=torch.float32, device=DEV)
        pm = torch.full((B, T + 1), 5., dtype=torch.float32, device=DEV)
        n_vert = o["n_vert"].clamp(min=0)                   # case e: no path
        steps = torch.full((B,), ns, dtype=torch.int32, device=DEV)
        rt.check(gcpx_lib.gcpx_prm_resample(o["node_xy"].data_ptr(), o["n_nodes"].data_ptr(), o["path"].data_ptr(), n_vert.data_ptr(),
                                            steps.data_ptr(), o["sg"].data_ptr(), B, cap, T, plan.data_ptr(), ok.data_ptr(), st.data_ptr(),
                                            ac.data_ptr(), pm.data_ptr(), rt.current_stream()), "resample")
        torch.cuda.synchronize()
        for i, c in enumerate(cases):
            if c == "e":
                assert int(ok[i]) == 0 and (plan[i] == 0).all() and (st[i] == 0).all() and (ac[i] == 0).all() and (pm[i] == 0).all()
                continue
            want = gold[f"case_{c}/spline_{ns}"]
            bound = max(100.0 * float(gold[f"case_{c}/spline_route_diff"]), 1e-12)
            got = plan[i].cpu().numpy()
            err = np.abs(got[:ns] - want).max()
            print(f"case {c} n_steps {ns}: max |plan - splev| = {err:.3e}, bound {bound:.3e}")
            assert int(ok[i]) == 1 and err <= bound and (got[ns:] == 0).all()
            sg = gold[f"case_{c}/start_goal"]
            es, ea, ep = NG.episode_numpy(got[:ns], sg[2:], T)
            assert np.array_equal(pm[i].cpu().numpy(), ep) and np.array_equal(ac[i].cpu().numpy(), ea)
            s = st[i].cpu().numpy()
            assert np.array_equal(s[:, [0, 1, 3, 4]], es[:, [0, 1, 3, 4]]) and np.abs(s[:, 2] - es[:, 2]).max() <= 1e-6


def test_resample_rejects_what_splprep_rejects(gcpx_lib, planned):
    o = planned["a"][0]
    B, cap, T = o["B"], o["cap"], 16
    plan = torch.zeros(B, T, 2, dtype=torch.float64, device=DEV)
    ok = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    path = o["path"].clone()
    path[1, 3] = path[1, 2]                                  # case b: a repeated vertex
    path[2, 1] = cap + 5                                     # case c: an index outside the nodes
    n_vert = o["n_vert"].clamp(min=0)
    n_vert[0] = 3                                            # case a: fewer than 4 vertices
    steps = torch.full((B,), 10, dtype=torch.int32, device=DEV)
    rt.check(gcpx_lib.gcpx_prm_resample(o["node_xy"].data_ptr(), o["n_nodes"].data_ptr(), path.data_ptr(), n_vert.data_ptr(),
                                        steps.data_ptr(), None, B, cap, T, plan.data_ptr(), ok.data_ptr(), None, None, None,
                                        rt.current_stream()), "resample")
    torch.cuda.synchronize()
    assert ok.tolist() == [0, 0, 0, 0] and (plan == 0).all()


def sample(lib, boxes, tabs, keys, draw0, seed):
    off = np.zeros(len(tabs) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(t) for t in tabs])
    total = int(off[-1])
    px, py = torch.full((total,), 9., dtype=torch.float64, device=DEV), torch.full((total,), 9., dtype=torch.float64, device=DEV)
    t = [dev(boxes), dev(np.concatenate(tabs).astype(np.int32)), dev(off), dev(np.array(keys, dtype=np.int64)), dev(np.array(draw0, dtype=np.int32))]
    rt.check(lib.gcpx_prm_sample_points(t[0].data_ptr(), boxes.shape[0], t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), t[4].data_ptr(),
                                        len(tabs), total, int(np.diff(off).max()), seed, px.data_ptr(), py.data_ptr(), rt.current_stream()),
             "sample_points")
    torch.cuda.synchronize()
    return px.cpu().numpy(), py.cpu().numpy(), off


def test_point_sampler(gcpx_lib):
    L, rb = NL.layout(3), NL.RoomBoxes(3)
    boxes = rb.box_table(L.doors)
    rs = np.random.RandomState(0)
    tabs = [rs.randint(0, boxes.shape[0], size=n).tolist() for n in (300, 1, 65, 256, 257, 40, 513)]
    keys, draw0 = [5, 6, 7, 8, 9, 10, 1 << 40], [0, 3, 0, 2048, 0, 7, 0]
    px, py, off = sample(gcpx_lib, boxes, tabs, keys, draw0, seed=11)
    for i, tab in enumerate(tabs):
        b = boxes[np.array(tab)]
        x, y = px[off[i]:off[i + 1]], py[off[i]:off[i + 1]]
        assert (np.abs(x - b[:, 0]) <= b[:, 2] / 2).all() and (np.abs(y - b[:, 1]) <= b[:, 3] / 2).all()      # inside its room's / door's box
        wx, wy = NG.sample_points_numpy(boxes, tab, keys[i], draw0[i], 11)
        assert np.array_equal(x, wx) and np.array_equal(y, wy)                                              # the numpy restatement, bit for bit
        x1, y1, _ = sample(gcpx_lib, boxes, [tab], [keys[i]], [draw0[i]], seed=11)                          # alone: batch 1 against 7
        assert np.array_equal(x1, x) and np.array_equal(y1, y)
    same_box = [[0] * 64, [0] * 64]
    qx, qy, _ = sample(gcpx_lib, boxes, same_box, [1, 2], [0, 0], seed=11)
    assert len(np.unique(qx)) == 128 and len(np.unique(qy)) == 128                                          # other indices, other points
    rx, _, _ = sample(gcpx_lib, boxes, same_box, [1, 2], [0, 0], seed=12)
    assert not np.array_equal(rx, qx)
    zero = [[L.n_rooms + 2 * len(L.doors) - 1] * 3]                                                          # sample_door_center: the centre itself
    zx, zy, _ = sample(gcpx_lib, boxes, zero, [1], [0], seed=11)
    assert (zx == boxes[-1, 0]).all() and (zy == boxes[-1, 1]).all()


def test_invalid_arguments_are_rejected(gcpx_lib):
    lib = gcpx_lib
    assert lib.gcpx_prm_sample_points(None, 0, None, None, None, None, 0, 0, 0, 0, None, None, None) == -1
    assert lib.gcpx_prm_shortest_path(None, None, None, 1, 8, 10, 2.0, None, None, None, None, None) == -1
    t = torch.zeros(64, dtype=torch.float64, device=DEV).data_ptr()
    assert lib.gcpx_prm_roadmap(t, t, t, 1, 1, 1, 0., 0., 0.025, t, t, t, t, 1, 4, 4, NG.PRM_MAX_NODES + 1, 10, 0.02, 0.1, t, t, t, t, None) == -1
    assert b"cap" in lib.gcpx_last_error()
    assert lib.gcpx_prm_roadmap(t, t, t, 1, 1, 1, 0., 0., 0.02, t, t, t, t, 1, 4, 4, 6, 10, 0.02, 0.1, t, t, t, t, None) == -1   # cell <= rr
    assert lib.gcpx_prm_resample(t, t, t, t, t, None, 1, 8, 16, t, t, t, None, None, None) == -1


@pytest.fixture(scope="module")
def dataset_dir(tmp_path_factory):
    root = tmp_path_factory.mktemp("nav9")
    res = NG.write_dataset(str(root), 24, n_rooms=9, T=100, seed=4, traj_per_file=2, split=(0.5, 0.25, 0.25), device=DEV)
    return str(root), res


def test_end_to_end_dataset(gcpx_lib, dataset_dir, tmp_path):
    from video_gcp_amd import dataset as D
    root, res = dataset_dir
    T, L = 100, NL.layout(3)
    gen = NG.NavGenerator(9, T=T, seed=4, device=DEV)
    full = gen.generate(24, keep_paths=True)
    for k in ("states", "actions", "pad_mask", "n_steps", "start_goal"):
        assert torch.equal(full[k], res[k]), k               # a second run with the same seed: the same bits
    assert torch.equal(gen.generate(5)["states"], res["states"][:5])      # and a trajectory does not depend on its batch-mates
    st, ac, pm, ns = (full[k].cpu().numpy() for k in ("states", "actions", "pad_mask", "n_steps"))
    sg, nv, pxy = full["start_goal"].cpu().numpy(), full["n_vert"].cpu().numpy(), full["path_xy"].cpu().numpy()
    for j in range(24):
        length, _ = NL.compute_shortest_path(3, sg[j, :2], sg[j, 2:])
        n = int(ns[j])
        assert n == min(int(length * 20), T) and n >= 2
        f32 = lambda v: np.asarray(v, dtype=np.float64).astype(np.float32)
        ulp = 2.0 ** -20                                     # of a float32 below 16: the stored states' rounding
        assert np.abs(st[j, 0, :2] - f32([27 * sg[j, 0], -27 * sg[j, 1]])).max() <= ulp      # starts at its start
        assert np.abs(st[j, n - 1, :2] - f32([27 * sg[j, 2], -27 * sg[j, 3]])).max() <= ulp  # ends at its goal
        assert np.array_equal(st[j, n, :2], st[j, n - 1, :2]) and (st[j, n + 1:] == 0).all()
        assert np.array_equal(st[j, :n + 1, 3:], np.tile(f32([27 * sg[j, 2], -27 * sg[j, 3]]), (n + 1, 1)))
        assert pm[j].tolist() == [1.] * (n + 1) + [0.] * (T - n) and (ac[j, n - 1:] == 0).all()
        assert np.abs(ac[j, :n - 1] - np.diff(st[j, :n, :2].astype(np.float64), axis=0)).max() <= 2 * ulp     # two rounded states and the rounded action
        m = int(nv[j])
        assert m >= 4 and np.array_equal(pxy[j, 0], sg[j, :2]) and np.array_equal(pxy[j, m - 1], sg[j, 2:]) and (pxy[j, m:] == 0).all()
        assert NG.path_is_free_numpy(pxy[j, :m, 0], pxy[j, :m, 1], L.ox, L.oy, L.robot_size, 0.1)
    # the tree is what VideoDataset opens, and the existing top-down assembly renders a batch of it
    spec = D.load_spec(root)
    ds = D.VideoDataset(root, spec, "train", img_sz=32)
    assert ds.topdown is not None and ds.T == T and len(ds) == 12 and ds.traj_per_file == 2
    items = [ds.item(i, D.item_rng(0, 0, i)) for i in range(4)]
    want = D.assemble_numpy(items, ds.T, img_sz=32, topdown=ds.topdown)
    B, S, A = 4, 2, 2
    coords = np.zeros(B * T * 2 + B * 2, dtype=np.int32)
    aux = np.zeros(B * T + B * T * S + B * (T - 1) * A, dtype=np.float32)
    info = np.zeros((B, D.N_INFO), dtype=np.int32)
    for j, it in enumerate(items):
        D.pack_item(it, j, coords, aux, info, B, T, S, A, topdown=ds.topdown)
    out = dict(traj_seq=torch.empty(B, T, 3, 32, 32, device=DEV), I_0=torch.empty(B, 3, 32, 32, device=DEV),
               I_g=torch.empty(B, 3, 32, 32, device=DEV), pad_mask=torch.empty(B, T, device=DEV), end_ind=torch.empty(B, dtype=torch.int64, device=DEV),
               start_ind=torch.empty(B, dtype=torch.int64, device=DEV), traj_seq_states=torch.empty(B, T, S, device=DEV),
               actions=torch.empty(B, T - 1, A, device=DEV))
    D.topdown_assemble_into(gcpx_lib, D.topdown_device_assets(ds.topdown, 32, DEV), dev(coords), dev(aux), dev(info), dev(D.LUT), None, None,
                            out, S, A, rt.current_stream())
    torch.cuda.synchronize()
    assert np.array_equal(out["traj_seq"].cpu().numpy(), want["traj_seq"])
    assert np.array_equal(out["traj_seq_states"].cpu().numpy(), want["traj_seq_states"])
    assert float(out["traj_seq"].std()) > 0.05               # rooms, walls and dots: not a blank picture
    # byte-identical files from a second writer
    NG.write_dataset(str(tmp_path), 24, n_rooms=9, T=100, seed=4, traj_per_file=2, split=(0.5, 0.25, 0.25), device=DEV)
    names = sorted(os.listdir(os.path.join(root, "hdf5")))
    assert len(names) == 12 and names == sorted(os.listdir(os.path.join(str(tmp_path), "hdf5")))
    for name in names:
        with np.load(os.path.join(root, "hdf5", name)) as a, np.load(os.path.join(str(tmp_path), "hdf5", name)) as b:
            assert a.files == b.files and all(a[k].tobytes() == b[k].tobytes() for k in a.files)


def test_trainer_runs_on_a_generated_dataset(tmp_path):
    """`gen_nav` then `train --path EXP --data_dir DIR`, with no flag and nothing converted"""
    from video_gcp_amd import dataset as D
    from video_gcp_amd import gen_nav
    from video_gcp_amd.train import ModelTrainer, get_cmd_args
    data, exp = tmp_path / "data", tmp_path / "exp"
    assert gen_nav.main(["--n_rooms", "9", "--n_traj", "20", "--T", "20", "--out", str(data), "--seed", "2", "--split", "0.6,0.2,0.2"]) == 0
    exp.mkdir()
    (exp / "conf.json").write_text('{"config": "c1", "num_epochs": 1, "epoch_cycles_train": 1}')
    mt = ModelTrainer(get_cmd_args(["--path", str(exp), "--data_dir", str(data), "--log_outputs_interval", "1"]))
    assert isinstance(mt.train_loader, D.HostFedLoader) and mt.train_loader.ds.topdown is not None
    assert mt.train_loader.ds.src_size == (80, 80) and len(mt.train_loader.ds) == 12 and len(mt.val_loader.ds) == 4
    mt.run()
    torch.cuda.synchronize()
    assert mt.global_step == len(mt.train_loader) > 0 and all(np.isfinite(v) for _, v in mt.log)


@pytest.mark.parametrize("n_rooms,params", [(9, dict(use_var_sampling=True, sample_door_center=True)), (16, dict(n_samples_per_door=5, n_knn=5)),
                                            (25, dict(cost_power=1, bottleneck_sampling=True))])
def test_generator_options_and_the_other_layouts(n_rooms, params):
    """variable sampling rates (up to 300 points per room: more than 64 candidates per node), door centres, another n_knn and cost
    power, on the 16- and 25-room mazes: every trajectory is planned, ends at its goal and its vertices pass the collision test"""
    T, rps = 40, NL.rooms_per_side_of(n_rooms)
    L = NL.layout(rps)
    full = NG.NavGenerator(n_rooms, T=T, seed=1, device=DEV, **params).generate(6, keep_paths=True)
    ns, nv = full["n_steps"].cpu().numpy(), full["n_vert"].cpu().numpy()
    sg, pxy, st, pm = (full[k].cpu().numpy() for k in ("start_goal", "path_xy", "states", "pad_mask"))
    assert (ns >= 2).all() and (ns <= T).all() and (nv >= 4).all() and (pm.sum(axis=1) == ns + 1).all()
    for j in range(6):
        assert np.array_equal(pxy[j, 0], sg[j, :2]) and np.array_equal(pxy[j, nv[j] - 1], sg[j, 2:])
        assert np.abs(st[j, ns[j] - 1, :2] - np.array([27 * sg[j, 2], -27 * sg[j, 3]])).max() <= 2.0 ** -19      # |x| < 32: one float32 ulp
        assert NG.path_is_free_numpy(pxy[j, :nv[j], 0], pxy[j, :nv[j], 1], L.ox, L.oy, L.robot_size, 0.1)
