"""-m gpu: the hierarchical search for K tasks per call.

1. every entry point of csrc/tree_search.hip against its torch mirror (tree_latent_search.*_torch) on small tables: K = 3, G in {2, 3},
   T = 12, nz in {8, 128}; lengths from {1, 2, 3, 4, 5, 7, 12}; fixed (row, frame) goals and the raw goal (row = -1); the costs given to the
   selection hold an inf, a NaN that is not first, and a tie.  Everything is a copy, an integer table or one IEEE float32 add: equal, no
   tolerance.
2. HierarchicalCEMPlanner.plan_batch on the c1 model of tests/test_gpu_planning.py (32 x 32, T = 20), K = 3 different start / goal pairs,
   rates [3, 2], 2 dense samples: the recorded draw blocks and rollout rows of task k are replayed into the per-task
   DeviceHierarchicalTreeLatentOptimizer with the learned cost -- populations, per-iteration costs, plans and optimised trees equal bit
   for bit (the cost MLP's rows are independent, csrc/mlp.hip); the K returned plans equal the simulator's rollout of the optimised trees.
   With predicted lengths the length draw is at least 3 frames (gcpx_sample_length's min_len = 2 is an END INDEX, base_gcp.py:219-226),
   so no rollout is shorter than 3 frames; what the walk meets, and the test asserts, are the short halves of 3 .. 5-frame rollouts
   one level down: short candidates, stand-in rows and short alternatives that win.
3. the same tasks, every population rolled out per task instead of together: the latents agree within the tolerance
   test_simulator_rollout_matches_oracle gives the same tensor against the oracle (5e-5 + 1e-4 |x|); the largest difference is printed.
   Bit-equality is NOT asserted here: a forward of K n rows need not equal one of n rows in the last bits.
4. ControlRunner(batch_plans=True): E = 3, 9 rooms, the model and T of tests/test_gpu_nav_env.py, closed and open loop."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from video_gcp_amd import planning as P  # noqa: E402
from video_gcp_amd import runtime as rt  # noqa: E402
from video_gcp_amd import tree_latent_search as TS  # noqa: E402
from video_gcp_amd.model import Outputs  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K, T = 3, 12
LENGTHS = (1, 2, 3, 4, 5, 7, 12)
INF, NAN = float("inf"), float("nan")


def same(a, b):
    a, b = (torch.as_tensor(x).detach().cpu().numpy() for x in (a, b))
    if a.dtype.kind != "f":
        return a.shape == b.shape and a.dtype == b.dtype and bool((a == b).all())
    a, b = a.astype(np.float32), b.astype(np.float32)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def st():
    return rt.current_stream()


@pytest.fixture(scope="module")
def lib():
    return rt.load_library()


# ---- 1. the entry points ------------------------------------------------------------------------------------------------------------------
def tables(G, nz, seed):
    """lat [K G + 1, T, nz] with the stand-in row last; views of the lengths above, some starting inside the rollout, one the stand-in"""
    g = torch.Generator().manual_seed(seed)
    rng = np.random.RandomState(seed)
    lat = torch.randn(K * G + 1, T, nz, generator=g)
    lat[-1] = 0
    lat[-1, 0] = lat[-1, 2] = INF
    lens = rng.choice(LENGTHS, size=K * G)
    lens[:6] = (1, 12, 2, 3, 5, 7)                        # the shortest and the longest among them
    a = np.array([rng.randint(0, T - l + 1) for l in lens])
    views = np.stack([np.arange(K * G), a, a + lens], -1).astype(np.int32).reshape(K, G, 3)
    views[1, G - 1] = (K * G, 0, 3)                       # the stand-in row as a candidate
    fixed = np.array([[0, 3], [K * G, 1], [2, T - 1]], dtype=np.int32)
    raw = np.full((K, 2), -1, dtype=np.int32)
    return lat, torch.from_numpy(views), torch.from_numpy(fixed), torch.from_numpy(raw)


@pytest.mark.parametrize("G,nz", [(2, 8), (3, 8), (2, 128), (3, 128)])
def test_subgoal_rows_and_segment_windows_equal_their_mirrors(lib, G, nz):
    lat, views, fixed, raw = tables(G, nz, 10 * G + nz)
    latd, vd = lat.to(DEV), views.to(DEV)
    for goal in (fixed, raw):
        gd = goal.to(DEV)
        opa, opb = torch.full((2 * K * G, nz), -7.0, device=DEV), torch.full((2 * K * G, nz), -7.0, device=DEV)
        mids = torch.full((K, G), -7, dtype=torch.int32, device=DEV)
        rt.check(lib.gcpx_tree_subgoal_rows(latd.data_ptr(), vd.data_ptr(), gd.data_ptr(), opa.data_ptr(), opb.data_ptr(), mids.data_ptr(),
                                            K, G, latd.shape[0], T, nz, st()), "tree_subgoal_rows")
        wa, wb, wm = TS.subgoal_rows_torch(lat, views, goal)
        assert same(opa, wa) and same(opb, wb) and same(mids, wm)
        assert (wm == 0).any() and (wm > 0).any()                              # a one-frame view among them
        for tmax in (T, 2):                                                    # the dense bottom's window and the short alternative's
            seg = torch.full((K * G, tmax, nz), -7.0, device=DEV)
            lens, rows = torch.full((K * G,), -7, dtype=torch.int32, device=DEV), torch.full((K * G, nz), -7.0, device=DEV)
            rt.check(lib.gcpx_tree_segment_windows(latd.data_ptr(), vd.data_ptr(), gd.data_ptr(), seg.data_ptr(), lens.data_ptr(),
                                                   rows.data_ptr(), K, G, latd.shape[0], T, tmax, nz, st()), "tree_segment_windows")
            ws, wl, wr = TS.segment_windows_torch(lat, views, goal, tmax)
            assert same(seg, ws) and same(lens, wl) and same(rows, wr)
            assert int(wl.max()) == min(tmax, 12) and int(wl.min()) == 1


@pytest.mark.parametrize("G", [2, 3])
def test_split_views_equals_its_mirror(lib, G):
    _, views, _, _ = tables(G, 8, 3 + G)
    vd = views.to(DEV)
    left, right = torch.full_like(vd, -7), torch.full_like(vd, -7)
    lgoal, short = torch.full((K, 2), -7, dtype=torch.int32, device=DEV), torch.full((K, G), -7, dtype=torch.int32, device=DEV)
    rt.check(lib.gcpx_tree_split_views(vd.data_ptr(), K * G, left.data_ptr(), right.data_ptr(), lgoal.data_ptr(), short.data_ptr(), K, G, st()),
             "tree_split_views")
    wl, wr, wg, ws = TS.split_views_torch(views, K * G)
    assert same(left, wl) and same(right, wr) and same(lgoal, wg) and same(short, ws)
    assert ws.any() and not ws.all() and ws[0, 0] == 1 and wg[0].tolist() == [K * G, 1]      # task 0's first candidate is short: its goal is the stand-in's


def test_select_equals_its_mirror(lib):
    G, zf = 3, 3 * 8
    c1 = torch.tensor([[1.0, 0.5, 0.25], [INF, 1.0, 2.0], [0.5, NAN, NAN]])
    c2 = torch.tensor([[0.5, 0.25, 0.5], [1.0, NAN, 0.0], [0.5, 1.0, 0.0]])      # totals: a tie (0.75, 0.75), [inf, nan, 2], [1, nan, nan]
    draw = torch.randn(K, G, zf, generator=torch.Generator().manual_seed(0))
    masks = [None, torch.tensor([[1, 0, 1], [1, 0, 1], [0, 0, 0]], dtype=torch.int32)]
    for second in (c2, None):
        for mask in masks:
            for d in (draw, None):
                if mask is not None and d is not None:
                    continue                                                    # the walk never masks a level's own draw
                idx, cost = torch.full((K,), -7, dtype=torch.int32, device=DEV), torch.full((K,), -7.0, device=DEV)
                best = None if d is None else torch.full((K, zf), -7.0, device=DEV)
                dev = lambda x: None if x is None else x.to(DEV)
                a, b, m, dd = c1.to(DEV), dev(second), dev(mask), dev(d)
                rt.check(lib.gcpx_tree_select(a.data_ptr(), rt.ptr(b), rt.ptr(m), rt.ptr(dd), rt.ptr(best), idx.data_ptr(), cost.data_ptr(),
                                              K, G, zf, st()), "tree_select")
                wi, wc, wb = TS.select_torch(c1, second, mask, d)
                assert same(idx, wi) and same(cost, wc), (second is None, mask, idx, wi, cost, wc)
                if d is not None:
                    assert same(best, wb)
                if mask is None:                                                # numpy's argmin is the definition
                    total = (c1 if second is None else c1 + second).numpy()
                    assert wi.tolist() == [int(np.argmin(r)) for r in total]
    wi, _, _ = TS.select_torch(c1, c2)
    assert wi.tolist() == [1, 1, 1]                                             # the tie's first, the NaN behind an inf, the first of two NaN


def test_short_alternative_equals_its_mirror(lib):
    lc = torch.tensor([1.0, 1.0, NAN, NAN, INF, 2.0, 0.5])
    rc = torch.tensor([1.0, 1.0, 1.0, 1.0, 1.0, -INF, 0.25])
    sc = torch.tensor([1.5, 2.0, 3.0, 3.0, 7.0, 1.0, 0.75])
    sidx = torch.tensor([0, 1, 2, -1, 0, 1, 0], dtype=torch.int32)
    n = lc.shape[0]
    cost, use = torch.full((n,), -7.0, device=DEV), torch.full((n,), -7, dtype=torch.int32, device=DEV)
    d = [x.to(DEV) for x in (lc, rc, sc, sidx)]
    rt.check(lib.gcpx_tree_short_alternative(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), cost.data_ptr(), use.data_ptr(),
                                             n, st()), "tree_short_alternative")
    wc, wu = TS.short_alternative_torch(lc, rc, sc, sidx)
    assert same(cost, wc) and same(use, wu)
    assert wu.tolist() == [1, 0, 1, 0, 1, 0, 0]           # lower; equal; NaN; NaN without a short candidate; inf; -inf; a tie keeps the children


def test_entry_points_refuse_bad_arguments(lib):
    x = torch.zeros(64, device=DEV)
    p = x.data_ptr()
    assert lib.gcpx_tree_subgoal_rows(None, p, p, p, p, p, 1, 1, 1, 1, 4, st()) == -1 and b"gcpx_tree_subgoal_rows" in lib.gcpx_last_error()
    assert lib.gcpx_tree_subgoal_rows(p, p, p, p, p, p, 1, 1, 1, 1, 6, st()) == -1
    assert lib.gcpx_tree_select(p, None, None, p, None, p, p, 1, 1, 4, st()) == -1 and lib.gcpx_tree_select(p, None, None, p, p, p, p, 1, 1, 6, st()) == -1
    assert lib.gcpx_tree_split_views(p, -1, p, p, p, p, 1, 1, st()) == -1 and lib.gcpx_tree_split_views(p, 0, p, p, p, None, 1, 1, st()) == -1
    assert lib.gcpx_tree_segment_windows(p, p, p, p, p, p, 1, 1, 1, 1, 0, 4, st()) == -1
    assert lib.gcpx_tree_short_alternative(p, p, p, p, p, p, 0, st()) == -1
    torch.cuda.synchronize()
    assert (x == 0).all()


# ---- 2., 3. the search on real rollouts -------------------------------------------------------------------------------------------------
class ReplayGenerator(np.random.Generator):
    """hands out recorded blocks instead of drawing"""

    def __init__(self, blocks):
        super().__init__(np.random.PCG64(0))
        self.blocks = list(blocks)

    def standard_normal(self, size=None, dtype=np.float64, out=None):
        b = self.blocks.pop(0)
        assert tuple(size) == b.shape and dtype == np.float32, (size, b.shape, dtype)
        return b.copy()


@pytest.fixture(scope="module")
def setup():
    import video_gcp_amd as V
    from video_gcp_amd.model import GCPTreeModel
    hp = V.config("c1")
    model = GCPTreeModel(hp, params=V.init_params(hp, seed=1, randomize_affine=True), device="cuda")
    model.eval()
    rng = np.random.RandomState(21)
    states, goals = (rng.randint(0, 256, size=(K, hp.img_sz, hp.img_sz, 3)).astype(np.uint8) for _ in range(2))
    return hp, model, states, goals


def _planner(hp, model, pred_length):
    return P.HierarchicalCEMPlanner(P.GCPImageSimulator(model, pred_length=pred_length), P.LearnedCostEstimate(model), hp.hierarchy_levels,
                                    [3, 2], n_ll_samples=2, action_dim=hp.nz_vae, max_seq_len=hp.max_seq_len, fast_draws=True, seed=7)


def _len_u(rows):
    """length draws that reach the shortest rollouts (the low end of the inverse CDF) and long ones alike"""
    return torch.tensor([0.001, 0.03, 0.5, 0.08, 0.97, 0.12])[torch.arange(rows) % 6]


@pytest.fixture(scope="module")
def batches(setup):
    """plan_batch(record=True) of the K tasks at fixed and at predicted lengths, and at fixed lengths with at most 2 rows per forward
    (one task per scoring forward, the final rollouts in two): {(pred_length, max_rows): (planner, plans)}"""
    hp, model, states, goals = setup
    res = {}
    for pred_length, max_rows in CASES:
        planner = _planner(hp, model, pred_length)
        assert isinstance(planner._sampler._rng, torch.Generator)
        res[pred_length, max_rows] = (planner, planner.plan_batch(states, goals, record=True, max_rows=max_rows,
                                                                  len_u=_len_u if pred_length else None))
    return res


CASES = [(False, None), (True, None), (False, 2)]


@pytest.mark.parametrize("pred_length,max_rows", CASES)
def test_plan_batch_equals_the_per_task_search_on_its_own_rollouts(setup, batches, pred_length, max_rows):
    hp, model, states, goals = setup
    planner, out = batches[pred_length, max_rows]
    rec = planner.batch_record
    opt, cost = rec.optimizer, P.LearnedCostEstimate(model)
    pops = (3, 2, 2)
    assert len(out) == K and opt.fully_optimized and [p.shape[1] for p in rec.populations] == list(pops)
    for k in range(K):
        chk = TS.DeviceHierarchicalTreeLatentOptimizer(hp.nz_vae, [3, 2], hp.hierarchy_levels, cost, cost, 2,
                                                       rng=ReplayGenerator([b[k].cpu().numpy() for b in rec.draws]))
        for it, n in enumerate(pops):
            assert same(chk.sample(), rec.populations[it][k]), (k, it)
            lat, lens = rec.rollouts[it]
            plan, c = chk.optimize(Outputs(latents=lat[k * n:(k + 1) * n], lengths=lens[k * n:(k + 1) * n]))
            print(f"task {k} iteration {it}: cost {float(c)!r} batched {float(opt.costs[it][k])!r}")
            assert same(np.float32(c), opt.costs[it][k]), (k, it, c, opt.costs[it][k])
            assert [(int(i), int(t)) for i, t in plan] == opt.plans(it)[k], (k, it)
        assert not chk._rng.blocks and chk.fully_optimized
        assert same(chk.sample()[0], rec.best_samples[k]), k
        assert out[k].cost == float(opt.costs[-1][k])
    lens = torch.cat([l for _, l in rec.rollouts]).cpu().numpy()
    kinds = [(kind, t) for decisions in opt.tables() for kind, t in decisions]
    short = [(t["views"][..., 2] - t["views"][..., 1]) < 3 for kind, t in kinds if kind == "children"]
    if pred_length:
        # the shortest length draw is 3 frames: its halves are the short candidates of the level below
        assert lens.min() == 3 and lens.max() > 5 and len(set(lens.tolist())) > 2, lens
        assert any(s.any() for s in short) and any(t["use"].any() for kind, t in kinds if kind == "children")
        assert any((t["mids"] == 0).any() for kind, t in kinds if kind == "subgoal")
    else:
        assert (lens == hp.max_seq_len).all() and not any(s.any() for s in short)
    # the K returned plans: the simulator's own rollout of the optimised trees
    # (max_rows tasks per forward, as plan_batch rolls them out)
    best = rec.best_samples.cpu().numpy()
    for lo in range(0, K, max_rows or K):
        hi = min(lo + (max_rows or K), K)
        kw = dict(len_u=_len_u(hi - lo)) if pred_length else {}
        direct = planner._sim.rollout(states[lo:hi], goals[lo:hi], best[lo:hi], hp.max_seq_len, **kw)
        for k in range(lo, hi):
            assert np.array_equal(out[k].predictions, direct.predictions[k - lo]) and np.array_equal(out[k].latents, direct.latents[k - lo])
            assert np.array_equal(out[k].actions, direct.actions[k - lo]) and np.array_equal(out[k].states, direct.states[k - lo])
            assert out[k].predictions.shape[1] == 3 * hp.img_sz ** 2 + hp.nz_enc and np.isfinite(out[k].cost)
    assert not np.array_equal(out[0].predictions[0], out[1].predictions[0])       # different tasks, different plans


def test_batched_rollouts_against_rollouts_per_task(setup, batches):
    """a report with a loose bound, not bit-equality: each population rolled out for its task alone against its rows in the batch
    (fixed lengths)"""
    from helpers import assert_close
    hp, model, states, goals = setup
    planner, out = batches[False, None]
    rec = planner.batch_record
    worst = 0.0
    for it, pop in enumerate(rec.populations):
        n = pop.shape[1]
        for k in range(K):
            alone = planner._sim.rollout_device(states[k:k + 1], goals[k:k + 1], pop[k], hp.max_seq_len, decode=False).latents
            together = rec.rollouts[it][0][k * n:(k + 1) * n]
            worst = max(worst, float((alone - together).abs().max()))
            assert_close(together, alone, 5e-5, 1e-4, f"latents, task {k} iteration {it}")
    print(f"rollout latents, K n rows per forward against n rows per forward: max |difference| = {worst!r}")


# ---- 4. the runner ---------------------------------------------------------------------------------------------------------------------------
class ShortPlans:
    """a planner whose plans are cut to n frames, so that every episode has to plan again; counts both kinds of call"""

    def __init__(self, planner, n):
        self.planner, self.n, self.single_calls, self.batch_calls = planner, n, 0, []

    def __call__(self, state, goal):
        self.single_calls += 1
        img, act, lat, cost = self.planner(state, goal)
        return img[:self.n], act[:self.n - 1], lat[:self.n], cost

    def plan_batch(self, states, goals):
        self.batch_calls.append(len(states))
        return [Outputs(predictions=r.predictions[:self.n], actions=r.actions[:self.n - 1], latents=r.latents[:self.n], cost=r.cost)
                for r in self.planner.plan_batch(states, goals)]


@pytest.fixture(scope="module")
def small_model():
    from test_gpu_nav_env import HP
    from video_gcp_amd.model import GCPTreeModel
    from video_gcp_amd.params import init_params
    n = GCPTreeModel._n_models
    m = GCPTreeModel(HP, params=init_params(HP, seed=0), device=torch.device("cuda", 0))
    m.eval()
    yield m
    GCPTreeModel._n_models = max(n, GCPTreeModel._n_models) + 8      # later modules' models: streams none of these used


@pytest.mark.parametrize("closed_loop", [True, False])
def test_runner_with_batched_plans(small_model, closed_loop):
    from test_gpu_nav_env import CW, IMG, T as TE, Replay, _frames_numpy
    from video_gcp_amd import control as CT
    from video_gcp_amd import dataset as DS
    from video_gcp_amd import nav_env as NE
    model, E = small_model, 3
    planner = ShortPlans(P.HierarchicalCEMPlanner(P.GCPImageSimulator(model), P.LearnedCostEstimate(model), 4, [3, 3], n_ll_samples=5,
                                                  action_dim=32, max_seq_len=12, fast_draws=True, seed=1), 4)
    env = NE.NavEnvBatch(9, CW, TE, IMG, DEV)
    runner = CT.ControlRunner(model, planner, env, replan_interval=TE + 2, num_max_replans=10, closed_loop_execution=closed_loop, batch_plans=True)
    tasks = NE.draw_tasks(9, 2, range(E))
    res = runner.run(tasks)
    assert res["full_traj"].shape == (E, TE + 1, 3) and res["actions"].shape == (E, TE, 2) and np.isfinite(res["actions"]).all()
    frames, goal_frames = env.frames.cpu().numpy(), env.goal_frames.cpu().numpy()
    goal_pix = DS.topdown_pixels(tasks["goal"], 9, env.scale, env.S, env.cw)
    for t in range(TE + 1):
        assert np.array_equal(frames[:, t], _frames_numpy(env, res["full_traj"][:, t], goal_pix)), t
    steps = {}
    for e in range(E):
        ref = NE.rollout_numpy(9, tasks["start"][e], tasks["goal"][e], res["actions"][e])
        assert np.array_equal(ref["full_traj"].view(np.uint32), res["full_traj"][e].view(np.uint32))
        replay = Replay(runner.plans[e], frames[e])
        policy = P.ImageCEMPolicy(model, replay, replan_interval=TE + 2, num_max_replans=10, closed_loop_execution=closed_loop)
        planned_at = []
        for t in range(TE):
            before = replay.calls
            a = np.asarray(policy.act(t=t, i_tr=0, images=frames[e, :t + 1], goal_image=goal_frames[e][None]).actions, dtype=np.float32)
            if replay.calls != before:
                planned_at.append(t)
            assert np.array_equal(a.view(np.uint32), res["actions"][e, t].view(np.uint32)), (e, t, a, res["actions"][e, t])
        assert planned_at == [p["t"] for p in runner.plans[e]] and replay.calls == len(runner.plans[e]) == res["n_replans"][e]
        assert planned_at[0] == 0 and len(planned_at) >= 2
        for t in planned_at:
            steps[t] = steps.get(t, 0) + 1
    # one plan_batch call per step at which anybody planned, carrying everybody who did; no per-episode call
    assert planner.single_calls == 0 and planner.batch_calls == [steps[t] for t in sorted(steps)] and max(planner.batch_calls) > 1
    # the flag off on the same runner: a planner call per episode and plan, as before
    runner.batch_plans = False
    n_batch = len(planner.batch_calls)
    res = runner.run(tasks)
    assert len(planner.batch_calls) == n_batch and planner.single_calls == int(res["n_replans"].sum()) >= 2 * E


def test_control_main_with_batched_plans(tmp_path):
    from nav_env_cases import CONF
    from test_gpu_nav_env import CW, T as TE
    from video_gcp_amd import control as CT
    conf = tmp_path / "mod_hyper.py"
    conf.write_text(CONF.format(env_params="n_rooms=9, crop_window=40, heading_smoothing=0.1, init_pos=None, goal_pos=None",
                                env_cls="TopdownMultiroom3dEnv", T=TE))
    out = str(tmp_path / "out")
    argv = ["--experiment", str(conf), "--data_dir", str(tmp_path / "data"), "--exp_dir", str(tmp_path / "exp"), "--random_weights", "1",
            "--n_tasks", "2", "--task_seed", "3", "--out", out, "--batch_plans", "1"]
    with pytest.raises(ValueError, match="reference_rng"):
        CT.main(argv + ["--reference_rng"])
    res = CT.main(argv)
    n = 2
    shapes = dict(improvement=(n,), initial_dist=(n,), final_dist=(n,), all_goal_distances=(n, TE + 1), full_traj=(n, TE + 1, 3), goal=(n, 2),
                  path_len=(n,), blocked=(n, TE), reset_state=(n, 5), term_t=(n,), actions=(n, TE, 2))
    with np.load(os.path.join(out, "control_results.npz")) as z:
        assert set(shapes) <= set(z.files)
        for k, shape in shapes.items():
            assert z[k].shape == shape and np.array_equal(z[k], res[k]), k
        assert np.isfinite(z["actions"]).all()
