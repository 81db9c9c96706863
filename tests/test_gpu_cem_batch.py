"""-m gpu: the flat CEM planner for K tasks per call (csrc/cem_batch.hip, planning.CEMPlanner.plan_batch).

1. every entry point of csrc/cem_batch.hip against its torch mirror (planning.cem_*_torch, computed on CPU tensors: torch's device kernels
   may divide by a scalar through its reciprocal), equal bit for bit.  K = 3; n in {5, 70} (70 crosses a wave and is no multiple of 64)
   and 300 for the elites (a thread ranks more than one score); n_elite in {1, 7, n}; D in {2, 38, 260, 1100}: no alignment, a column
   tail past one 256-wide block, and past one 1024-column population chunk; clip in {0.5, inf}; the population in place; scores with a
   tie, -0.0 beside +0.0, both infinities, NaNs that are not first and an all-NaN row; an elite index out of range handed to the refit;
   bad arguments.
2. CEMPlanner.plan_batch on the c1 model of tests/test_gpu_planning.py (32 x 32, T = 20), K = 3 different start / goal pairs,
   SimpleTreeCEMSampler, batch_size 6, elite_frac 0.5, 2 iterations, the learned cost; fixed and predicted lengths, max_rows None and 6 (one
   task per forward).  Each task is replayed from the record: its noise block through FlatCEMSampler.from_unit_noise, its scores from its
   recorded rollout rows through the cost on the device (the cost MLP's rows are independent, csrc/mlp.hip), the elites by
   `select_elites`, the refit by the mirror: populations, scores, elites, refits and `best` equal bit for bit; the K returned plans equal
   sim.rollout of the `best` rows.  With predicted lengths and no len_u the draws are the sampler's own: a generator seeded alike and
   asked for the same blocks in the same order reproduces the noise and the final rollout's lengths.
3. the same with L2ImageCost and a goal image per task: gcpx_rollout_cost gives every candidate a workgroup of its own, which reads that
   candidate's rows and goal only (csrc/misc.hip: rollout_cost_kernel), so per-row goals give the bits rollout_cost_device gives task
   by task on the same rows.
4. K = 2 with ActCondGCPImageSimulator: the samples are action sequences, D = 2 (T - 1).
5. every population rolled out per task instead of together: the latents agree within 5e-5 + 1e-4 |x|, the tolerance
   test_simulator_rollout_matches_oracle gives this tensor; the largest difference is printed.  No bit-equality: DESIGN.md 5.7.
6. ControlRunner(batch_plans=True) with the flat planner (E = 3, 9 rooms, closed and open loop), and control.main on a flat conf."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from video_gcp_amd import planning as P  # noqa: E402
from video_gcp_amd import runtime as rt  # noqa: E402
from test_gpu_tree_search import ShortPlans, same  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K = 3
INF, NAN = float("inf"), float("nan")


def st():
    return rt.current_stream()


@pytest.fixture(scope="module")
def lib():
    return rt.load_library()


# ---- 1. the entry points ------------------------------------------------------------------------------------------------------------------
def special_scores(n, seed):
    """[K, n]: row 0 the special values among random ones, row 1 random with a tie, row 2 all NaN"""
    s = torch.randn(K, n, generator=torch.Generator().manual_seed(seed))
    s[0, :5] = torch.tensor([INF, NAN, -0.0, 0.0, -INF])
    if n >= 12:
        s[0, 5:12] = torch.tensor([0.0, NAN, -0.0, INF, -INF, s[0, 12 % n], NAN])
    s[1, n - 1] = s[1, 0]
    s[1, n // 2] = s[1, 0]
    s[2] = NAN
    return s


@pytest.mark.parametrize("n", [5, 70])
@pytest.mark.parametrize("D", [2, 38, 260, 1100])
def test_population_equals_its_mirror(lib, n, D):
    g = torch.Generator().manual_seed(n + D)
    mean, std, eps = torch.randn(K, D, generator=g), torch.rand(K, D, generator=g) + 0.25, torch.randn(K, n, D, generator=g)
    eps[1, n - 1, D - 1], eps[2, 0, 0] = NAN, INF
    md, sd = mean.to(DEV), std.to(DEV)
    for clip in (0.5, INF):
        want = P.cem_population_torch(mean, std, eps, clip)
        ed = eps.to(DEV)
        out = torch.full((K, n, D), -7.0, device=DEV)
        rt.check(lib.gcpx_cem_population(md.data_ptr(), sd.data_ptr(), ed.data_ptr(), clip, out.data_ptr(), K, n, D, st()), "cem_population")
        assert same(out, want) and same(ed, eps)
        rt.check(lib.gcpx_cem_population(md.data_ptr(), sd.data_ptr(), ed.data_ptr(), clip, ed.data_ptr(), K, n, D, st()), "cem_population")
        assert same(ed, want)                                                       # in place
        assert same(P.cem_population(md, sd, eps.to(DEV), clip), want)
        for k in range(K):                                                          # block k: the per-task sampler with task k's distribution
            s = P.FlatCEMSampler(clip, 1, D, 1.0, device="cpu")
            s.mean, s.std = mean[k][None], std[k][None]
            assert same(out[k], s.from_unit_noise(eps[k][:, None])[:, 0])
        assert bool(torch.isnan(want[1, n - 1, D - 1])) and float(want[2, 0, 0]) == clip        # a NaN stays; an infinity is clamped, or stays
        assert not np.isfinite(clip) or float(want[~torch.isnan(want)].abs().max()) == clip


@pytest.mark.parametrize("n,n_elite", [(5, 1), (5, 5), (70, 1), (70, 7), (70, 70), (300, 7), (300, 300)])
def test_elites_equal_their_mirror(lib, n, n_elite):
    scores = special_scores(n, n)
    sd = scores.to(DEV)
    idx, best = torch.full((K, n_elite), -7, dtype=torch.int32, device=DEV), torch.full((K, n_elite), -7.0, device=DEV)
    rt.check(lib.gcpx_cem_elites(sd.data_ptr(), idx.data_ptr(), best.data_ptr(), K, n, n_elite, st()), "cem_elites")
    wi, wb = P.cem_elites_torch(scores, n_elite)
    assert same(idx, wi) and same(best, wb), (idx, wi)
    for k in range(K):
        assert idx[k].tolist() == np.argsort(scores[k].numpy(), kind="stable")[:n_elite].tolist()
    gi, gb = P.cem_elites(sd, n_elite)
    assert same(gi, wi) and same(gb, wb)
    assert idx[2].tolist() == list(range(n_elite)) and idx[0, 0] == 4                # all NaN: by index; -inf first


@pytest.mark.parametrize("n,n_elite", [(5, 1), (5, 5), (70, 1), (70, 7), (70, 70)])
@pytest.mark.parametrize("D", [2, 38, 260, 1100])
def test_refit_equals_its_mirror(lib, n, n_elite, D):
    g = torch.Generator().manual_seed(n * n_elite + D)
    samples = torch.randn(K, n, D, generator=g) * torch.logspace(-2, 2, D)
    samples[1] += 3.0
    idx = torch.stack([torch.randperm(n, generator=g)[:n_elite] for _ in range(K)]).to(torch.int32)

    def run(ix):
        xd, ixd = samples.to(DEV), ix.to(DEV)
        out = [torch.full((K, D), -7.0, device=DEV) for _ in range(3)]
        rt.check(lib.gcpx_cem_refit(xd.data_ptr(), ixd.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), K, n, n_elite, D,
                                    st()), "cem_refit")
        return out
    got, want = run(idx), P.cem_refit_torch(samples, idx)
    for a, b, name in zip(got, want, ("mean", "std", "best")):
        assert same(a, b), (name, float((a.cpu() - b).abs().max()))
    for a, b in zip(P.cem_refit(samples.to(DEV), idx.to(DEV)), want):
        assert same(a, b)
    if n_elite == 1:
        assert bool((got[1] == 0).all()) and same(got[0], got[2])
    # one index out of range, in task 1, last position (too large) or first (negative): NaN for that task alone, no fault
    for pos, val in ((n_elite - 1, n), (0, -1), (0, 2 ** 31 - 1)):
        bad = idx.clone()
        bad[1, pos] = val
        gb, wb = run(bad), P.cem_refit_torch(samples, bad)
        for a, b, ok in zip(gb, wb, got):
            assert same(a, b) and bool(torch.isnan(a[1]).all()) and same(a[0], ok[0]) and same(a[2], ok[2])


def test_entry_points_refuse_bad_arguments(lib):
    x = torch.zeros(64, device=DEV)
    p = x.data_ptr()
    big = 8192 + 1                                                                  # GCPX_CEM_MAX_N + 1
    assert lib.gcpx_cem_population(None, p, p, 1.0, p, 1, 1, 1, st()) == -1 and b"gcpx_cem_population" in lib.gcpx_last_error()
    assert lib.gcpx_cem_population(p, p, p, 1.0, None, 1, 1, 1, st()) == -1 and lib.gcpx_cem_population(p, p, p, 1.0, p, 0, 1, 1, st()) == -1
    assert lib.gcpx_cem_population(p, p, p, 1.0, p, 1, 1, -3, st()) == -1
    assert lib.gcpx_cem_elites(p, p, None, 1, 4, 2, st()) == -1 and b"gcpx_cem_elites" in lib.gcpx_last_error()
    assert lib.gcpx_cem_elites(p, p, p, 1, 4, 5, st()) == -1 and b"n_elite" in lib.gcpx_last_error()
    assert lib.gcpx_cem_elites(p, p, p, 1, 4, 0, st()) == -1 and lib.gcpx_cem_elites(p, p, p, 1, big, 2, st()) == -1
    assert b"GCPX_CEM_MAX_N" in lib.gcpx_last_error()
    assert lib.gcpx_cem_refit(p, None, p, p, p, 1, 4, 2, 4, st()) == -1 and b"gcpx_cem_refit" in lib.gcpx_last_error()
    assert lib.gcpx_cem_refit(p, p, p, p, p, 1, 4, 5, 4, st()) == -1 and lib.gcpx_cem_refit(p, p, p, p, p, 1, 4, 2, 0, st()) == -1
    assert lib.gcpx_cem_refit(p, p, p, p, p, 1, big, 2, 4, st()) == -1
    torch.cuda.synchronize()
    assert (x == 0).all()


# ---- 2. - 5. the planner on real rollouts ------------------------------------------------------------------------------------------------
N_CAND, N_ELITE, N_ITERS, SEED = 6, 3, 2, 7


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


def _len_u(rows):
    """length draws that reach the shortest rollouts (the low end of the inverse CDF) and long ones alike"""
    return torch.tensor([0.001, 0.03, 0.5, 0.08, 0.97, 0.12])[torch.arange(rows) % 6]


def _planner(hp, model, pred_length, cost=None):
    sampler = P.SimpleTreeCEMSampler(2.0, None, hp.nz_vae, 1.0, n_level_hierarchy=hp.hierarchy_levels, device=DEV, seed=SEED)
    return P.CEMPlanner(P.GCPImageSimulator(model, pred_length=pred_length), cost or P.LearnedCostEstimate(model), sampler, n_iters=N_ITERS,
                        batch_size=N_CAND, elite_frac=0.5, max_seq_len=hp.max_seq_len)


# (pred_length, max_rows, the test's own length draws)
CASES = [(False, None, False), (False, 6, False), (True, None, False), (True, 6, True)]


@pytest.fixture(scope="module")
def batches(setup):
    hp, model, states, goals = setup
    res = {}
    for pred_length, max_rows, own in CASES:
        planner = _planner(hp, model, pred_length)
        res[pred_length, max_rows, own] = (planner, planner.plan_batch(states, goals, record=True, max_rows=max_rows, len_u=_len_u if own else None))
    return res


def replay(planner, n_tasks, n, n_elite, score=None):
    """every task of planner.batch_record replayed alone (on CPU tensors but for `score`, which gets the task's recorded rollout rows)"""
    rec, s = planner.batch_record, planner._sampler
    for k in range(n_tasks):
        chk = P.FlatCEMSampler(s._clip_val, s._n_steps, s._action_dim, s._initial_std, device="cpu")
        rows = slice(k * n, (k + 1) * n)
        for it in range(len(rec.noise)):
            pop = chk.from_unit_noise(rec.noise[it][k].cpu())
            assert same(pop, rec.populations[it][k]), (k, it)
            scores = rec.scores[it][k]
            if score is not None:
                (lat, lens), e_goal = rec.rollouts[it], rec.goal_latents[it]
                alone = score(lat[rows].contiguous(), lens[rows].contiguous(), e_goal[rows].contiguous())
                assert same(alone, scores), (k, it, alone, scores)
            scores = scores.cpu()
            idx = P.select_elites(scores, n_elite)
            assert idx.tolist() == rec.elite_idx[it][k].tolist(), (k, it)
            assert same(scores[idx], planner.logs[it].elite_scores[k])
            assert float(planner.logs[it].mean_score[k]) == pytest.approx(float(scores.double().mean()), rel=1e-5)
            mean, std, best = P.cem_refit_torch(pop[None], idx[None].to(torch.int32))
            assert same(mean[0], rec.means[it][k]) and same(std[0], rec.stds[it][k]), (k, it)
            chk.mean, chk.std = mean[0], std[0]
        assert same(best[0], rec.best_samples[k])
    assert [tuple(l.elite_scores.shape) for l in planner.logs] == [(n_tasks, n_elite)] * len(rec.noise)
    assert [tuple(l.mean_score.shape) for l in planner.logs] == [(n_tasks,)] * len(rec.noise)


@pytest.mark.parametrize("pred_length,max_rows,own", CASES)
def test_plan_batch_equals_the_per_task_replay(setup, batches, pred_length, max_rows, own):
    hp, model, states, goals = setup
    planner, out = batches[pred_length, max_rows, own]
    rec, cost = planner.batch_record, P.LearnedCostEstimate(model)
    assert len(out) == K and len(rec.noise) == N_ITERS and tuple(rec.noise[0].shape) == (K, N_CAND, hp.n_nodes, hp.nz_vae)
    replay(planner, K, N_CAND, N_ELITE, score=cost.sequence_cost_device)
    assert float(rec.populations[0].abs().max()) == 2.0                              # the clip was reached
    sampler = planner._sampler
    assert bool((sampler.mean == 0).all()) and bool((sampler.std == 1).all())        # the sampler's own distribution: untouched
    lens = torch.cat([l for _, l in rec.rollouts]).cpu().numpy()
    kw = {}
    if not pred_length:
        assert (lens == hp.max_seq_len).all()
    elif own:
        assert 3 <= lens.min() <= 5 < lens.max()                                     # short rollouts and long ones
        kw = dict(len_u=_len_u(K))
    else:
        # the draws came from the sampler's generator: K n tasks' noise, then one uniform number per row of every forward
        twin = torch.Generator(device=DEV)
        twin.manual_seed(SEED)
        for it in range(N_ITERS):
            assert same(torch.randn(K, N_CAND, hp.n_nodes, hp.nz_vae, device=DEV, generator=twin), rec.noise[it])
            torch.rand(K * N_CAND, device=DEV, generator=twin)
        kw = dict(len_u=torch.rand(K, device=DEV, generator=twin))
        assert len(set(lens.tolist())) > 1
    direct = planner._sim.rollout(states, goals, rec.best_samples, hp.max_seq_len, **kw)
    for k in range(K):
        assert np.array_equal(out[k].predictions, direct.predictions[k]) and np.array_equal(out[k].latents, direct.latents[k])
        assert np.array_equal(out[k].actions, direct.actions[k]) and np.array_equal(out[k].states, direct.states[k])
        assert out[k].predictions.shape[1] == 3 * hp.img_sz ** 2 + hp.nz_enc and np.isfinite(out[k].cost)
        assert out[k].cost == float(planner.logs[-1].elite_scores[k, 0])
    assert not np.array_equal(out[0].predictions[0], out[1].predictions[0])       # different tasks, different plans


@pytest.mark.parametrize("max_rows", [None, 6])
def test_plan_batch_with_a_goal_image_per_task(setup, max_rows):
    hp, model, states, goals = setup
    goals01 = goals.astype(np.float32) / 255.0                                   # L2ImageCost's goal: the env image in [0, 1]
    cost = P.L2ImageCost(True, 1.5)
    planner = _planner(hp, model, False, cost=cost)
    assert planner.decode_candidates
    out = planner.plan_batch(states, goals01, record=True, max_rows=max_rows)
    replay(planner, K, N_CAND, N_ELITE)
    # the scores: per-row goals against rollout_cost_device task by task on the same rows
    sim, rec = planner._sim, planner.batch_record
    z = rec.populations[0].reshape(K * N_CAND, hp.n_nodes, hp.nz_vae)
    r = sim.rollout_device(np.repeat(states, N_CAND, 0), np.repeat(goals01, N_CAND, 0), z, hp.max_seq_len)
    x = sim.predictions_device(r)
    rows = cost.rollout_cost_rows_device(x, r.lengths, [g[None] for g in goals01], repeat=N_CAND)
    for k in range(K):
        sl = slice(k * N_CAND, (k + 1) * N_CAND)
        assert same(rows[sl], cost.rollout_cost_device(x[sl], r.lengths[sl], goals01[k:k + 1])), k
    if max_rows is None:                                                            # the same forward as the planner's first: its scores
        assert same(rows.reshape(K, N_CAND), rec.scores[0])
    assert len({float(s) for s in rows[:2 * N_CAND:N_CAND]}) == 2 and all(np.isfinite(o.cost) for o in out)
    with pytest.raises(ValueError, match="goals"):
        cost.rollout_cost_rows_device(x, r.lengths, [g[None] for g in goals01], repeat=N_CAND - 1)


def test_plan_batch_action_conditioned():
    import video_gcp_amd as V
    from video_gcp_amd.sequential import GCPSequentialModel
    hp = V.config("c1", nz_mid_lstm=128, lstm_init="zero", action_conditioned_pred=True, non_goal_conditioned=True, nz_vae=0,
                  var_inf="deterministic")
    model = GCPSequentialModel(hp, params=V.init_params_sequential(hp, seed=2, randomize_affine=True), device="cuda")
    model.eval()
    rng = np.random.RandomState(4)
    states, goals = (rng.randint(0, 256, size=(2, hp.img_sz, hp.img_sz, 3)).astype(np.uint8) for _ in range(2))
    T = hp.max_seq_len
    sampler = P.FlatCEMSampler(clip_val=INF, n_steps=T - 1, action_dim=hp.n_actions, initial_std=1.0, device=DEV, seed=3)
    cost = P.LearnedCostEstimate(model)
    planner = P.CEMPlanner(P.ActCondGCPImageSimulator(model), cost, sampler, n_iters=2, batch_size=6, elite_frac=0.5, max_seq_len=T)
    out = planner.plan_batch(states, goals, record=True)
    assert tuple(planner.batch_record.best_samples.shape) == (2, T - 1, hp.n_actions)
    replay(planner, 2, 6, 3, score=cost.sequence_cost_device)
    direct = planner._sim.rollout(states, goals, planner.batch_record.best_samples, T)
    for k in range(2):
        assert out[k].predictions.shape == (T, 3 * hp.img_sz ** 2 + hp.nz_enc) and out[k].latents.shape == (T, hp.nz_enc)
        assert np.array_equal(out[k].predictions, direct.predictions[k]) and np.isfinite(out[k].cost)


def test_batched_rollouts_against_rollouts_per_task(setup, batches):
    """a report with a loose bound, not bit-equality: each population rolled out for its task alone against its rows in the batch
    (fixed lengths)"""
    from helpers import assert_close
    hp, model, states, goals = setup
    planner, out = batches[False, None, False]
    rec = planner.batch_record
    worst = 0.0
    for it, pop in enumerate(rec.populations):
        for k in range(K):
            alone = planner._sim.rollout_device(states[k:k + 1], goals[k:k + 1], pop[k], hp.max_seq_len, decode=False).latents
            together = rec.rollouts[it][0][k * N_CAND:(k + 1) * N_CAND]
            worst = max(worst, float((alone - together).abs().max()))
            assert_close(together, alone, 5e-5, 1e-4, f"latents, task {k} iteration {it}")
    print(f"rollout latents, K n rows per forward against n rows per forward: max |difference| = {worst!r}")


# ---- 6. the runner and the entry point ------------------------------------------------------------------------------------------------------
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
def test_runner_with_batched_flat_plans(small_model, closed_loop):
    from test_gpu_nav_env import CW, IMG, T as TE, Replay
    from video_gcp_amd import control as CT
    from video_gcp_amd import nav_env as NE
    model, E = small_model, 3
    sampler = P.SimpleTreeCEMSampler(INF, None, 32, 1.0, n_level_hierarchy=4, device=DEV, seed=1)
    flat = P.CEMPlanner(P.GCPImageSimulator(model), P.LearnedCostEstimate(model), sampler, n_iters=1, batch_size=5, elite_frac=1.0, max_seq_len=12)
    planner = ShortPlans(flat, 4)
    env = NE.NavEnvBatch(9, CW, TE, IMG, DEV)
    runner = CT.ControlRunner(model, planner, env, replan_interval=TE + 2, num_max_replans=10, closed_loop_execution=closed_loop, batch_plans=True)
    tasks = NE.draw_tasks(9, 2, range(E))
    res = runner.run(tasks)
    assert res["full_traj"].shape == (E, TE + 1, 3) and res["actions"].shape == (E, TE, 2) and np.isfinite(res["actions"]).all()
    frames, goal_frames = env.frames.cpu().numpy(), env.goal_frames.cpu().numpy()
    steps = {}
    for e in range(E):
        replay_ = Replay(runner.plans[e], frames[e])
        policy = P.ImageCEMPolicy(model, replay_, replan_interval=TE + 2, num_max_replans=10, closed_loop_execution=closed_loop)
        planned_at = []
        for t in range(TE):
            before = replay_.calls
            a = np.asarray(policy.act(t=t, i_tr=0, images=frames[e, :t + 1], goal_image=goal_frames[e][None]).actions, dtype=np.float32)
            if replay_.calls != before:
                planned_at.append(t)
            assert np.array_equal(a.view(np.uint32), res["actions"][e, t].view(np.uint32)), (e, t, a, res["actions"][e, t])
        assert planned_at == [p["t"] for p in runner.plans[e]] and replay_.calls == len(runner.plans[e]) == res["n_replans"][e]
        assert planned_at[0] == 0 and len(planned_at) >= 2
        for t in planned_at:
            steps[t] = steps.get(t, 0) + 1
    # one plan_batch call per step at which anybody planned, carrying everybody who did; no per-episode call
    assert planner.single_calls == 0 and planner.batch_calls == [steps[t] for t in sorted(steps)] and max(planner.batch_calls) > 1


def test_control_main_with_a_flat_conf_and_batched_plans(tmp_path):
    from nav_env_cases import CONF
    from test_control_conf_cpu import FLAT
    from test_gpu_nav_env import T as TE
    from video_gcp_amd import control as CT
    text = CONF.format(env_params="n_rooms=9, crop_window=40, heading_smoothing=0.1, init_pos=None, goal_pos=None",
                       env_cls="TopdownMultiroom3dEnv", T=TE)
    for old, new in (("ImageHierarchicalTreeCEMSampler", FLAT["sampler"]), ("ImageLearnedCostEstimate", FLAT["cost"]),
                     ("n_iters=3, batch_size=3, sampling_rates_per_layer=[3, 3]", FLAT["cem_extra"])):
        assert old in text
        text = text.replace(old, new)
    conf = tmp_path / "mod_hyper.py"
    conf.write_text(text)
    out = str(tmp_path / "out")
    argv = ["--experiment", str(conf), "--data_dir", str(tmp_path / "data"), "--exp_dir", str(tmp_path / "exp"), "--random_weights", "1",
            "--n_tasks", "2", "--task_seed", "3", "--out", out, "--batch_plans", "1"]
    with pytest.raises(ValueError, match="reference_rng"):
        CT.main(argv + ["--reference_rng"])
    res = CT.main(argv)
    with np.load(os.path.join(out, "control_results.npz")) as z:
        assert set(CT.RESULT_KEYS) <= set(z.files)
        for k in CT.RESULT_KEYS:
            assert z[k].shape[0] == 2 and np.array_equal(z[k], res[k]), k
        assert z["actions"].shape == (2, TE, 2) and np.isfinite(z["actions"]).all()
