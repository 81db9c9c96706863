"""Receding-horizon CEM in the flat batch planner, without a GPU: warm starts, carried elites, temporally correlated noise
(planning.cem_warm_start_torch, cem_population_ex_torch, CEMPlanner(noise_rho, keep_elites, warm_std).plan_batch(warm=),
control.ControlRunner(warm_start=True)).  On CPU tensors plan_batch runs through the mirrors, which are the kernels' checkers
(tests/test_gpu_cem_warm.py).

1. cem_warm_start_torch against a numpy loop: K = 4, S = 5, A = 3, the shifts -1, 0, 2, 4, 5, 9 in two calls, prev of a task without a
   plan filled with NaN, warm_std 1 and 0.5.
2. cem_population_ex_torch: rho = 0, m = 0 is cem_population_torch bit for bit with NaN and +-Inf in the noise; rho = 0.5 against a float32
   numpy loop that rounds every operation; the variance of the AR(1) noise stays 1 along the steps; carried rows are the words of
   prev_pop at prev_idx; an index out of range gives NaN rows.
3. plan_batch at default options: the populations, scores, means and stds of a planner built without the new arguments, the same
   generator state afterwards, the extended entry point never called.
4. carried elites: the best score of every task never gets worse over the iterations, rows < m are the previous elites.
5. ControlRunner(warm_start=True): the shifts and previous samples it hands to plan_batch, host and device hand-over; the refusals of the
   command line.
6. the point of it on a toy: receding-horizon control of a point, one CEM iteration per step."""
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cem_warm_stubs import DIM, EndDistance, PointSim, check_carried_elites, images, point_planner, same  # noqa: E402
from video_gcp_amd import control as CT  # noqa: E402
from video_gcp_amd import planning as P  # noqa: E402
from video_gcp_amd.model import Outputs  # noqa: E402

INF, NAN = float("inf"), float("nan")
SHIFTS = [-1, 0, 2, 4, 5, 9]
f32 = np.float32


# ---- 1. the warm start --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("warm_std", [1.0, 0.5])
@pytest.mark.parametrize("shifts", [SHIFTS[:4], SHIFTS[4:] + [-1, 2]])
def test_warm_start_mirror_is_the_shifted_plan(shifts, warm_std):
    K, S, A, init_std = 4, 5, 3, 0.3
    g = torch.Generator().manual_seed(11)
    prev = torch.randn(K, S, A, generator=g)
    for k, s in enumerate(shifts):
        if s < 0:
            prev[k] = NAN                                   # never read
    prev[shifts.index(2), 3, 1] = NAN                       # a NaN of the plan itself moves with it
    mean, std = P.cem_warm_start_torch(prev, torch.tensor(shifts, dtype=torch.int32), init_std, warm_std)
    assert mean.dtype == std.dtype == torch.float32 and tuple(mean.shape) == tuple(std.shape) == (K, S, A)
    wm, ws = np.zeros((K, S, A), f32), np.full((K, S, A), f32(init_std), f32)
    p = prev.numpy()
    for k, s in enumerate(shifts):
        for t in range(S):
            if s >= 0 and t + s < S:
                wm[k, t], ws[k, t] = p[k, t + s], f32(warm_std) * f32(init_std)
    assert same(mean, wm) and same(std, ws)
    k2 = shifts.index(2)
    assert bool(torch.isnan(mean[k2, 1, 1])) and int(torch.isnan(mean).sum()) == 1
    for k, s in enumerate(shifts):
        if s < 0 or s >= S:                                 # a cold start
            assert bool((mean[k] == 0).all()) and bool((std[k] == f32(init_std)).all())


# ---- 2. the population --------------------------------------------------------------------------------------------------------------------
def test_population_ex_at_rho_0_is_the_population_mirror():
    g = torch.Generator().manual_seed(5)
    K, n, S, A = 3, 6, 4, 3
    mean, std, eps = torch.randn(K, S, A, generator=g), torch.rand(K, S, A, generator=g) + 0.25, torch.randn(K, n, S, A, generator=g)
    eps[0, 1, 0, 2], eps[1, 2, 1, 0], eps[2, 0, 2, 1], eps[2, 5, 3, 2] = NAN, INF, -INF, NAN
    for clip in (0.5, INF):
        want = P.cem_population_torch(mean, std, eps, clip)
        got = P.cem_population_ex_torch(mean, std, eps, clip, rho=0.0, m=0)
        assert same(got, want)
        # the non-finite numbers stay in their own step: nothing of the next step is touched
        assert bool(torch.isnan(got[0, 1, 0, 2])) and bool(torch.isfinite(got[0, 1, 1:, 2]).all()) and bool(torch.isfinite(got[1, 2, 2:, 0]).all())


def test_population_ex_ar1_against_a_rounding_loop():
    g = torch.Generator().manual_seed(6)
    K, n, S, A, rho = 2, 5, 7, 3, 0.5
    mean, std, eps = torch.randn(K, S, A, generator=g), torch.rand(K, S, A, generator=g) + 0.25, torch.randn(K, n, S, A, generator=g)
    r, c = f32(rho), f32(np.sqrt(1.0 - float(f32(rho)) ** 2))
    assert P.cem_noise_c(rho) == float(c)
    mu, sd, e = mean.numpy(), std.numpy(), eps.numpy()
    for clip in (0.75, INF):
        want = np.zeros((K, n, S, A), f32)
        for k in range(K):
            for j in range(n):
                for a in range(A):
                    xi = e[k, j, 0, a]
                    for t in range(S):
                        if t > 0:
                            xi = f32(f32(r * xi) + f32(c * e[k, j, t, a]))
                        v = f32(mu[k, t, a] + f32(sd[k, t, a] * xi))
                        want[k, j, t, a] = v if not np.isfinite(clip) else min(max(v, f32(-clip)), f32(clip))
        assert same(P.cem_population_ex_torch(mean, std, eps, clip, rho=rho), want)
    for bad in (-0.1, 1.0, NAN):
        with pytest.raises(ValueError, match="rho"):
            P.cem_population_ex_torch(mean, std, eps, INF, rho=bad)


def test_ar1_noise_keeps_unit_variance():
    """xi_0 = eps_0 and xi_t = rho xi_{t-1} + sqrt(1 - rho^2) eps_t: by induction Var xi_t = rho^2 + (1 - rho^2) = 1, xi_t normal, and the
    N rows are independent.  The sample variance s^2 of N independent N(0, 1) numbers has Var s^2 = 2 / (N - 1) ((N - 1) s^2 is chi-squared
    with N - 1 degrees of freedom, variance 2 (N - 1)), so its standard error at N = 4096 is sqrt(2 / 4095) = 0.0221 and the bound 5 of
    them, 0.1105.  (White noise summed with weights rho, 1 instead, xi_t = rho xi_{t-1} + eps_t, would reach 1 / (1 - rho^2) = 5.3.)"""
    N, S, rho = 4096, 16, 0.9
    eps = torch.randn(1, N, S, 1, generator=torch.Generator().manual_seed(7))
    xi = P.cem_population_ex_torch(torch.zeros(1, S, 1), torch.ones(1, S, 1), eps, INF, rho=rho)[0, :, :, 0].double().numpy()
    var, se = xi.var(axis=0, ddof=1), np.sqrt(2.0 / (N - 1))
    print("sample variance of xi_t:", np.round(var, 4).tolist(), "standard error", round(float(se), 4))
    assert var.shape == (S,) and (np.abs(var - 1.0) <= 5 * se).all(), var
    lag1 = float(np.mean(xi[:, 1:] * xi[:, :-1]))          # and the noise is correlated as asked
    assert abs(lag1 - rho) < 0.05


def test_population_ex_carried_rows():
    g = torch.Generator().manual_seed(8)
    K, n, n_prev, S, A, m = 3, 5, 4, 3, 2, 2
    mean, std, eps = torch.randn(K, S, A, generator=g), torch.rand(K, S, A, generator=g) + 0.25, torch.randn(K, n, S, A, generator=g)
    prev_pop = 10.0 * torch.randn(K, n_prev, S, A, generator=g)                     # far outside the clip: not clamped again
    prev_pop[0, 3, 1, 1] = torch.tensor(np.array([0x7fc01234], np.uint32).view(f32))[0]     # a NaN with a payload: moved as a word
    idx = torch.tensor([[3, 0], [1, 1], [2, 3]], dtype=torch.int32)
    for rho in (0.0, 0.5):
        got = P.cem_population_ex_torch(mean, std, eps, 0.5, rho=rho, prev_pop=prev_pop, prev_idx=idx, m=m)
        free = P.cem_population_ex_torch(mean, std, eps, 0.5, rho=rho)
        assert same(got[:, m:], free[:, m:])                                        # the other rows: as without carried rows
        for k in range(K):
            for j in range(m):
                assert np.array_equal(got[k, j].numpy().view(np.uint32), prev_pop[k, int(idx[k, j])].numpy().view(np.uint32))
        # one index out of range: NaN in that task's carried rows, the rest as before
        for val in (n_prev, -1, 2 ** 31 - 1):
            bad = idx.clone()
            bad[1, 1] = val
            out = P.cem_population_ex_torch(mean, std, eps, 0.5, rho=rho, prev_pop=prev_pop, prev_idx=bad, m=m)
            assert bool(torch.isnan(out[1, :m]).all()) and same(out[1, m:], got[1, m:]) and same(out[0], got[0]) and same(out[2], got[2])
    for kw in (dict(m=n + 1), dict(m=n_prev + 1, prev_idx=torch.zeros(K, n_prev + 1, dtype=torch.int32)), dict(m=1, prev_pop=None), dict(m=-1)):
        with pytest.raises(ValueError, match="m ="):
            P.cem_population_ex_torch(mean, std, eps, 0.5, **dict(dict(prev_pop=prev_pop, prev_idx=idx, m=m), **kw))


# ---- 3. the defaults leave plan_batch alone ------------------------------------------------------------------------------------------------
# the stub simulator and cost of tests/test_cem_batch_cpu.py (a simulator that draws its lengths from the sampler's generator)
NZ, T, N_NODES, DIM_Z = 5, 12, 7, 4
LENGTHS = torch.tensor([1, 2, 3, 5, 12], dtype=torch.int32)


class StubCost:
    input_dim = NZ

    def pair_cost(self, a, b):
        d = (a - b) ** 2
        acc = d[:, 0]
        for j in range(1, d.shape[1]):
            acc = acc + d[:, j]
        return acc[:, None]

    def sequence_cost_device(self, lat, lens, goal):
        n, tmax, nz = lat.shape
        lens = torch.as_tensor(lens).long().clamp(max=tmax)
        acc = torch.zeros(n)
        for t in range(tmax):
            nxt = torch.where((t + 1 < lens)[:, None], lat[:, min(t + 1, tmax - 1)], goal)
            acc = acc + torch.where(t < lens, self.pair_cost(lat[:, t], nxt)[:, 0], torch.zeros(n))
        return acc


class StubSim:
    supports_latent_only = True
    pred_length = True
    _append_latent = False

    def _latents(self, state, goal, samples, len_u):
        z = torch.as_tensor(samples, dtype=torch.float32)
        flat = z.reshape(z.shape[0], -1)
        t, d = torch.arange(T)[:, None], torch.arange(NZ)[None]
        off = torch.tensor([f32(int(s.astype(np.int64).sum()) - int(g.astype(np.int64).sum())) / f32(s.size * 255)
                            for s, g in zip(np.asarray(state), np.asarray(goal))], dtype=torch.float32)
        lat = flat[:, (3 * t + d) % flat.shape[1]] * (0.5 + 0.125 * t.to(torch.float32))[None] + off[:, None, None]
        lens = LENGTHS[(torch.as_tensor(len_u) * len(LENGTHS)).long().clamp(max=len(LENGTHS) - 1)]
        return lat, lens

    def rollout_device(self, state, goal, samples, rollout_len, decode=True, len_u=None):
        lat, lens = self._latents(state, goal, samples, len_u)
        return Outputs(images=None, latents=lat, lengths=lens, actions=None, states=None, e_goal=lat[:, -1] * 0.5)

    def rollout(self, state, goal, samples, rollout_len, len_u=None):
        lat, lens = self._latents(state, goal, samples, len_u)
        cut = [lat[i, :l].numpy() for i, l in enumerate(lens.tolist())]
        return Outputs(predictions=cut, actions=[c[:-1, :2] for c in cut], latents=cut)


def test_default_options_leave_plan_batch_alone(monkeypatch):
    rng = np.random.RandomState(2)
    states, goals = (rng.randint(0, 256, size=(3, 4, 4, 3)).astype(np.uint8) for _ in range(2))
    kw = dict(n_iters=3, batch_size=6, elite_frac=0.5, max_seq_len=T)

    def build(**extra):
        sampler = P.SimpleTreeCEMSampler(0.9, None, DIM_Z, 0.75, n_level_hierarchy=3, device="cpu", seed=5)
        return P.CEMPlanner(StubSim(), StubCost(), sampler, **kw, **extra), sampler

    def refuse(*a, **k):
        raise AssertionError("the default does not go through the extended entry point")
    monkeypatch.setattr(P, "cem_population_ex", refuse)
    monkeypatch.setattr(P, "cem_warm_start", refuse)
    plain, s0 = build()
    explicit, s1 = build(noise_rho=0.0, keep_elites=0.0, warm_std=1.0)
    assert (plain.noise_rho, plain.keep_elites, plain.warm_std) == (0.0, 0.0, 1.0)
    out0, out1 = plain.plan_batch(states, goals, record=True), explicit.plan_batch(states, goals, record=True, warm=None)
    r0, r1 = plain.batch_record, explicit.batch_record
    assert r0.m == r1.m == 0 and bool((r0.start_mean == 0).all()) and bool((r0.start_std == 0.75).all())
    for key in ("noise", "populations", "scores", "means", "stds"):
        assert len(r0[key]) == len(r1[key]) == 3 and all(same(a, b) for a, b in zip(r0[key], r1[key])), key
    assert torch.equal(s0._gen.get_state(), s1._gen.get_state())
    # and they are what the planner computed before it had the options: the per-task sampler's population of each noise block, a
    # generator seeded alike asked for the same blocks in the same order
    twin = torch.Generator().manual_seed(5)
    chk = [P.FlatCEMSampler(0.9, N_NODES, DIM_Z, 0.75, device="cpu") for _ in range(3)]
    for it in range(3):
        assert same(torch.randn(3, 6, N_NODES, DIM_Z, generator=twin), r0.noise[it])
        torch.rand(18, generator=twin)
        for k in range(3):
            assert same(chk[k].from_unit_noise(r0.noise[it][k]), r0.populations[it][k])
            chk[k].mean, chk[k].std = r0.means[it][k], r0.stds[it][k]
    torch.rand(3, generator=twin)
    assert torch.equal(twin.get_state(), s0._gen.get_state())
    assert same(plain.batch_best, r0.best_samples) and all(a.cost == b.cost for a, b in zip(out0, out1))


def test_planner_validates_its_options():
    mk = lambda **k: P.CEMPlanner(PointSim(), EndDistance(), P.FlatCEMSampler(INF, 4, DIM, 1.0, device="cpu"), **k)
    for bad in (dict(noise_rho=1.0), dict(noise_rho=-0.1), dict(noise_rho=NAN), dict(keep_elites=1.0), dict(keep_elites=-0.5), dict(warm_std=0.0),
                dict(warm_std=1.5), dict(warm_std=NAN)):
        with pytest.raises(ValueError, match=next(iter(bad))):
            mk(**bad)
    p = mk(noise_rho=0.25, keep_elites=0.5, warm_std=0.75, n_iters=1, batch_size=4, elite_frac=0.5)
    assert (p.noise_rho, p.keep_elites, p.warm_std) == (0.25, 0.5, 0.75)
    pos = np.zeros((2, DIM), f32)
    for warm in ((torch.zeros(2, 3, DIM), torch.zeros(2, dtype=torch.int32)), (torch.zeros(2, 4, DIM, dtype=torch.float64), torch.zeros(2, dtype=torch.int32)),
                 (torch.zeros(2, 4, DIM), torch.zeros(2, dtype=torch.int64)), (torch.zeros(2, 4, DIM), torch.zeros(3, dtype=torch.int32))):
        with pytest.raises(ValueError, match="warm"):
            p.plan_batch(images(pos), images(pos + 1), warm=warm)


# ---- 4. carried elites ---------------------------------------------------------------------------------------------------------------------
def test_carried_elites_never_lose_a_plan():
    K = 5
    g = torch.Generator().manual_seed(4)
    start, goal = images(torch.zeros(K, DIM).numpy()), images((3.0 * torch.randn(K, DIM, generator=g)).numpy())
    planner = point_planner(keep_elites=0.5)
    planner.plan_batch(start, goal, record=True)
    check_carried_elites(planner, K, 2)
    assert planner._sim.forwards == [K * 8] * 4                                              # carried rows are rolled out like the others
    # without them the same seed does lose its best plan at some iteration of some task: the property is the option's
    free = point_planner()
    free.plan_batch(start, goal, record=True)
    assert free.batch_record.m == 0
    assert (np.diff(torch.stack([l.elite_scores[:, 0] for l in free.logs]).numpy(), axis=0) > 0).any()
    # the noise blocks do not depend on the option: rows < m of the draw were ignored, not skipped
    assert all(same(a, b) for a, b in zip(planner.batch_record.noise, free.batch_record.noise))
    assert torch.equal(planner._sampler._gen.get_state(), free._sampler._gen.get_state())


def test_first_population_of_a_warm_call_holds_the_starting_mean():
    K, S = 3, 6
    g = torch.Generator().manual_seed(9)
    prev, shift = torch.randn(K, S, DIM, generator=g), torch.tensor([1, -1, 2], dtype=torch.int32)
    prev[1] = NAN
    start, goal = images(np.zeros((K, DIM), f32)), images(np.ones((K, DIM), f32))
    planner = point_planner(keep_elites=0.5, noise_rho=0.5, warm_std=0.5, n_iters=2)
    planner.plan_batch(start, goal, record=True, warm=(prev, shift))
    rec = planner.batch_record
    wm, ws = P.cem_warm_start_torch(prev, shift, 1.0, 0.5)
    assert same(rec.start_mean, wm) and same(rec.start_std, ws) and bool((rec.start_mean[1] == 0).all())
    assert same(rec.populations[0][:, 0], rec.start_mean)                                   # row 0 alone, cold tasks included
    want = P.cem_population_ex_torch(wm, ws, rec.noise[0], INF, rho=0.5)
    assert same(rec.populations[0][:, 1:], want[:, 1:])
    check_carried_elites(planner, K, 2)
    assert same(planner.batch_best, rec.best_samples)
    # warm without carried rows: the first population is all noise around the warm start; prev None: a cold start
    other = point_planner(noise_rho=0.5, warm_std=0.5, n_iters=1)
    other.plan_batch(start, goal, record=True, warm=(prev, shift))
    assert same(other.batch_record.populations[0], P.cem_population_ex_torch(wm, ws, other.batch_record.noise[0], INF, rho=0.5))
    other.plan_batch(start, goal, record=True, warm=(None, shift))
    assert bool((other.batch_record.start_mean == 0).all()) and bool((other.batch_record.start_std == 1).all())


# ---- 5. the runner ---------------------------------------------------------------------------------------------------------------------------
E_R, T_R, S_R, L_R = 3, 5, 4, 6


class StubEnv:
    def __init__(self):
        self.E, self.T, self.device = E_R, T_R, torch.device("cpu")
        self.frames = torch.zeros(E_R, T_R + 1, 2, 2, 3, dtype=torch.uint8)
        self.goal_frames = torch.ones(E_R, 2, 2, 3, dtype=torch.uint8)
        self.actions = torch.zeros(E_R, T_R, 2)
        self.t = 0

    def reset(self, tasks):
        self.t = 0
        return self.frames[:, 0]

    def step(self, a):
        self.actions[:, self.t] = a
        self.t += 1

    def observe(self):
        return self.frames[:, self.t]

    def eval(self):
        return {}


class RecordingPlanner:
    """plan_batch keeps its `warm` argument and hands out a `batch_best` that names the call and the episode"""
    device_plans = True

    def __init__(self):
        self.warm, self.batch_best, self.due = [], None, []

    def plan_batch(self, states, goals, device=False, latents=True, warm=None):
        K, call = len(states), len(self.warm)
        self.warm.append(warm)
        self.batch_best = (100.0 * (call + 1) + torch.arange(K, dtype=torch.float32))[:, None, None].expand(K, S_R, 2).clone()
        if device:
            return Outputs(best=self.batch_best, costs=torch.zeros(K), lengths=torch.full((K,), L_R, dtype=torch.int32),
                           actions=torch.zeros(K, L_R - 1, 2), n_actions=torch.full((K,), L_R - 1, dtype=torch.int32), latents=None)
        return [Outputs(predictions=np.zeros((L_R, 3), f32), actions=np.zeros((L_R - 1, 2), f32), latents=np.zeros((L_R, 4), f32), cost=0.0)
                for _ in range(K)]


@pytest.mark.parametrize("keep_plans", [True, False])
def test_runner_hands_over_shifts_and_previous_samples(keep_plans):
    model = types.SimpleNamespace(_hp=types.SimpleNamespace(attach_inv_mdl=False, max_seq_len=L_R, n_actions=2, nz_enc=4))
    planner = RecordingPlanner()
    runner = CT.ControlRunner(model, planner, StubEnv(), replan_interval=2, num_max_replans=10, batch_plans=True, keep_plans=keep_plans,
                              warm_start=True)
    tasks = dict(start=np.zeros((E_R, 3), f32), goal=np.zeros((E_R, 2), f32))
    runner.run(tasks)
    assert len(planner.warm) == 3                                                   # t = 0, 2, 4
    prev, shift = planner.warm[0]
    assert prev is None and shift.dtype == torch.int32 and shift.tolist() == [-1] * E_R
    for call in (1, 2):
        prev, shift = planner.warm[call]
        assert shift.dtype == torch.int32 and shift.tolist() == [2] * E_R          # the steps executed on the plan that is replaced
        want = (100.0 * call + torch.arange(E_R, dtype=torch.float32))[:, None, None].expand(E_R, S_R, 2)
        assert prev.dtype == torch.float32 and torch.equal(prev, want)
    assert torch.equal(runner.best, planner.batch_best) and tuple(runner.best.shape) == (E_R, S_R, 2)
    runner.run(tasks)                                                               # a new run starts without previous plans
    assert planner.warm[3][0] is None and planner.warm[3][1].tolist() == [-1] * E_R
    # off: plan_batch is called as before
    planner = RecordingPlanner()
    CT.ControlRunner(model, planner, StubEnv(), replan_interval=2, batch_plans=True, keep_plans=keep_plans).run(tasks)
    assert planner.warm == [None] * 3
    with pytest.raises(ValueError, match="batch_plans"):
        CT.ControlRunner(model, planner, StubEnv(), warm_start=True)


@pytest.mark.parametrize("flag", [["--warm_start", "1"], ["--warm_std", "0.5"], ["--keep_elites", "0.5"], ["--noise_rho", "0.5"]])
def test_command_line_refusals(flag):
    base = ["--experiment", "none.py", "--out", "none"]
    with pytest.raises(ValueError, match="--batch_plans 1"):
        CT.main(base + flag)
    with pytest.raises(ValueError, match="reference_rng"):
        CT.main(base + flag + ["--batch_plans", "1", "--reference_rng"])
    given = CT.receding_options(CT.get_args(base + flag + ["--batch_plans", "1"]))
    assert list(given) == [flag[0][2:]]

    class Other:
        def plan_batch(self, states, goals):
            return []
    with pytest.raises(ValueError, match="Other"):
        CT.apply_receding_options(Other(), given)
    with pytest.raises(ValueError, match="HierarchicalCEMPlanner"):
        CT.apply_receding_options(object.__new__(P.HierarchicalCEMPlanner), given)
    planner = P.CEMPlanner(PointSim(), EndDistance(), P.FlatCEMSampler(INF, 4, DIM, 1.0, device="cpu"))
    CT.apply_receding_options(planner, given)
    assert (planner.noise_rho, planner.keep_elites, planner.warm_std) == (0.5 if "rho" in flag[0] else 0.0, 0.5 if "elites" in flag[0] else 0.0,
                                                                          0.5 if "warm_std" in flag[0] else 1.0)
    assert CT.receding_options(CT.get_args(base)) == {}
    CT.apply_receding_options(Other(), {})                                          # nothing given: nothing asked of the planner


# ---- 6. the point of it --------------------------------------------------------------------------------------------------------------------
def drive(options, K=16, steps=8, S=6, n=16):
    """receding-horizon control of K points: at every step one CEM iteration over S-step action sequences, the best sample's first action
    executed.  -> the final squared distances to the goals [K]"""
    g = torch.Generator().manual_seed(12)
    pos, goal = torch.zeros(K, DIM), 4.0 * torch.randn(K, DIM, generator=g)
    planner = point_planner(seed=1, S=S, n=n, n_iters=1, **options)
    prev = None
    for step in range(steps):
        kw = {}
        if options:
            kw = dict(warm=(prev, torch.full((K,), 1 if step else -1, dtype=torch.int32)))
        planner.plan_batch(images(pos.numpy()), images(goal.numpy()), **kw)
        prev = planner.batch_best
        pos = pos + prev[:, 0]
    return ((pos - goal) ** 2).sum(dim=1)


def test_receding_horizon_options_pay_on_a_toy():
    """K = 16 points with goals drawn from N(0, 16 I), 8 re-plans of one iteration each, 16 candidates of 6 steps, 8 elites, unit initial std,
    the generator seeded alike.  Measured mean final cost (squared distance to the goal): 16.7055 with the options off, 0.6746 with warm
    starts (warm_std 0.5), half of the elites carried (m = 4) and rho = 0.5: a factor of 25."""
    off = float(drive({}).mean())
    on = float(drive(dict(noise_rho=0.5, keep_elites=0.5, warm_std=0.5)).mean())
    print(f"mean final cost: options off {off:.4f}, on {on:.4f}")
    assert on < off
