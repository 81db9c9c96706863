"""The flat CEM loop for K tasks per call (planning.CEMPlanner.plan_batch) without a GPU: the torch mirrors of the csrc/cem_batch.hip
kernels (cem_population_torch, cem_elites_torch, cem_refit_torch) against numpy, and plan_batch on CPU tensors -- where it runs through
those mirrors -- against K per-task replays.

1. cem_elites_torch is np.argsort(kind="stable")[:n_elite] per task, on rows with a tie, -0.0 beside +0.0, both infinities, a NaN that is
   not first, and an all-NaN row.
2. cem_refit_torch against numpy float64 within a bound derived from the data (test_refit_mirror_within_the_derived_bound), which
   torch's own float32 mean / std -- what the per-task FlatCEMSampler.fit computes -- meets as well.
3. plan_batch (K = 3, n = 6, elite_frac 0.5, 3 iterations, N = 7, dim = 4, T = 12, lengths from {1, 2, 3, 5, 12}) against per-task replays
   fed task k's noise block and length draws: each scores its own n rows alone, picks its elites with `select_elites` and refits with
   the mirror.  The stub simulator's latents are a function of the row's own sample and images made of float32 multiplies and adds
   only, and the stub cost (tests/test_tree_search_cpu.py) adds in a fixed order, so a row's score does not depend on its batch-mates:
   everything is equal bit for bit.  Task 2's candidates 1 and 4 of the first iteration are made identical.
4. the refusals, and that the sampler's own distribution is left alone."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_tree_search_cpu import StubCost, NZ, same  # noqa: E402
from video_gcp_amd import planning as P  # noqa: E402
from video_gcp_amd.model import Outputs  # noqa: E402

INF, NAN = float("inf"), float("nan")
U = 2.0 ** -24                                             # float32 unit roundoff


# ---- 1. elites ----------------------------------------------------------------------------------------------------------------------------
SPECIAL = [[3.0, 1.0, 2.0, 1.0, 0.5, 1.0, 7.0],                                 # a three-way tie
           [0.0, -0.0, 0.0, -1.0, -0.0, 1.0, 0.0],                              # -0.0 == +0.0: by index
           [INF, 2.0, -INF, INF, 1.0, -INF, 0.0],                               # both infinities, tied
           [1.0, NAN, 0.5, NAN, INF, -INF, 0.0],                                # NaNs that are not first: after inf, by index
           [NAN, NAN, NAN, NAN, NAN, NAN, NAN]]                                 # all NaN: the identity


@pytest.mark.parametrize("n_elite", [1, 3, 7])
def test_elites_mirror_is_the_stable_argsort(n_elite):
    scores = torch.tensor(SPECIAL)
    idx, best = P.cem_elites_torch(scores, n_elite)
    assert idx.dtype == torch.int32 and tuple(idx.shape) == tuple(best.shape) == (len(SPECIAL), n_elite)
    for k, row in enumerate(scores.numpy()):
        want = np.argsort(row, kind="stable")[:n_elite]
        assert idx[k].tolist() == want.tolist(), (k, idx[k], want)
        assert same(best[k].numpy(), row[want])
        assert idx[k].tolist() == P.select_elites(scores[k], n_elite).tolist()   # the per-task planner's pick
    if n_elite == 7:
        assert idx[1].tolist() == [3, 0, 1, 2, 4, 6, 5] and idx[3].tolist() == [5, 6, 2, 0, 4, 1, 3] and idx[4].tolist() == list(range(7))


# ---- 2. refit -----------------------------------------------------------------------------------------------------------------------------
def _gamma(k):
    return k * U / (1.0 - k * U)


def refit_bounds(x):
    """x float64 [m, ...] (the elites of one task, exact values of float32 data) -> (mean, std, E_mean, E_std), see the test below"""
    m = x.shape[0]
    mu, sigma = x.mean(0), x.std(0)
    A = np.abs(x).mean(0)
    e_mu = _gamma(m + 1) * A
    d = np.abs(x - mu)
    e = e_mu * (1 + U) + U * d
    e_v = (e * (2 * d + e)).mean(0) + _gamma(m + 2) * ((d + e) ** 2).mean(0)
    with np.errstate(divide="ignore", invalid="ignore"):
        root = np.where(sigma > 0, np.minimum(np.sqrt(e_v), e_v / sigma), np.sqrt(e_v))
    e_sigma = root + U * (sigma + root)
    return mu, sigma, e_mu, e_sigma


@pytest.mark.parametrize("n_elite", [1, 5, 51])
def test_refit_mirror_within_the_derived_bound(n_elite):
    """Float32 arithmetic with unit roundoff u = 2^-24, gamma_k = k u / (1 - k u) (Higham, Accuracy and Stability, ch. 3-4); m = n_elite
    elites x_1 .. x_m of one column, A = sum |x_j| / m, exact mean mu and population std sigma (numpy float64 of the float32 data, whose
    own error, ~m 2^-53, is 2^-29 of these bounds).

    mean  A sum of m terms in ANY order is within gamma_{m-1} sum |x_j| of the exact sum.  The division by m is one more rounding; a
          multiplication by a rounded 1 / m instead would be two.  So, for the mirror (sequential, one division) and for any other
          float32 mean alike:          |mean - mu| <= gamma_{m+1} A =: E_mu.
    std   second pass: d_j = fl(x_j - mean) differs from x_j - mu by at most e_j = E_mu (1 + u) + u |x_j - mu| (the inherited error of
          the mean, and one rounding).  Squaring, summing the m squares (any order) and dividing are at most m + 2 roundings on
          sum d_j^2 / m, and | d_j^2 - (x_j - mu)^2 | <= e_j (2 |x_j - mu| + e_j).  So the variance v is within
                 E_v = mean_j e_j (2 |x_j - mu| + e_j) + gamma_{m+2} mean_j (|x_j - mu| + e_j)^2,
          and, with | sqrt(a) - sqrt(b) | <= min( sqrt|a - b| , |a - b| / sqrt(b) ) and one rounding of the root,
                 |std - sigma| <= r + u (sigma + r) =: E_sigma,   r = min( sqrt(E_v), E_v / sigma ).
    For m = 1 nothing is rounded: mean = x_1 / 1 = x_1, d_1 = 0 and the std is exactly 0, which is asserted as such.

    torch's own mean(0) / std(0, unbiased=False) of the same elites -- FlatCEMSampler.fit -- is asserted to lie inside the same bounds (its
    std is no two-pass float32 sum, but is at least as accurate on these data): the per-task and the batched refit are within
    2 E_mu and 2 E_sigma of each other."""
    g = torch.Generator().manual_seed(40 + n_elite)
    K, n, shape = 3, 60, (7, 4)
    samples = torch.randn(K, n, *shape, generator=g)
    samples[1] = 3.0 + 0.1 * samples[1]                    # a mean far from 0 relative to the spread
    samples[2] = samples[2] * torch.logspace(-3, 3, 28).reshape(shape)      # columns of very different scale
    idx = torch.stack([torch.randperm(n, generator=g)[:n_elite] for _ in range(K)]).to(torch.int32)
    mean, std, best = P.cem_refit_torch(samples, idx)
    assert mean.dtype == std.dtype == torch.float32 and tuple(mean.shape) == tuple(std.shape) == tuple(best.shape) == (K,) + shape
    worst = [0.0, 0.0, 0.0, 0.0]
    for k in range(K):
        elites = samples[k][idx[k].long()]
        assert same(best[k].numpy(), elites[0].numpy())
        mu, sigma, e_mu, e_sigma = refit_bounds(elites.numpy().astype(np.float64))
        own_mean, own_std = elites.mean(0), elites.std(0, unbiased=False)
        for j, (got, want, bound) in enumerate(((mean[k], mu, e_mu), (std[k], sigma, e_sigma), (own_mean, mu, e_mu), (own_std, sigma, e_sigma))):
            err = np.abs(got.numpy().astype(np.float64) - want)
            if n_elite > 1:
                worst[j] = max(worst[j], float((err / bound).max()))
            assert (err <= bound).all(), (k, j, float(err.max()), float(bound.min()))
        if n_elite == 1:
            assert same(mean[k].numpy(), elites[0].numpy()) and bool((std[k] == 0).all()) and bool((own_std == 0).all())
    print(f"n_elite {n_elite}: largest error / bound: mirror mean {worst[0]:.3f} std {worst[1]:.3f}; torch mean {worst[2]:.3f} std {worst[3]:.3f}")


def test_refit_mirror_bad_index_and_population_mirror():
    g = torch.Generator().manual_seed(3)
    samples = torch.randn(3, 5, 2, 3, generator=g)
    idx = torch.tensor([[0, 4], [1, 5], [2, -1]], dtype=torch.int32)
    mean, std, best = P.cem_refit_torch(samples, idx)
    good = P.cem_refit_torch(samples[:1], idx[:1])
    assert all(same(a[0].numpy(), b[0].numpy()) for a, b in zip((mean, std, best), good))
    assert all(bool(torch.isnan(t[1:]).all()) and bool(torch.isfinite(t[0]).all()) for t in (mean, std, best))
    # block k of the population is the per-task sampler's from_unit_noise with task k's distribution
    mean, std = torch.randn(3, 2, 3, generator=g), torch.rand(3, 2, 3, generator=g)
    for clip in (0.5, INF):
        pop = P.cem_population_torch(mean, std, samples, clip)
        for k in range(3):
            s = P.FlatCEMSampler(clip, 2, 3, 1.0, device="cpu")
            s.mean, s.std = mean[k], std[k]
            assert same(pop[k].numpy(), s.from_unit_noise(samples[k]).numpy())
        assert float(pop.abs().max()) <= clip and (np.isfinite(clip)) == bool((pop.abs() == clip).any())


# ---- 3. plan_batch against per-task replays ----------------------------------------------------------------------------------------------
K, N_CAND, N_ITERS, N_NODES, DIM, T = 3, 6, 3, 7, 4, 12
LENGTHS = torch.tensor([1, 2, 3, 5, 12], dtype=torch.int32)
H = 4


class StubSim:
    """latents [rows, T, NZ]: lat[i, t, d] = sample[i].flatten()[(3 t + d) % (N dim)] * (0.5 + 0.125 t) + (s_i - g_i), s_i / g_i the mean byte of
    the row's start / goal image: float32 multiplies and adds of the row's own numbers"""
    supports_latent_only = True
    pred_length = True
    _append_latent = False

    def __init__(self):
        self.forwards = []

    def _latents(self, state, goal, samples, len_u):
        z = torch.as_tensor(samples, dtype=torch.float32)
        rows = z.shape[0]
        flat = z.reshape(rows, -1)
        t, d = torch.arange(T)[:, None], torch.arange(NZ)[None]
        off = torch.tensor([np.float32(int(s.astype(np.int64).sum()) - int(g.astype(np.int64).sum())) / np.float32(s.size * 255)
                            for s, g in zip(np.asarray(state), np.asarray(goal))], dtype=torch.float32)
        lat = flat[:, (3 * t + d) % flat.shape[1]] * (0.5 + 0.125 * t.to(torch.float32))[None] + off[:, None, None]
        lens = LENGTHS[(torch.as_tensor(len_u) * len(LENGTHS)).long().clamp(max=len(LENGTHS) - 1)]
        return lat, lens

    def rollout_device(self, state, goal, samples, rollout_len, decode=True, len_u=None):
        assert rollout_len == T and not decode and len(state) == len(goal) == len(samples)
        self.forwards.append(len(samples))
        lat, lens = self._latents(state, goal, samples, len_u)
        return Outputs(images=None, latents=lat, lengths=lens, actions=None, states=None, e_goal=lat[:, -1] * 0.5)

    def rollout(self, state, goal, samples, rollout_len, len_u=None):
        lat, lens = self._latents(state, goal, samples, len_u)
        cut = [lat[i, :l].numpy() for i, l in enumerate(lens.tolist())]
        return Outputs(predictions=cut, actions=[c[:-1, :2] for c in cut], latents=cut)


class LengthDraws:
    """f(rows) -> uniform numbers, kept; rows 1 and 4 of task 2 (rows 13 and 16 of an 18-row forward) get the same one"""

    def __init__(self):
        self.g, self.calls = torch.Generator().manual_seed(9), []

    def __call__(self, rows):
        u = torch.rand(rows, generator=self.g)
        if rows == K * N_CAND:
            u[2 * N_CAND + 4] = u[2 * N_CAND + 1]
        self.calls.append(u)
        return u


def _tasks():
    rng = np.random.RandomState(2)
    return tuple(rng.randint(0, 256, size=(K, H, H, 3)).astype(np.uint8) for _ in range(2))


@pytest.fixture(scope="module")
def batch():
    real = torch.randn

    def randn(*size, **kw):
        eps = real(*size, **kw)
        if tuple(size) == (K, N_CAND, N_NODES, DIM):
            eps[2, 4] = eps[2, 1]                          # two identical candidates of task 2, in every iteration
        return eps

    states, goals = _tasks()
    sampler = P.SimpleTreeCEMSampler(0.9, None, DIM, 0.75, n_level_hierarchy=3, device="cpu", seed=5)
    sim, draws = StubSim(), LengthDraws()
    planner = P.CEMPlanner(sim, StubCost(), sampler, n_iters=N_ITERS, batch_size=N_CAND, elite_frac=0.5, max_seq_len=T)
    before = (sampler.mean.clone(), sampler.std.clone())
    mp = pytest.MonkeyPatch()
    mp.setattr(torch, "randn", randn)
    try:
        out = planner.plan_batch(states, goals, record=True, len_u=draws)
    finally:
        mp.undo()
    return planner, sampler, sim, draws, out, before, states, goals


def test_plan_batch_equals_the_per_task_replays(batch):
    planner, sampler, sim, draws, out, before, states, goals = batch
    rec, cost, n_elite = planner.batch_record, StubCost(), 3
    assert len(out) == K and len(rec.noise) == N_ITERS and sim.forwards == [K * N_CAND] * N_ITERS and len(draws.calls) == N_ITERS + 1
    assert [tuple(l.elite_scores.shape) for l in planner.logs] == [(K, n_elite)] * N_ITERS
    assert [tuple(l.mean_score.shape) for l in planner.logs] == [(K,)] * N_ITERS
    tie = False
    for k in range(K):
        chk = P.FlatCEMSampler(0.9, N_NODES, DIM, 0.75, device="cpu")
        best = None
        for it in range(N_ITERS):
            pop = chk.from_unit_noise(rec.noise[it][k])
            assert same(pop.numpy(), rec.populations[it][k].numpy()), (k, it)
            alone = StubSim().rollout_device(np.repeat(states[k:k + 1], N_CAND, 0), np.repeat(goals[k:k + 1], N_CAND, 0), pop, T, decode=False,
                                             len_u=draws.calls[it][k * N_CAND:(k + 1) * N_CAND])
            rows = slice(k * N_CAND, (k + 1) * N_CAND)
            assert same(alone.latents.numpy(), rec.rollouts[it][0][rows].numpy()) and same(alone.lengths.numpy(), rec.rollouts[it][1][rows].numpy())
            scores = cost.sequence_cost_device(alone.latents, alone.lengths, alone.e_goal)
            assert same(scores.numpy(), rec.scores[it][k].numpy()), (k, it)
            idx = P.select_elites(scores, n_elite)
            assert idx.tolist() == rec.elite_idx[it][k].tolist() == np.argsort(scores.numpy(), kind="stable")[:n_elite].tolist(), (k, it)
            assert same(scores[idx].numpy(), planner.logs[it].elite_scores[k].numpy())
            assert float(planner.logs[it].mean_score[k]) == pytest.approx(float(scores.double().mean()), rel=1e-6)     # (a log entry)
            mean, std, best = P.cem_refit_torch(pop[None], idx[None].to(torch.int32))
            assert same(mean[0].numpy(), rec.means[it][k].numpy()) and same(std[0].numpy(), rec.stds[it][k].numpy()), (k, it)
            assert same(best[0].numpy(), pop[idx[0]].numpy())
            chk.mean, chk.std = mean[0], std[0]
            if k == 2:
                order = np.argsort(scores.numpy(), kind="stable").tolist()
                assert scores[1] == scores[4] and order.index(4) == order.index(1) + 1
                tie |= order.index(1) == n_elite - 1                # the pair straddles the cut: the tie alone decides that 1 is an elite
        assert same(best[0].numpy(), rec.best_samples[k].numpy())
        assert out[k].cost == float(planner.logs[-1].elite_scores[k, 0])
        final = StubSim().rollout(states[k:k + 1], goals[k:k + 1], rec.best_samples[k:k + 1], T, len_u=draws.calls[-1][k:k + 1])
        assert same(out[k].latents, final.latents[0]) and same(out[k].predictions, final.predictions[0]) and same(out[k].actions, final.actions[0])
        assert out[k].states is None
    lens = torch.cat([r[1] for r in rec.rollouts]).tolist()
    assert set(lens) == set(LENGTHS.tolist())                      # every length occurred, the one-frame rollout among them
    assert tie
    assert float(rec.populations[0].abs().max()) == pytest.approx(0.9)          # the clip was reached


def test_plan_batch_chunks_whole_tasks(batch):
    """max_rows = 6: one task per scoring forward, the same populations (the noise comes from the same seed), so the same search"""
    planner, _, _, _, _, _, states, goals = batch
    sampler = P.SimpleTreeCEMSampler(0.9, None, DIM, 0.75, n_level_hierarchy=3, device="cpu", seed=5)
    sim = StubSim()
    other = P.CEMPlanner(sim, StubCost(), sampler, n_iters=N_ITERS, batch_size=N_CAND, elite_frac=0.5, max_seq_len=T)
    other.plan_batch(states, goals, record=True, max_rows=N_CAND)
    assert sim.forwards == [N_CAND] * (K * N_ITERS)
    assert tuple(other.batch_record.rollouts[0][0].shape) == (K * N_CAND, T, NZ) and other.batch_record.scores[0].shape == (K, N_CAND)
    assert other.batch_record.best_samples.shape == (K, N_NODES, DIM)


# ---- 4. refusals and state ----------------------------------------------------------------------------------------------------------------
def test_plan_batch_leaves_the_sampler_alone(batch):
    planner, sampler, sim, draws, out, before, states, goals = batch
    assert torch.equal(sampler.mean, before[0]) and torch.equal(sampler.std, before[1])
    assert bool((sampler.mean == 0).all()) and bool((sampler.std == 0.75).all())
    assert not torch.equal(planner.batch_record.means[-1][0], sampler.mean)


def test_plan_batch_refusals():
    class Sim:
        def rollout_device(self, *a, **k):
            raise AssertionError("nothing may be rolled out")

    frames = np.zeros((2, H, H, 3), np.uint8)
    kw = dict(n_iters=1, batch_size=4, elite_frac=0.5, max_seq_len=T)
    flat = lambda **k: P.FlatCEMSampler(INF, N_NODES, DIM, 1.0, device="cpu", **k)
    with pytest.raises(ValueError, match="verbose"):
        P.CEMPlanner(Sim(), StubCost(), flat(), verbose=True, **kw).plan_batch(frames, frames)
    with pytest.raises(ValueError, match="PDDMSampler"):
        P.CEMPlanner(Sim(), StubCost(), P.PDDMSampler(INF, N_NODES, DIM, 1.0, device="cpu"), **kw).plan_batch(frames, frames)
    with pytest.raises(ValueError, match="shard"):
        P.CEMPlanner(Sim(), StubCost(), flat(n_shards=2), **kw).plan_batch(frames, frames)
    for bad in ((frames[0], frames[0]), (frames, frames[:1]), (frames[None], frames[None])):
        with pytest.raises(ValueError, match=r"\[K, H, W, 3\]"):
            P.CEMPlanner(Sim(), StubCost(), flat(), **kw).plan_batch(*bad)
