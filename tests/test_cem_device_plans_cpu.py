"""CEMPlanner.plan_batch(device=True) and the horizon cap of plan_batch without a GPU, on the stub simulator and cost of
tests/test_cem_batch_cpu.py (CPU tensors go through the torch mirrors of the kernels).

The plans handed over as tensors are the plans of the host path on the same seed: the same best samples and costs, `lengths` the frames
of each returned plan, the first `lengths` latents and the first `n_actions` actions equal bit for bit -- with and without a horizon
(4, among rollout lengths 1, 2, 3, 5 and 12), with the inverse-model actions and with the best sample as the action plan."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_cem_batch_cpu import DIM, H, K, N_CAND, N_NODES, StubSim, T, _tasks  # noqa: E402
from test_tree_search_cpu import StubCost, same  # noqa: E402
from video_gcp_amd import planning as P  # noqa: E402
from video_gcp_amd.model import Outputs  # noqa: E402


class ActingStubSim(StubSim):
    """the stub with the actions of its host contract on the device rollout too: the first two latent columns of every frame but the last"""

    def rollout_device(self, state, goal, samples, rollout_len, decode=True, len_u=None):
        r = super().rollout_device(state, goal, samples, rollout_len, decode=decode, len_u=len_u)
        return Outputs(r, actions=r.latents[:, :-1, :2])


def len_u(rows):
    """length draws that make the first row of every forward a 12-frame rollout, the next a 2-frame one, then 5, 1, ..."""
    return (torch.arange(rows) * 0.37 + 0.95) % 1.0


def planner(horizon, inferred):
    sampler = P.FlatCEMSampler(0.9, N_NODES, DIM, 0.75, device="cpu", seed=5)
    return P.CEMPlanner(ActingStubSim(), StubCost(), sampler, n_iters=2, batch_size=N_CAND, elite_frac=0.5, max_seq_len=T, horizon=horizon,
                        use_inferred_actions=inferred)


@pytest.mark.parametrize("horizon", [None, 4])
@pytest.mark.parametrize("inferred", [True, False])
@pytest.mark.parametrize("max_rows", [None, N_CAND])
def test_device_plans_are_the_host_plans(horizon, inferred, max_rows):
    states, goals = _tasks()
    host_planner, dev_planner = planner(horizon, inferred), planner(horizon, inferred)
    host = host_planner.plan_batch(states, goals, record=True, max_rows=max_rows, len_u=len_u)
    dev = dev_planner.plan_batch(torch.as_tensor(states), torch.as_tensor(goals), record=True, max_rows=max_rows, device=True, len_u=len_u)
    assert same(dev.best, host_planner.batch_record.best_samples) and tuple(dev.best.shape) == (K, N_NODES, DIM)
    assert tuple(dev.costs.shape) == tuple(dev.lengths.shape) == tuple(dev.n_actions.shape) == (K,)
    lens = []
    for k in range(K):
        n = int(dev.lengths[k])
        lens.append(n)
        assert float(dev.costs[k]) == host[k].cost
        assert n == len(host[k].predictions) == len(host[k].latents) and same(dev.latents[k, :n], host[k].latents)
        assert int(dev.n_actions[k]) == len(host[k].actions) and same(dev.actions[k, :len(host[k].actions)], host[k].actions)
        if not inferred:
            assert same(host[k].actions, dev.best[k]) and len(host[k].actions) == N_NODES          # the sample itself, uncut
        elif horizon is None:
            assert len(host[k].actions) == max(n - 1, 0)
    if horizon is not None:
        assert lens == [4, 2, 4]                                      # rollouts of 12, 2 and 5 frames
        for _, rl in host_planner.batch_record.rollouts:
            assert int(rl.max()) == horizon and int(rl.min()) < horizon          # the cost read capped and uncapped rollouts
    # latents=False: nothing of the final rollout is handed over; this simulator draws its lengths, so the rollout still runs
    other = planner(horizon, inferred)
    light = other.plan_batch(torch.as_tensor(states), torch.as_tensor(goals), max_rows=max_rows, device=True, latents=False, len_u=len_u)
    assert light.latents is None and same(light.best, dev.best) and same(light.lengths, dev.lengths) and same(light.costs, dev.costs)


def test_horizon_changes_the_scores_only_where_it_cuts():
    """the capped cost is the cost of the rollout cut to the horizon: the uncapped planner's scores of the rows no longer than it"""
    states, goals = _tasks()
    a, b = planner(None, True), planner(4, True)
    a.plan_batch(states, goals, record=True, len_u=len_u)
    b.plan_batch(states, goals, record=True, len_u=len_u)
    ra, rb = a.batch_record, b.batch_record
    assert same(ra.populations[0], rb.populations[0])                 # the first population does not depend on the scores
    short = (ra.rollouts[0][1] <= 4).reshape(K, N_CAND)
    assert bool(short.any()) and not bool(short.all())
    assert same(ra.scores[0][short], rb.scores[0][short]) and not same(ra.scores[0][~short], rb.scores[0][~short])
    assert same(rb.rollouts[0][1], ra.rollouts[0][1].clamp(max=4))


def test_a_fixed_length_simulator_needs_no_final_rollout():
    """no drawn lengths, the best sample as the action plan, no latents wanted: plan_batch(device=True) rolls nothing out after the search"""

    class Fixed(ActingStubSim):
        pred_length = False

        def rollout_device(self, state, goal, samples, rollout_len, decode=True, len_u=None):
            return super().rollout_device(state, goal, samples, rollout_len, decode=decode, len_u=torch.full((len(samples),), 0.99))

    states, goals = _tasks()
    sampler = P.FlatCEMSampler(0.9, N_NODES, DIM, 0.75, device="cpu", seed=5)
    sim = Fixed()
    p = P.CEMPlanner(sim, StubCost(), sampler, n_iters=2, batch_size=N_CAND, elite_frac=0.5, max_seq_len=T, horizon=4, use_inferred_actions=False)
    r = p.plan_batch(torch.as_tensor(states), torch.as_tensor(goals), device=True, latents=False)
    assert sim.forwards == [K * N_CAND] * 2 and r.latents is None and r.lengths.tolist() == [4] * K and r.n_actions.tolist() == [N_NODES] * K
    assert r.actions is r.best
