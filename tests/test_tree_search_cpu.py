"""The batched hierarchical search (tree_latent_search.BatchedDeviceTreeLatentOptimizer) on CPU tensors, through the torch mirrors of
the csrc/tree_search.hip kernels, against K runs of DeviceHierarchicalTreeLatentOptimizer: each is fed task k's slice of the rollouts and
replays task k's slice of every block the batched search drew.  Everything compared is a copy, an integer table or one float32 add of
the same two numbers: equal bit for bit (NaN costs: NaN on both sides).

The stub cost's rows are independent and it adds in a fixed order, so a cost does not depend on its batch-mates or on the padding of a
window: pair_cost(a, b) = sum_d (a_d - b_d)^2, the sequence cost its masked sum over the steps, both accumulated one term at a time.

Shapes: K = 3 tasks, rates [3, 2], 2 dense samples, depth 4, T = 12, nz = 8; latents and lengths (from {1, 2, 3, 4, 5, 7, 12}) are drawn
from fixed seeds, then a few rows are set so that every edge of the walk occurs, which the test asserts from the search's own tables:
a view with m = 0, a group with some short candidates, a group whose candidates are all short (the children's cost is NaN through the
stand-in row), a short alternative that wins, and an exact tie between identical rows, which the first wins."""
import numpy as np
import pytest
import torch

from video_gcp_amd import tree_latent_search as TS
from video_gcp_amd.model import Outputs

K, RATES, N_LL, DEPTH, T, NZ = 3, [3, 2], 2, 4, 12, 8
LENGTHS = (1, 2, 3, 4, 5, 7, 12)
POP = (3, 2, 2)                                           # candidates per task and iteration


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


class ReplayGenerator(np.random.Generator):
    """hands out recorded blocks instead of drawing"""

    def __init__(self, blocks):
        super().__init__(np.random.PCG64(0))
        self.blocks = list(blocks)

    def standard_normal(self, size=None, dtype=np.float64, out=None):
        b = self.blocks.pop(0)
        assert tuple(size) == b.shape and dtype == np.float32, (size, b.shape, dtype)
        return b.copy()


def rollouts():
    """per iteration: latents [K n, T, NZ], lengths [K n]"""
    g = torch.Generator().manual_seed(5)
    rng = np.random.RandomState(5)
    lat = [torch.randn(K * n, T, NZ, generator=g) for n in POP]
    lens = [rng.choice(LENGTHS, size=K * n).astype(np.int32) for n in POP]
    lens[0][0:3] = (1, 5, 12)                             # iteration 0, task 0: a one-frame rollout, m = 0
    lens[1][0:2] = (2, 12)                                # iteration 1, task 0: one short candidate of two
    lens[1][2:4] = (1, 2)                                 #              task 1: both short
    lens[1][4:6] = (3, 12)                                #              task 2: three frames split into 1 + 2, the left half has m = 0
    lens[2][0:2], lens[2][2:4], lens[2][4:6] = (5, 7), (12, 4), (12, 12)
    lat[2][5] = lat[2][4]                                 # iteration 2, task 2: two identical candidates, every decision a tie
    return lat, lens


def same(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


@pytest.fixture(scope="module")
def searches():
    lat, lens = rollouts()
    cost = StubCost()
    opt = TS.BatchedDeviceTreeLatentOptimizer(NZ, list(RATES), DEPTH, cost, cost, N_LL, K, torch.Generator().manual_seed(3), record=True)
    pops = []
    for it, n in enumerate(POP):
        pops.append(opt.sample())
        assert tuple(pops[-1].shape) == (K, n, 2 ** DEPTH - 1, NZ)
        opt.optimize(Outputs(latents=lat[it], lengths=torch.as_tensor(lens[it])))
    opt.record = False
    best = opt.sample()
    return opt, pops, best, lat, lens


def test_batched_walk_equals_the_per_task_search(searches):
    opt, pops, best, lat, lens = searches
    assert opt.fully_optimized and tuple(best.shape) == (K, 1, 2 ** DEPTH - 1, NZ) and len(opt.costs) == len(POP)
    cost = StubCost()
    for k in range(K):
        chk = TS.DeviceHierarchicalTreeLatentOptimizer(NZ, list(RATES), DEPTH, cost, cost, N_LL,
                                                       rng=ReplayGenerator([b[k].numpy() for b in opt.draws]))
        for it, n in enumerate(POP):
            assert same(chk.sample(), pops[it][k].numpy()), (k, it)
            plan, c = chk.optimize(Outputs(latents=lat[it][k * n:(k + 1) * n], lengths=lens[it][k * n:(k + 1) * n].tolist()))
            assert same(np.float32(c), opt.costs[it][k].numpy()), (k, it, c, opt.costs[it][k])
            assert [(int(i), int(t)) for i, t in plan] == opt.plans(it)[k], (k, it)
        assert not chk._rng.blocks                           # every block the batch drew was consumed, in order
        assert chk.fully_optimized and same(chk.sample(), best[k].numpy()), k


def test_every_edge_of_the_walk_occurred(searches):
    opt, pops, best, lat, lens = searches
    tables = opt.tables()
    m0 = short_some = short_all = short_won = False
    for it, decisions in enumerate(tables):
        dummy = K * POP[it]                                # the stand-in row of that iteration's rollout
        for kind, t in decisions:
            v = t["views"]
            if kind == "subgoal":
                m0 |= bool(((t["mids"] == 0) & (v[..., 2] - v[..., 1] == 1) & (v[..., 0] < dummy)).any())
            if kind == "children":
                short = (v[..., 2] - v[..., 1]) < 3
                short_some |= bool((short.any(1) & ~short.all(1)).any())
                short_all |= bool(short.all(1).any())
                short_won |= bool(t["use"].any())
                assert ((t["sidx"] >= 0) == short.any(1)).all()
                for k in np.nonzero(short.all(1))[0]:      # all short: both children are searched on the stand-in row: NaN, the segment wins
                    assert t["use"][k] and short[k, t["sidx"][k]]
    assert m0 and short_some and short_all and short_won
    # where every candidate was short the cost is the short segment's: finite, like all the others
    assert bool(torch.isfinite(torch.stack(opt.costs)).all())
    # the tie: task 2's two candidates of the last iteration are identical; the first wins every decision
    n = POP[2]
    assert torch.equal(lat[2][2 * n], lat[2][2 * n + 1]) and lens[2][2 * n] == lens[2][2 * n + 1]
    picks = [t["idx"][2] for kind, t in tables[2] if kind == "segment"]
    assert len(picks) == 4 and all(p == 0 for p in picks)


def test_select_mirror_has_numpy_argmin_semantics():
    inf, nan = float("inf"), float("nan")
    c = torch.tensor([[3.0, 1.0, 1.0], [inf, nan, 0.0], [2.0, nan, nan], [inf, inf, inf]])
    idx, cost, _ = TS.select_torch(c)
    assert idx.tolist() == [int(np.argmin(r)) for r in c.numpy()] == [1, 1, 1, 0]
    mask = torch.tensor([[1, 0, 1], [1, 0, 1], [0, 0, 0], [0, 1, 1]], dtype=torch.int32)
    idx, cost, _ = TS.select_torch(c, mask=mask)
    assert idx.tolist() == [2, 2, -1, 1] and cost.tolist() == [1.0, 0.0, inf, inf]


def test_plan_batch_needs_the_device_generator_and_no_verbose_logs():
    from video_gcp_amd import planning as P

    class Sim:
        def rollout_device(self, *a, **k):
            raise AssertionError("nothing may be rolled out")

    frames = np.zeros((2, 8, 8, 3), np.uint8)
    planner = P.HierarchicalCEMPlanner(Sim(), StubCost(), DEPTH, RATES, n_ll_samples=N_LL, action_dim=NZ, max_seq_len=T)      # np.random
    assert planner.device_resident and planner._sampler._rng is None
    with pytest.raises(ValueError, match="np.random"):
        planner.plan_batch(frames, frames)
    planner = P.HierarchicalCEMPlanner(Sim(), StubCost(), DEPTH, RATES, n_ll_samples=N_LL, action_dim=NZ, max_seq_len=T, fast_draws=True,
                                       verbose=True)
    with pytest.raises(ValueError, match="verbose"):
        planner.plan_batch(frames, frames)
