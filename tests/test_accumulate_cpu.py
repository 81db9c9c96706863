"""CPU: the data side and the flags of gradient accumulation (train.py --accumulate_steps k).
  * the schedule a loader with accumulate = k walks is, in order (global batch g, j), the schedule of virtual rank rank·k + j of a
    virtual world world·k (dataset.epoch_schedule): with shuffling, two passes per epoch, and item counts that leave a remainder;
  * make_loader / SyntheticLoader / the argument parser / the start-up line;
  * two gloo ranks: the trainer's exchange hooks issue no collective during the micro-steps of a cycle and one per bucket at its end,
    over the cycle's sum."""
import os
import sys
import types

import pytest
import torch

from test_dist_cpu import _run_ranks, _wire

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import video_gcp_amd  # noqa: E402,F401
from video_gcp_amd import dataset as DS  # noqa: E402


class _Items:
    phase, T, img_sz = "train", 4, 8

    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


def _loader(n_items, B, n_repeat, seed, rank, world, accumulate):
    model = types.SimpleNamespace(_hp=types.SimpleNamespace(max_seq_len=_Items.T, img_sz=_Items.img_sz, batch_size=B), device="cpu")
    return DS.RingLoader(_Items(n_items), model, B, n_repeat, seed, rank, world, 2, True, 1, accumulate=accumulate)


def _virtual(n_items, B, n_repeat, seed, epoch, ranks, world):
    per = [DS.epoch_schedule(n_items, B, n_repeat, seed, epoch, True, rank=r, world=world) for r in ranks]
    assert len({len(p) for p in per}) == 1
    return [per[j][g] for g in range(len(per[0])) for j in range(len(ranks))]


def test_raw_schedule_identity():
    """what the feature rests on (holds without it): batch g·k + r of a single process is batch g of rank r of k"""
    for n_items, B, k, n_repeat in ((37, 2, 3, 2), (64, 4, 2, 1), (50, 3, 8, 1)):
        for cycle in range(2):
            one = DS.batch_schedule(n_items, B, 5, cycle, True, 0, 1)
            for r in range(k):
                rank = DS.batch_schedule(n_items, B, 5, cycle, True, r, k)
                assert rank == [one[g * k + r] for g in range(len(rank))]


@pytest.mark.parametrize("n_items,B,k,n_repeat", [(37, 2, 3, 2), (64, 4, 2, 1), (50, 3, 8, 1)])
def test_loader_walks_the_schedules_of_k_virtual_ranks(n_items, B, k, n_repeat):
    ld = _loader(n_items, B, n_repeat, 5, 0, 1, k)
    for epoch in (0, 3):
        ld.set_epoch(epoch)
        got = ld.schedule()
        assert got == _virtual(n_items, B, n_repeat, 5, epoch, range(k), k)
        assert len(got) == len(ld) == n_repeat * k * (n_items // (B * k)) and len(ld) % k == 0
        # a pass (not the epoch) drops its leftovers as the k-rank run does: every pass is whole cycles over its own shuffle
        per_pass = len(got) // n_repeat
        for r in range(n_repeat):
            cycles = {c for b in got[r * per_pass:(r + 1) * per_pass] for _, _, c in b}
            assert cycles == {epoch * n_repeat + r}
        # within a pass no item is read twice, and positions are the k-rank run's: contiguous from 0
        first = [p for b in got[:per_pass] for _, p, _ in b]
        assert sorted(first) == list(range(per_pass * B))


def test_two_ranks_accumulating_two_walk_a_world_of_four():
    n_items, B, n_repeat = 37, 2, 2
    seen = []
    for rank in range(2):
        ld = _loader(n_items, B, n_repeat, 9, rank, 2, 2)
        ld.set_epoch(1)
        got = ld.schedule()
        assert got == _virtual(n_items, B, n_repeat, 9, 1, (2 * rank, 2 * rank + 1), 4)
        assert len(ld) == len(got) == n_repeat * 2 * (n_items // 8) == 16
        seen += [i for b in got[:len(got) // n_repeat] for i, _, _ in b]
    assert len(set(seen)) == len(seen) == 32                               # the two ranks share a pass without overlap


def test_accumulate_one_is_the_plain_loader_and_bad_values_raise():
    ld = _loader(37, 2, 2, 5, 1, 2, 1)
    assert ld.schedule() == DS.epoch_schedule(37, 2, 2, 5, 0, True, 1, 2) and len(ld) == 2 * (37 // 4)
    with pytest.raises(ValueError):
        _loader(37, 2, 2, 5, 0, 1, 0)
    # 18 batches per pass are no multiple of 4: the plain loader keeps the two that no cycle can use
    four = _loader(37, 2, 2, 5, 0, 1, 4)
    assert len(four) == 2 * 16 and len(_loader(37, 2, 2, 5, 0, 1, 1)) == 2 * 18
    assert four.schedule() == _virtual(37, 2, 2, 5, 0, range(4), 4)


def test_make_loader_passes_accumulate_on(tmp_path):
    from dataset_fixture import write_random_dataset
    from video_gcp_amd.train import make_loader
    write_random_dataset(str(tmp_path), T=8, img=8, n_files=3, traj_per_file=3, seed=1, phases=("train",))
    hp = types.SimpleNamespace(max_seq_len=8, img_sz=8, batch_size=2)
    model = types.SimpleNamespace(_hp=hp, device="cpu")
    spec = DS.load_spec(str(tmp_path))
    ld = make_loader(str(tmp_path), spec, "train", hp, model, {}, n_repeat=2, seed=5, accumulate=2)
    assert ld.accumulate == 2 and len(ld) == 2 * 2 * (9 // 4) == 8
    assert ld.schedule() == _virtual(9, 2, 2, 5, 0, (0, 1), 2)
    assert len(make_loader(str(tmp_path), spec, "train", hp, model, {}, n_repeat=2, seed=5)) == 2 * (9 // 2)


def test_synthetic_loader_ends_on_a_cycle_boundary():
    import video_gcp_amd as V
    from video_gcp_amd.train import SyntheticLoader
    hp = V.config("tiny")
    assert len(SyntheticLoader(hp, 5, 0, "cpu", accumulate=2)) == 4
    assert len(SyntheticLoader(hp, 5, 0, "cpu", accumulate=8)) == 0
    assert len(SyntheticLoader(hp, 5, 0, "cpu")) == 5
    assert sum(1 for _ in SyntheticLoader(hp, 5, 0, "cpu", accumulate=2)) == 4


def test_flag_and_start_up_line(capsys):
    from video_gcp_amd.train import get_cmd_args, startup_line
    assert get_cmd_args([]).accumulate_steps == 1
    assert get_cmd_args(["--accumulate_steps", "8"]).accumulate_steps == 8
    with pytest.raises(SystemExit):
        get_cmd_args(["--accumulate_steps", "0"])
    capsys.readouterr()
    assert startup_line(16, 8, 1) == "[train] micro-batch 16 x accumulate_steps 8 x world 1 = effective batch 128"
    assert startup_line(16, 2, 4).endswith("= effective batch 128")


def test_trainer_rejects_a_bad_accumulate():
    from video_gcp_amd.training import GCPTrainStep
    model = types.SimpleNamespace(_hp=None)
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match="accumulate"):
            GCPTrainStep(model, accumulate=bad)


def _cycle_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    import torch.distributed as dist
    from video_gcp_amd import dist as D
    from video_gcp_amd.model import _Plan
    from video_gcp_amd.training import GCPTrainStep
    D.init_from_env("gloo")
    n, k = 1000, 2
    ranges = [("tree2", 700, 1000), ("tree1", 300, 700), ("rest", 0, 300)]
    # the trainer's exchange hooks around a stub backward plan (as test_dist_cpu._rebackward_worker), driven the way _micro_step drives
    # them: _accumulating during every backward of the cycle, then begin() + finish() over the sum
    tr = GCPTrainStep.__new__(GCPTrainStep)
    tr.grad = torch.zeros(n)
    tr.buckets = D.GradBuckets(tr.grad, ranges, None)
    tr._lane_streams = []
    state, calls = {}, []
    real = dist.all_reduce

    def counted(*a, **kw):
        calls.append(1)
        return real(*a, **kw)
    dist.all_reduce = counted

    def write(lo, hi, _stream):
        tr.grad[lo:hi] = state["g"][lo:hi]
        return 0
    plan = _Plan.__new__(_Plan)
    plan.lib, plan.ops, plan.keep, plan.lane = None, [], [], 0
    plan.add("bw.zero", lambda _s: (tr.grad.zero_(), 0)[1])
    for i, (_, lo, hi) in enumerate(ranges[:-1]):
        plan.add(f"bw.level{i}", write, lo, hi)
        plan.mark("bucket", i)
    plan.add("bw.rest", write, 0, 300)
    acc = torch.zeros(n)
    counts = []
    for j in range(k):
        state["g"] = torch.randn(n, generator=torch.Generator().manual_seed(10 * j + rank))
        tr._accumulating = True
        plan.run([None], on_mark=tr._on_mark)
        tr._accumulating = False
        counts.append(len(calls))
        if j < k - 1:
            acc = tr.grad.clone() if j == 0 else acc + tr.grad
    tr.grad += acc
    tr.buckets.begin()
    scale = tr.buckets.finish()
    counts.append(len(calls))
    q.put(_wire((rank, counts, scale, tr.grad.clone())))
    dist.destroy_process_group()


def test_two_ranks_exchange_once_per_cycle():
    res = {r[0]: r[1:] for r in _run_ranks(_cycle_worker)}
    want = sum(torch.randn(1000, generator=torch.Generator().manual_seed(10 * j + r)) for j in range(2) for r in range(2))
    for rank in range(2):
        counts, scale, grad = res[rank]
        assert list(counts) == [0, 0, 3], counts                         # nothing during the micro-steps, one collective per bucket
        assert scale == 0.5
        assert torch.allclose(grad, want, atol=1e-5)
    assert torch.equal(res[0][2], res[1][2])
