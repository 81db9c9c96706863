"""Stub simulator and cost of the receding-horizon CEM tests (tests/test_cem_warm_cpu.py, tests/test_gpu_cem_warm.py): a point that the
actions move, on CPU or device tensors alike.

An "image" is [1, 1, 3] float32 with the point's position in its first DIM channels.  A sample is an action sequence [S, DIM]; the state
after step t is the start plus the first t + 1 actions, added one at a time.  The cost is the squared distance of the last state to the
goal, the squares added in the order of the coordinates.  Every operation is a float32 multiply, add or subtract of a row's own numbers:
a row's score depends on nothing but the row, and a device computes the bits the CPU computes."""
import numpy as np
import torch

from video_gcp_amd import planning as P
from video_gcp_amd.model import Outputs

DIM = 2


def images(pos):
    """positions [K, DIM] -> 'images' [K, 1, 1, 3] of the same kind (numpy or tensor)"""
    if torch.is_tensor(pos):
        img = torch.zeros(pos.shape[0], 1, 1, 3, device=pos.device)
    else:
        img = np.zeros((pos.shape[0], 1, 1, 3), dtype=np.float32)
    img[:, 0, 0, :DIM] = pos
    return img


class PointSim:
    supports_latent_only = True
    pred_length = False
    _append_latent = False

    def __init__(self, device="cpu"):
        self.device, self.forwards = torch.device(device), []

    def task_frames(self, imgs, n):
        return torch.as_tensor(imgs, dtype=torch.float32).to(self.device).repeat_interleave(n, dim=0)

    def _states(self, state, goal, samples):
        a = torch.as_tensor(samples, dtype=torch.float32).to(self.device)
        pos = torch.as_tensor(state, dtype=torch.float32).to(self.device)[:, 0, 0, :DIM]
        out = []
        for t in range(a.shape[1]):
            pos = pos + a[:, t]
            out.append(pos)
        return torch.stack(out, dim=1), torch.as_tensor(goal, dtype=torch.float32).to(self.device)[:, 0, 0, :DIM]

    def rollout_device(self, state, goal, samples, rollout_len, decode=True, len_u=None):
        assert len(state) == len(goal) == len(samples)
        self.forwards.append(len(samples))
        lat, g = self._states(state, goal, samples)
        lens = torch.full((lat.shape[0],), lat.shape[1], dtype=torch.int32, device=self.device)
        return Outputs(images=None, latents=lat, lengths=lens, actions=None, states=None, e_goal=g)

    def rollout(self, state, goal, samples, rollout_len, len_u=None):
        lat = self._states(state, goal, samples)[0].cpu().numpy()
        rows = [lat[i] for i in range(lat.shape[0])]
        return Outputs(predictions=rows, actions=[np.asarray(torch.as_tensor(samples[i]).cpu()) for i in range(lat.shape[0])], latents=rows)


class EndDistance:
    """the learned-cost interface of CEMPlanner: squared distance of a rollout's last state to the goal"""
    input_dim = DIM

    def sequence_cost_device(self, lat, lens, goal):
        d = lat[:, -1] - goal
        d = d * d
        acc = d[:, 0]
        for j in range(1, d.shape[1]):
            acc = acc + d[:, j]
        return acc


def same(a, b):
    """equal bit for bit, NaNs of any payload alike"""
    a, b = (np.ascontiguousarray(x.detach().cpu().numpy() if torch.is_tensor(x) else x, dtype=np.float32) for x in (a, b))
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def point_planner(device="cpu", seed=3, S=6, n=8, n_iters=4, **kw):
    sampler = P.FlatCEMSampler(float("inf"), S, DIM, 1.0, device=device, seed=seed)
    return P.CEMPlanner(PointSim(device), EndDistance(), sampler, n_iters=n_iters, batch_size=n, elite_frac=0.5, max_seq_len=S,
                        use_inferred_actions=False, **kw)


def check_carried_elites(planner, K, m):
    """the recorded call: rows < m of every population after the first are the previous elites in rank order, and no task's best score
    ever gets worse"""
    rec = planner.batch_record
    assert rec.m == m and len(rec.populations) == planner.n_iters
    for it in range(1, planner.n_iters):
        for k in range(K):
            for j in range(m):
                assert same(rec.populations[it][k, j], rec.populations[it - 1][k, int(rec.elite_idx[it - 1][k, j])]), (it, k, j)
    best = torch.stack([l.elite_scores[:, 0] for l in planner.logs]).cpu().numpy()              # [n_iters, K]
    assert best.shape == (planner.n_iters, K) and (np.diff(best, axis=0) <= 0).all(), best
