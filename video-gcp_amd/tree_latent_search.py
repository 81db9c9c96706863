"""Hierarchical latent search for tree-structured predictors (host side, numpy).

Behavioural mirror of the reference's `ImageHierarchicalTreeLatentOptimizer` / `HierarchicalTreeLatentOptimizer`
(/root/reference/gcp/planning/tree_optimizer.py:7-260): the top `len(sampling_rates)` tree levels are optimised one
level per CEM iteration by scoring each sampled subgoal with a pairwise cost to both parents (:86-132); what remains
below is optimised jointly as dense "segments" (:79-84, 175-180).  Pinned bit-exactly — RNG draw order included — by
tests/golden/ref_tree_optimizer.npz, which was produced by executing the reference class
(tests/golden/make_ref_planner_goldens.py).

Layout contract (tree_optimizer.py:45-68): `sample()` returns [n, 2^depth - 1, latent_dim] with the
node axis in depth-first (in-order) order, i.e. [left subtree | this node | right subtree] — what
`GCPTreeModel.forward` expects for `inputs['z']`.

Written as an explicit search-state tree plus free functions instead of the reference's self-recursive class.
"""
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np


@dataclass
class _Level:
    """Search state of one position in the hierarchy."""
    depth: int
    n_samples: int
    n_latents: int
    left: Optional[List["_Level"]] = None      # one child search per sample (None at the dense bottom)
    right: Optional[List["_Level"]] = None
    done: bool = False
    best_z: Optional[np.ndarray] = None        # [n_latents, dim] once optimised
    last_draw: Optional[np.ndarray] = None     # [k, n_latents, dim] most recent draw


def _build(rates, depth, n_dense):
    if rates:
        k = rates[0]
        return _Level(depth, k, 1, [_build(rates[1:], depth - 1, n_dense) for _ in range(k)],
                      [_build(rates[1:], depth - 1, n_dense) for _ in range(k)])
    return _Level(depth, n_dense, 2 ** depth - 1)


class HierarchicalTreeLatentOptimizer:
    """Same constructor / methods as the reference class (image variant: states are flattened 3xRxR images)."""

    def __init__(self, latent_dim, sampling_rates, depth, subgoal_cost_fcn, ll_cost_fcn, final_layer_samples,
                 image_states=True, rng=None):
        """rng: None = the reference's draws (module-level np.random, the legacy Gaussian stream, every draw the reference makes —
        bit-exact with its class); a np.random.Generator = the same search on that generator with only the KEPT rows drawn, see
        _draw; a torch.Generator (of the device the rollouts run on) = the same, drawn on that device (_draw_device: `sample()` then
        returns a device tensor)"""
        self._rng = rng
        self._dim = latent_dim
        self._pair_cost = subgoal_cost_fcn
        self._seq_cost = ll_cost_fcn
        self._image_states = image_states
        self._root = _build(list(sampling_rates), depth, final_layer_samples)

    # ------------------------------------------------------------------ sampling
    def sample(self):
        return self._draw(self._root, False)

    def _draw_device(self, lv, below):
        """`_draw` in generator mode with a torch.Generator: the population is built where the model reads it (a dozen small launches
        per call instead of ~300 k host Gaussians and an upload); same tree walk, rows i.i.d. N(0, 1)"""
        import torch
        g = self._rng
        if below:
            assert not lv.done
            return torch.randn(1, 2 ** lv.depth - 1, self._dim, generator=g, device=g.device)
        if lv.done:
            z = lv.best_z[None]
        else:
            z = torch.randn(lv.n_samples, lv.n_latents, self._dim, generator=g, device=g.device)
            lv.last_draw = z
        if lv.left is None:
            return z
        rows = []
        for cl, cr, zi in zip(lv.left, lv.right, z):
            zl, zr = self._draw_device(cl, not lv.done), self._draw_device(cr, not lv.done)
            rows.append(torch.cat([zl, zi[:1].expand(zl.shape[0], 1, self._dim), zr], dim=1))      # depth-first: left | node | right
        return torch.cat(rows)

    def _draw(self, lv, below):
        if self._rng is not None and not isinstance(self._rng, np.random.Generator):
            return self._draw_device(lv, below)
        if below and self._rng is not None:
            # generator mode, below the level being optimised: nothing in this subtree is fixed yet (a level is optimised only after
            # its parent) and one row is kept of every draw — the whole subtree is one block of i.i.d. Gaussians, whatever its layout
            assert not lv.done
            return self._rng.standard_normal(size=(1, 2 ** lv.depth - 1, self._dim), dtype=np.float32)
        if lv.done:
            z = lv.best_z.copy()[None]
        else:
            # the reference draws np.random.normal(loc=zeros, scale=ones, size=...) (tree_optimizer.py:76-78): with array arguments
            # numpy walks the broadcast element by element, 0.0 + 1.0 * gauss — the same legacy Gaussian stream, in the same order, as
            # standard_normal fills in one call (bit-identical draws, pinned by tests/golden/ref_tree_optimizer.npz; 92 of the 97 ms
            # of a planner call were spent in the slow form)
            if self._rng is None:
                z = np.random.standard_normal(size=(lv.n_samples, lv.n_latents, self._dim))
                if below:                  # below the level being optimised only one latent is decoded
                    z = z[:1]
            else:
                # Below the level being optimised the reference draws n_samples rows and keeps the first (tree_optimizer.py:76-82):
                # 3.5 M Gaussians per planner call at rates [10, 10], 5 dense samples, 256-d latents, 26 ns each on the legacy
                # stream = 92 of the 98 ms of a call.  The rows are i.i.d., so drawing only the kept row gives the same
                # distribution of searches; float32 from the generator's ziggurat (what the model reads anyway).
                z = self._rng.standard_normal(size=(1 if below else lv.n_samples, lv.n_latents, self._dim), dtype=np.float32)
            lv.last_draw = z.copy()
        child_below = below or not lv.done
        if lv.left is None:
            return z
        rows = []
        for cl, cr, zi in zip(lv.left, lv.right, z):
            zl, zr = self._draw(cl, child_below), self._draw(cr, child_below)
            assert zl.shape == zr.shape
            mid = np.tile(zi[0], (zl.shape[0], 1, 1))
            rows.append(np.concatenate([zl, mid, zr], axis=1))      # depth-first: left | node | right
        return np.concatenate(rows)

    # ------------------------------------------------------------------ rollout helpers
    def _split(self, rollouts):
        d = self._pair_cost.input_dim
        states, latents = [], []
        for r in rollouts:
            s = r[..., :-d]
            if self._image_states:
                assert s.ndim == 2
                res = int(np.sqrt(s.shape[1] / 3))
                s = s.reshape(s.shape[0], 3, res, res)
            states.append(s)
            latents.append(r[..., -d:])
        return states, latents

    def _segment_inputs(self, rollouts, goal):
        states, latents = self._split(rollouts)
        if self._image_states:
            if goal.ndim > 2:              # raw goal image: score against each rollout's own last latent
                goals = [l[-1:] for l in latents]
            else:
                goals = [self._split([goal[None]])[1][0] for _ in latents]
            return latents, goals
        joined = goal.shape[-1] == rollouts[0].shape[-1]
        return states, (self._split([goal])[0][0] if joined else goal)

    def _best_segment(self, rollouts, goal):
        seqs, goals = self._segment_inputs(rollouts, goal)
        cost = self._seq_cost(seqs, goals)
        k = int(np.argmin(cost))
        return self._split(rollouts)[0][k], cost[k], k

    # ------------------------------------------------------------------ optimisation
    def optimize(self, all_rollouts, goal):
        return self._opt(self._root, all_rollouts, goal)

    def _opt(self, lv, rollouts, goal):
        if lv.left is None:
            best, cost, k = self._best_segment(rollouts, goal)
            lv.best_z, lv.done = lv.last_draw[k], True
            return best, cost
        if not lv.done:
            return self._opt_subgoal(lv, rollouts, goal)
        return self._opt_children(lv, rollouts, goal)

    def _opt_subgoal(self, lv, rollouts, goal):
        states, latents = self._split(rollouts)
        joined = goal.shape[-1] == rollouts[0].shape[-1]          # goal given as a (state ++ latent) vector
        mids = [int(np.floor(s.shape[0] / 2)) for s in states]
        start_s = np.stack([s[0] for s in states])
        start_l = np.stack([l[0] for l in latents])
        sub_s = np.stack([s[m] for s, m in zip(states, mids)])
        sub_l = np.stack([l[m] for l, m in zip(latents, mids)])
        if joined:
            gs, gl = self._split([goal[None]])
            goal_s = np.stack([gs[0][0] for _ in states])
            goal_l = np.stack([gl[0][0] for _ in latents])
        else:
            goal_s = np.stack([goal for _ in states])
            goal_l = np.stack([l[-1] for l in latents])
        total = self._pair_cost(start_l, sub_l) + self._pair_cost(sub_l, goal_l)
        k = int(np.argmin(total))
        lv.best_z = lv.last_draw[k]
        plan = [start_s[k]]
        if (sub_s[k] != plan[-1]).any():                          # identical when the sequence is too short
            plan.append(sub_s[k])
        if not joined:                                            # the final goal is appended exactly once
            g = goal_s[k]
            plan.append(g if g.shape == plan[-1].shape else g[0].transpose(2, 0, 1))
        lv.left, lv.right = lv.left[:1], lv.right[:1]             # keep only the winning branch
        lv.n_samples, lv.done = 1, True
        return np.stack(plan), total[k]

    def _opt_children(self, lv, rollouts, goal):
        results = []
        for cl, cr, group in zip(lv.left, lv.right, np.array_split(rollouts, lv.n_samples)):
            group = [r for r in group]
            short = []
            for i, r in enumerate(group):
                if r.shape[0] < 3:                                # nothing left to expand hierarchically
                    short.append(r)
                    group[i] = np.stack([np.full_like(r[0], np.inf), np.zeros_like(r[0]), np.full_like(r[0], np.inf)])
            cut = [int(np.floor(r.shape[0] / 2)) for r in group]
            subgoal = group[0][cut[0]]
            lr, lc = self._opt(cl, [r[:c] for r, c in zip(group, cut)], subgoal)
            rr, rc = self._opt(cr, [r[c:] for r, c in zip(group, cut)], goal)
            best, cost = np.concatenate([lr, rr]), lc + rc
            if short:
                sb, sc, _ = self._best_segment(short, goal)
                if sc < cost or np.isnan(cost):
                    best, cost = sb, sc
            results.append((best, cost))
        k = int(np.argmin(np.array([c for _, c in results])))
        return results[k]

    @property
    def fully_optimized(self):
        def full(lv):
            if lv.left is None:
                return lv.done
            return lv.done and all(full(c) for c in lv.left) and all(full(c) for c in lv.right)
        return full(self._root)


class ImageHierarchicalTreeLatentOptimizer(HierarchicalTreeLatentOptimizer):
    def __init__(self, *args, **kw):
        kw.setdefault("image_states", True)
        super().__init__(*args, **kw)


class DeviceHierarchicalTreeLatentOptimizer(ImageHierarchicalTreeLatentOptimizer):
    """The same search with the rollouts left on the device.

    The reference moves every rollout (image ++ latent, tens of MB per CEM iteration) to numpy and slices it on the host
    (tree_optimizer.py:86-180 via cem_simulator.py:68-70).  Only LATENTS enter the costs (subgoal pair cost :100-110, dense
    segment cost :70-84), so here a rollout is a (row, first frame, end frame) view into the simulator's device tensors:
    pair costs are one batched Predictor launch per branch (`cost.pair_cost`), segment costs one `cost.sequence_cost_device`
    call, and the host sees the sequence lengths and one argmin index per decision.  Plans are lists of (row, frame) references
    that are gathered into images only when somebody asks (`materialize`).  Draws, selections, costs and `best_z` are identical
    to the numpy class on identical np.random state: it stays in the tests as the checker."""

    RAW = ("raw",)                                   # goal given as the raw environment image: score against own last latent

    def sample(self):
        return super().sample()                      # np.random on the host: the search state is a few hundred KB

    def optimize(self, rollout, goal=None):
        """rollout: Outputs(latents [n, T, nz] device, lengths (device int32 or list), images [n, T, ...] or None)"""
        import torch
        lat = rollout.latents
        # one extra row holds the reference's stand-in for a rollout too short to split, [inf, 0, inf] (tree_optimizer.py:151-156)
        dummy = torch.zeros(1, lat.shape[1], lat.shape[2], device=lat.device)
        dummy[0, 0] = float("inf")
        if lat.shape[1] > 2:
            dummy[0, 2] = float("inf")
        self._lat = torch.cat([lat, dummy])
        self._dummy = lat.shape[0]
        lens = rollout.lengths.tolist() if torch.is_tensor(rollout.lengths) else list(rollout.lengths)
        self._rollout = rollout
        views = [(i, 0, l) for i, l in enumerate(lens)]
        plan, cost = self._dopt(self._root, views, self.RAW)
        return plan, cost

    def materialize(self, plan, goal_image=None):
        """plan references -> [len, 3, H, W] images on the device (the raw goal, when the plan ends in it, is `goal_image`)"""
        import torch
        img = self._rollout.images
        frames = [img[i, t] if i >= 0 else goal_image for i, t in plan]
        return torch.stack(frames)

    # ---- device mirrors of _opt / _opt_subgoal / _opt_children / _best_segment ----
    def _rows(self, refs):
        import torch
        idx = torch.tensor([[i, t] for i, t in refs], device=self._lat.device)
        return self._lat[idx[:, 0], idx[:, 1]]

    def _goal_rows(self, views, goal):
        if goal is self.RAW:
            return self._rows([(i, b - 1) for i, a, b in views])          # l[-1] of every rollout
        return self._rows([goal] * len(views))

    def _dbest_segment(self, views, goal):
        import torch
        n = len(views)
        tmax = max(b - a for _, a, b in views)
        lat = torch.zeros(n, tmax, self._lat.shape[-1], device=self._lat.device)
        for r, (i, a, b) in enumerate(views):
            lat[r, :b - a] = self._lat[i, a:b]
        lens = torch.tensor([b - a for _, a, b in views], dtype=torch.int32, device=self._lat.device)
        cost = self._seq_cost.sequence_cost_device(lat, lens, self._goal_rows(views, goal))
        k = int(torch.argmin(cost))
        i, a, b = views[k]
        return [(i, t) for t in range(a, b)], np.float32(cost[k].item()), k        # float32 like the numpy class: sums of costs stay bit-equal

    def _dopt(self, lv, views, goal):
        if lv.left is None:
            plan, cost, k = self._dbest_segment(views, goal)
            lv.best_z, lv.done = lv.last_draw[k], True
            return plan, cost
        if not lv.done:
            return self._dopt_subgoal(lv, views, goal)
        return self._dopt_children(lv, views, goal)

    def _dopt_subgoal(self, lv, views, goal):
        import torch
        mids = [(b - a) // 2 for _, a, b in views]
        start = self._rows([(i, a) for i, a, b in views])
        sub = self._rows([(i, a + m) for (i, a, b), m in zip(views, mids)])
        gl = self._goal_rows(views, goal)
        n = len(views)
        # both pair costs of all candidates in ONE Predictor launch
        c = self._pair_cost.pair_cost(torch.cat([start, sub]), torch.cat([sub, gl]))
        total = c[:n] + c[n:]
        k = int(torch.argmin(total.reshape(-1)))
        lv.best_z = lv.last_draw[k]
        i, a, b = views[k]
        plan = [(i, a)]
        if mids[k] != 0:
            plan.append((i, a + mids[k]))
        if goal is self.RAW:
            plan.append((-1, -1))                                 # the raw goal image closes the plan (tree_optimizer.py:127-129)
        lv.left, lv.right = lv.left[:1], lv.right[:1]
        lv.n_samples, lv.done = 1, True
        return plan, np.float32(total.reshape(-1)[k].item())

    def _dopt_children(self, lv, views, goal):
        results = []
        for cl, cr, group in zip(lv.left, lv.right, np.array_split(np.arange(len(views)), lv.n_samples)):
            group = [views[j] for j in group]
            short = [v for v in group if v[2] - v[1] < 3]                # nothing left to expand hierarchically
            group = [v if v[2] - v[1] >= 3 else (self._dummy, 0, 3) for v in group]
            cut = [(b - a) // 2 for _, a, b in group]
            i0, a0, _ = group[0]
            subgoal = (i0, a0 + cut[0])
            lr, lc = self._dopt(cl, [(i, a, a + c) for (i, a, b), c in zip(group, cut)], subgoal)
            rr, rc = self._dopt(cr, [(i, a + c, b) for (i, a, b), c in zip(group, cut)], goal)
            best, cost = lr + rr, lc + rc
            if short:
                sb, sc, _ = self._dbest_segment(short, goal)
                if sc < cost or np.isnan(cost):
                    best, cost = sb, sc
            results.append((best, cost))
        k = int(np.argmin(np.array([c for _, c in results])))
        return results[k]


# ---------------------------------------------------------------------------------------------------------------------------------------
# K tasks per walk
# ---------------------------------------------------------------------------------------------------------------------------------------
# The walk of _draw_device / _dopt* does not depend on the task: which level is drawn, which is optimised and how the population is laid
# out are the same for every task; only the views, the short-rollout cases and the chosen indices differ.  Each decision below is one
# library call over all K tasks (csrc/tree_search.hip) or, on CPU tensors, its torch mirror — the kernel's checker
# (tests/test_gpu_tree_search.py) and what lets the walk run without a device in the CPU tests (the convention of
# scalar_log.segment_norms_numpy); the mirrors are not a product path: tensors on a device always go through the library.

def _at(lat, row, frame):
    return lat[row.clamp(0, lat.shape[0] - 1), frame.clamp(0, lat.shape[1] - 1)]


def _goal_latents(lat, views, goal):
    v = views.long()
    row, b = v[..., 0], v[..., 2]
    gr, gf = goal[:, :1].long().expand_as(row), goal[:, 1:].long().expand_as(row)
    raw = gr < 0
    import torch
    return _at(lat, torch.where(raw, row, gr), torch.where(raw, b - 1, gf))


def subgoal_rows_torch(lat, views, goal):
    """gcpx_tree_subgoal_rows: lat [R, T, nz], views int32 [K, G, 3], goal int32 [K, 2] -> opa, opb [2 K G, nz], mids int32 [K, G]"""
    import torch
    v = views.long()
    row, a, b = v[..., 0], v[..., 1], v[..., 2]
    m = torch.where(b > a, (b - a) // 2, torch.zeros_like(a))
    start, sub, gl = _at(lat, row, a), _at(lat, row, a + m), _goal_latents(lat, views, goal)
    nz = lat.shape[-1]
    return torch.stack([start, sub]).reshape(-1, nz), torch.stack([sub, gl]).reshape(-1, nz), m.to(torch.int32)


def select_torch(c1, c2=None, mask=None, draw=None):
    """gcpx_tree_select: c1, c2 [K, G] float32, mask int32 [K, G], draw [K, G, zf] -> idx int32 [K], cost [K], best_z [K, zf] or None"""
    import torch
    total = c1 if c2 is None else c1 + c2
    K, G = total.shape
    ok = torch.ones_like(total, dtype=torch.bool) if mask is None else mask != 0
    ar = torch.arange(G, device=total.device).expand(K, G)
    none = torch.full_like(ar, G)
    nan = torch.isnan(total) & ok
    num = ok & ~nan
    low = torch.where(num, total, torch.full_like(total, float("inf"))).min(1, keepdim=True).values
    first_nan = torch.where(nan, ar, none).min(1).values
    first_min = torch.where(num & (total == low), ar, none).min(1).values
    idx = torch.where(first_nan < G, first_nan, first_min)                      # np.argmin: the first NaN, else the first minimum
    found = idx < G
    at = torch.where(found, idx, torch.zeros_like(idx))
    cost = torch.where(found, total.gather(1, at[:, None])[:, 0], torch.full_like(total[:, 0], float("inf")))
    best = None if draw is None else draw[torch.arange(K, device=total.device), at]
    return torch.where(found, idx, torch.full_like(idx, -1)).to(torch.int32), cost, best


def split_views_torch(views, dummy_row):
    """gcpx_tree_split_views: views int32 [K, G, 3] -> left, right int32 [K, G, 3], left_goal int32 [K, 2], short int32 [K, G]"""
    import torch
    row, a, b = views[..., 0], views[..., 1], views[..., 2]
    short = (b - a) < 3
    row = torch.where(short, torch.full_like(row, dummy_row), row)
    a = torch.where(short, torch.zeros_like(a), a)
    b = torch.where(short, torch.full_like(b, 3), b)
    c = (b - a) // 2
    left, right = torch.stack([row, a, a + c], -1), torch.stack([row, a + c, b], -1)
    return left, right, torch.stack([row[:, 0], (a + c)[:, 0]], -1), short.to(torch.int32)


def segment_windows_torch(lat, views, goal, tmax):
    """gcpx_tree_segment_windows: -> seg [K G, tmax, nz] (zero padded), lens int32 [K G], goal_rows [K G, nz]"""
    import torch
    v = views.long().reshape(-1, 3)
    row, a, b = v[:, 0], v[:, 1], v[:, 2]
    lens = (b - a).clamp(0, tmax)
    t = torch.arange(tmax, device=lat.device)
    seg = _at(lat, row[:, None].expand(-1, tmax), a[:, None] + t[None])
    seg = torch.where((t[None] < lens[:, None])[..., None], seg, torch.zeros_like(seg))
    return seg, lens.to(torch.int32), _goal_latents(lat, views, goal).reshape(-1, lat.shape[-1])


def short_alternative_torch(lc, rc, sc, sidx):
    """gcpx_tree_short_alternative: -> cost [K], use_short int32 [K]"""
    import torch
    c = lc + rc
    use = (sidx >= 0) & ((sc < c) | torch.isnan(c))
    return torch.where(use, sc, c), use.to(torch.int32)


class BatchedDeviceTreeLatentOptimizer:
    """DeviceHierarchicalTreeLatentOptimizer for K tasks at once: the same `_Level` tree and the same walk, a leading task axis on every
    tensor.  `best_z`, `last_draw`, the views, the selections and the costs are device tensors; a decision is one launch over all K
    tasks, a cost one Predictor call over the rows of all tasks, and nothing is read back until somebody asks for the plans.

    Draws come from one torch.Generator, in the order and block shapes of `_draw` in generator mode, each block with a leading K.
    Task k of the batch is the per-task search on the sample `[k]` of every block: tests/test_tree_search_cpu.py replays the blocks
    into K per-task searches and compares populations, costs, plans and optimised trees bit for bit."""

    def __init__(self, latent_dim, sampling_rates, depth, subgoal_cost_fcn, ll_cost_fcn, final_layer_samples, n_tasks, rng, record=False):
        import torch
        assert isinstance(rng, torch.Generator), "the batched search draws on the rollouts' device: rng is a torch.Generator"
        self._rng, self._dim, self.n_tasks = rng, latent_dim, int(n_tasks)
        self._pair_cost, self._seq_cost = subgoal_cost_fcn, ll_cost_fcn
        self._root = _build(list(sampling_rates), depth, final_layer_samples)
        self.record, self.draws = bool(record), []
        self.costs, self._records, self._tables = [], [], None

    # ------------------------------------------------------------------ sampling
    def sample(self):
        """[K, n, 2^depth - 1, latent_dim], node axis depth-first"""
        return self._bdraw(self._root, False)

    def _randn(self, s0, s1):
        import torch
        z = torch.randn(self.n_tasks, s0, s1, self._dim, generator=self._rng, device=self._rng.device)
        if self.record:
            self.draws.append(z)
        return z

    def _bdraw(self, lv, below):
        import torch
        if below:
            assert not lv.done
            return self._randn(1, 2 ** lv.depth - 1)
        if lv.done:
            z = lv.best_z[:, None]
        else:
            z = lv.last_draw = self._randn(lv.n_samples, lv.n_latents)
        if lv.left is None:
            return z
        rows = []
        for i, (cl, cr) in enumerate(zip(lv.left, lv.right)):
            zl, zr = self._bdraw(cl, not lv.done), self._bdraw(cr, not lv.done)
            rows.append(torch.cat([zl, z[:, i, None, :1].expand(-1, zl.shape[1], -1, -1), zr], dim=2))      # depth-first: left | node | right
        return torch.cat(rows, dim=1)

    # ------------------------------------------------------------------ the steps: library on a device, mirror on the host
    def _lib(self):
        from . import runtime as rt
        return rt, rt.load_library()

    @staticmethod
    def _stream(t):
        import torch
        return torch.cuda.current_stream(t.device).cuda_stream

    def _subgoal_rows(self, views, goal):
        import torch
        lat = self._lat
        if not lat.is_cuda:
            return subgoal_rows_torch(lat, views, goal)
        rt, lib = self._lib()
        K, G = views.shape[:2]
        opa, opb = torch.empty(2 * K * G, lat.shape[2], device=lat.device), torch.empty(2 * K * G, lat.shape[2], device=lat.device)
        mids = torch.empty(K, G, dtype=torch.int32, device=lat.device)
        rt.check(lib.gcpx_tree_subgoal_rows(lat.data_ptr(), views.data_ptr(), goal.data_ptr(), opa.data_ptr(), opb.data_ptr(), mids.data_ptr(),
                                            K, G, lat.shape[0], lat.shape[1], lat.shape[2], self._stream(lat)), "tree_subgoal_rows")
        return opa, opb, mids

    def _select(self, c1, c2=None, mask=None, draw=None):
        import torch
        if not c1.is_cuda:
            return select_torch(c1, c2, mask, draw)
        rt, lib = self._lib()
        K, G = c1.shape
        idx, cost = torch.empty(K, dtype=torch.int32, device=c1.device), torch.empty(K, device=c1.device)
        zf = 0 if draw is None else draw[0, 0].numel()
        best = None if draw is None else torch.empty((K,) + tuple(draw.shape[2:]), device=c1.device)
        rt.check(lib.gcpx_tree_select(c1.data_ptr(), rt.ptr(c2), rt.ptr(mask), rt.ptr(draw), rt.ptr(best), idx.data_ptr(), cost.data_ptr(),
                                      K, G, zf, self._stream(c1)), "tree_select")
        return idx, cost, best

    def _split_views(self, views):
        import torch
        if not views.is_cuda:
            return split_views_torch(views, self._dummy)
        rt, lib = self._lib()
        K, G = views.shape[:2]
        left, right = torch.empty_like(views), torch.empty_like(views)
        lgoal, short = torch.empty(K, 2, dtype=torch.int32, device=views.device), torch.empty(K, G, dtype=torch.int32, device=views.device)
        rt.check(lib.gcpx_tree_split_views(views.data_ptr(), self._dummy, left.data_ptr(), right.data_ptr(), lgoal.data_ptr(), short.data_ptr(),
                                           K, G, self._stream(views)), "tree_split_views")
        return left, right, lgoal, short

    def _segment_windows(self, views, goal, tmax):
        import torch
        lat = self._lat
        if not lat.is_cuda:
            return segment_windows_torch(lat, views, goal, tmax)
        rt, lib = self._lib()
        K, G = views.shape[:2]
        seg = torch.empty(K * G, tmax, lat.shape[2], device=lat.device)
        lens, rows = torch.empty(K * G, dtype=torch.int32, device=lat.device), torch.empty(K * G, lat.shape[2], device=lat.device)
        rt.check(lib.gcpx_tree_segment_windows(lat.data_ptr(), views.data_ptr(), goal.data_ptr(), seg.data_ptr(), lens.data_ptr(), rows.data_ptr(),
                                               K, G, lat.shape[0], lat.shape[1], tmax, lat.shape[2], self._stream(lat)), "tree_segment_windows")
        return seg, lens, rows

    def _short_alternative(self, lc, rc, sc, sidx):
        import torch
        if not lc.is_cuda:
            return short_alternative_torch(lc, rc, sc, sidx)
        rt, lib = self._lib()
        cost, use = torch.empty_like(lc), torch.empty_like(sidx)
        rt.check(lib.gcpx_tree_short_alternative(lc.data_ptr(), rc.data_ptr(), sc.data_ptr(), sidx.data_ptr(), cost.data_ptr(), use.data_ptr(),
                                                 lc.shape[0], self._stream(lc)), "tree_short_alternative")
        return cost, use

    # ------------------------------------------------------------------ optimisation
    def optimize(self, rollout):
        """rollout: Outputs(latents [K n, T, nz], lengths int32 [K n]) on the generator's device, the rows of task k at k n .. k n + n - 1.
        Optimises one level of every task; returns the K costs [K] float32 (a device tensor, also appended to `costs`)."""
        import torch
        lat = rollout.latents
        K = self.n_tasks
        assert lat.shape[0] % K == 0, "every task rolls out the same number of candidates"
        # the last row holds the reference's stand-in for a rollout too short to split, [inf, 0, inf] (tree_optimizer.py:142-147)
        dummy = torch.zeros(1, lat.shape[1], lat.shape[2], device=lat.device)
        dummy[0, 0] = float("inf")
        if lat.shape[1] > 2:
            dummy[0, 2] = float("inf")
        self._lat = torch.cat([lat, dummy]).contiguous()
        self._dummy = lat.shape[0]
        lens = torch.as_tensor(rollout.lengths, device=lat.device).to(torch.int32)
        rows = torch.arange(lat.shape[0], dtype=torch.int32, device=lat.device)
        views = torch.stack([rows, torch.zeros_like(rows), lens], -1).reshape(K, -1, 3).contiguous()
        raw = torch.full((K, 2), -1, dtype=torch.int32, device=lat.device)
        cost, rec = self._bopt(self._root, views, raw, True, lat.shape[1])
        self.costs.append(cost)
        self._records.append((rec, self._dummy))
        self._tables = None
        return cost

    def _segment_costs(self, views, goal, tmax):
        seg, lens, rows = self._segment_windows(views, goal, tmax)
        return self._seq_cost.sequence_cost_device(seg, lens, rows).reshape(views.shape[0], views.shape[1])

    def _bopt(self, lv, views, goal, raw, tmax):
        if lv.left is None:
            idx, cost, lv.best_z = self._select(self._segment_costs(views, goal, tmax), draw=lv.last_draw)
            lv.done = True
            return cost, dict(kind="segment", views=views, idx=idx)
        if not lv.done:
            return self._bopt_subgoal(lv, views, goal, raw)
        return self._bopt_children(lv, views, goal, raw, tmax)

    def _bopt_subgoal(self, lv, views, goal, raw):
        K, G = views.shape[:2]
        opa, opb, mids = self._subgoal_rows(views, goal)
        c = self._pair_cost.pair_cost(opa, opb).reshape(2, K, G)          # both pair costs of all candidates of all tasks: ONE Predictor launch
        idx, cost, lv.best_z = self._select(c[0], c[1], draw=lv.last_draw)
        lv.left, lv.right = lv.left[:1], lv.right[:1]                     # keep only the winning branch
        lv.n_samples, lv.done = 1, True
        return cost, dict(kind="subgoal", views=views, idx=idx, mids=mids, raw=raw)

    def _bopt_children(self, lv, views, goal, raw, tmax):
        assert lv.n_samples == 1                                          # an optimised level keeps one branch: the population is one group
        left, right, lgoal, short = self._split_views(views)
        half = max((tmax + 1) // 2, 2)                                    # a half is at most ceil(tmax / 2) frames; the stand-in's are 1 and 2
        lc, lrec = self._bopt(lv.left[0], left, lgoal, False, half)
        rc, rrec = self._bopt(lv.right[0], right, goal, raw, half)
        # the short candidates (fewer than 3 frames) scored as dense segments; the window is 2 frames, whatever the others hold is masked
        sidx, sc, _ = self._select(self._segment_costs(views, goal, 2), mask=short)
        cost, use = self._short_alternative(lc, rc, sc, sidx)
        return cost, dict(kind="children", views=views, sidx=sidx, use=use, left=lrec, right=rrec)

    # ------------------------------------------------------------------ results
    _TABLES = ("views", "idx", "mids", "sidx", "use")

    def _walk(self, rec):
        yield rec
        if rec["kind"] == "children":
            yield from self._walk(rec["left"])
            yield from self._walk(rec["right"])

    def _read_tables(self):
        """every selection and view table of every iteration so far in ONE copy to the host"""
        import torch
        if self._tables is None:
            ts = [(id(r), name, r[name]) for rec, _ in self._records for r in self._walk(rec) for name in self._TABLES if name in r]
            flat = torch.cat([t.reshape(-1).to(torch.int32) for _, _, t in ts]).cpu().numpy()
            self._tables, o = {}, 0
            for key, name, t in ts:
                self._tables[(key, name)] = flat[o:o + t.numel()].reshape(tuple(t.shape))
                o += t.numel()
        return self._tables

    def plans(self, iteration=-1):
        """the K plans of one iteration as lists of (row, frame) references, rows counted within the task (0 .. n - 1, n = the stand-in
        row; (-1, -1) = the raw goal image), rebuilt on the host from the selection tables"""
        tab = self._read_tables()
        rec, dummy = self._records[iteration]
        n = dummy // self.n_tasks

        def local(k, row):
            return n if row >= dummy else row - k * n

        def build(r, k):
            t = lambda name: tab[(id(r), name)]
            if r["kind"] == "children" and not t("use")[k]:
                return build(r["left"], k) + build(r["right"], k)
            if r["kind"] == "subgoal":
                j = t("idx")[k]
                i, a, b = (int(x) for x in t("views")[k, j])
                m = int(t("mids")[k, j])
                return [(local(k, i), a)] + ([(local(k, i), a + m)] if m != 0 else []) + ([(-1, -1)] if r["raw"] else [])
            j = t("sidx" if r["kind"] == "children" else "idx")[k]
            i, a, b = (int(x) for x in t("views")[k, j])
            return [(local(k, i), f) for f in range(a, b)]

        return [build(rec, k) for k in range(self.n_tasks)]

    def tables(self):
        """the selection tables (numpy) of every decision of every iteration, in walk order: [(kind, {name: array})]"""
        tab = self._read_tables()
        return [[(r["kind"], {name: tab[(id(r), name)] for name in self._TABLES if name in r}) for r in self._walk(rec)] for rec, _ in self._records]

    @property
    def fully_optimized(self):
        def full(lv):
            if lv.left is None:
                return lv.done
            return lv.done and all(full(c) for c in lv.left) and all(full(c) for c in lv.right)
        return full(self._root)
