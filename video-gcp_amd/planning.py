"""CEM planning over the gcp_tree predictor: host-side mirror of the reference's planning stack with the rollout,
the learned cost and the elite selection kept on the device, and the candidate population sharded across ranks.

Reference (paths relative to /root/reference):
  GCPSimulator.rollout / GCPImageSimulator        gcp/planning/cem/cem_simulator.py:14-96
  CEMPlanner.__call__ / _rollout / _get_best_rollouts  gcp/planning/cem/cem_planner.py:55-135
  FlatCEMSampler / SimpleTreeCEMSampler           gcp/planning/cem/sampler.py:33-76
  LearnedCostEstimate                             gcp/planning/cem/cost_fcn.py:79-101
  TestTimeCostModel.forward                       gcp/prediction/models/auxilliary_models/cost_mdl.py:138-145

Deviations, on purpose:
  * D2 (cem_planner.py:115-122 drops the remainder of `batch_size // max_rollout_bs`): every candidate is evaluated.
  * D3: the reference's rollout runs under `val_mode()` = pred_length=True (cem_simulator.py:29), so the length of every candidate
    is a DRAW from the length predictor (base_gcp.py:219-226).  `GCPImageSimulator(pred_length=True)` (the default) does the same,
    with the categorical draw fed as one uniform number per candidate so that sharded ranks agree; `pred_length=False` pins every
    rollout to `rollout_len` (the fixed-work setting bench.py and the configs[3] tests use).
  * The reference moves every rollout to numpy (~2 GB per 512-candidate call, cem_simulator.py:68-70).  `rollout()` keeps
    that contract; the planner itself uses `rollout_device()` and only the final plan crosses to the host.
  * Multi-GPU: candidates are sharded over ranks; every rank draws the SAME population from a shared
    seed, rolls out its own slice, and one all-gather of the per-candidate costs lets all ranks pick identical elites.
"""
import numpy as np
import torch

from . import dist as D
from . import runtime as rt
from .model import Outputs


def env2planner(img):
    """GCPImageSimulator._env2planner (cem_simulator.py:87-96): env image(s) -> NCHW in [-1, 1].
    Bytes that are already on a device are converted there through the 256 values the host conversion gives (a device division by a
    scalar may multiply by its reciprocal): the same bits as converting on the host and uploading, without the round trip."""
    if torch.is_tensor(img) and img.dtype == torch.uint8 and img.device.type != "cpu":
        table = torch.arange(256, dtype=torch.float32)
        if int(img.max()) > 1:
            table = table / 255.0
        out = (table * 2 - 1.0).to(img.device)[img.long()]
        if out.dim() == 5:
            out = out[0]
        return out.permute(0, 3, 1, 2) if out.dim() == 4 else out
    img = torch.as_tensor(img, dtype=torch.float32)
    if img.max() > 1.0:
        img = img / 255.0
    if img.dim() == 5:
        img = img[0]
    if img.dim() == 4:
        img = img.permute(0, 3, 1, 2)
    return img * 2 - 1.0


class PlannerFrames:
    """start or goal frames that are already in the planner's format (`env2planner`: NCHW in [-1, 1]) on the model's device, one per row"""

    def __init__(self, frames):
        self.frames = frames


class GCPImageSimulator:
    """Simulator interface of the planner: candidate latents -> model rollouts."""

    supports_latent_only = True      # rollout_device(..., decode=False) skips the image decoder

    def __init__(self, model, append_latent=True, pred_length=True):
        self._model = model
        self._append_latent = append_latent
        self.pred_length = pred_length

    def _bcast(self, img, n):
        """the (single) start / goal image is converted once and broadcast on the device (cem_simulator.py:18 repeats it on the host:
        512 x 64 x 64 x 3 numpy copies + two 25 MB pageable uploads were 42 ms of a 60 ms scoring rollout)"""
        if isinstance(img, PlannerFrames):
            t = img.frames
        else:
            t = env2planner(np.asarray(img) if not torch.is_tensor(img) else img).to(self._model.device)
        assert t.shape[0] in (1, n), "one image for all candidates, or one per candidate"
        return t.expand(n, *t.shape[1:]) if t.shape[0] == 1 else t

    def task_frames(self, images, n):
        """env images [k, H, W, 3] of k planning tasks -> the frames of k * n candidate rows, task by task, as `rollout_device` takes them:
        every image is converted once, on the host as `_bcast` converts it, and repeated on the device (the same values as converting the
        repeated images, without k n host copies and their upload)"""
        t = env2planner(np.asarray(images) if not torch.is_tensor(images) else images).to(self._model.device)
        return PlannerFrames(t.repeat_interleave(n, dim=0) if n > 1 else t)

    def rollout_device(self, state, goal_state, samples, rollout_len, decode=True, len_u=None):
        """Device-resident rollout.  state/goal_state: env images [1,H,W,3]; samples [n, N, nz_vae] (depth-first node
        order, tree.py:38).  Returns padded device tensors + lengths.  decode=False: latents only (images = None) — what the
        CEM scoring loop needs; the decoder is 3/4 of the rollout's FLOPs."""
        m = self._model
        n = samples.shape[0]
        I0, Ig = self._bcast(state, n), self._bcast(goal_state, n)
        z = torch.as_tensor(samples, dtype=torch.float32, device=m.device)
        inp = dict(I_0=I0, I_g=Ig, z=z,
                   end_ind=torch.full((n,), rollout_len - 1, dtype=torch.long, device=m.device))
        if self.pred_length and len_u is not None:
            inp["len_u"] = torch.as_tensor(len_u, dtype=torch.float32, device=m.device)
        with m.val_mode(pred_length=self.pred_length, decode=decode):
            out = m(inp, "train")                    # cem_simulator.py:29-31 (phase defaults to 'train')
        raw = out.raw
        if "E" not in raw:
            # the flat predictor (GCPSequentialModel, samples [n, max_seq_len - 1, nz_vae]) has no tree: its frames are `images`, its
            # goal latent `e_g`, what ActCondGCPImageSimulator reads
            return Outputs(images=raw.get("images"), latents=raw["model_enc_seq_padded"], lengths=raw["seq_len"],
                           actions=raw.get("actions_padded"), states=raw.get("regressed_state_padded"), e_goal=raw["e_g"], out=out)
        return Outputs(images=raw.get("pruned_padded"), latents=raw["model_enc_seq_padded"], lengths=raw["seq_len"],
                       actions=raw.get("actions_padded"), states=raw.get("regressed_state_padded"),
                       e_goal=raw["E"][:, -1], out=out)

    def predictions_device(self, r):
        """GCPSimulator._get_state_rollouts (cem_simulator.py:48-61) on the padded device rollout: [n, T, 3 H W (+ nz_enc)] — the flat
        image of every step, with the latent appended when the simulator was built with append_latent"""
        assert r.images is not None, "hand-written costs read the decoded rollouts: the planner must decode its candidates"
        n, T = r.images.shape[:2]
        img = r.images.reshape(n, T, -1)
        return torch.cat((img, r.latents), dim=-1) if self._append_latent else img

    def rollout(self, state, goal_state, samples, rollout_len, prune=False, len_u=None):
        """Reference contract (cem_simulator.py:14-43): lists of numpy arrays, one per candidate."""
        r = self.rollout_device(state, goal_state, samples, rollout_len, len_u=len_u)
        lens = r.lengths.tolist()
        n = len(lens)
        img = r.images.reshape(n, r.images.shape[1], -1)
        preds = []
        for i, l in enumerate(lens):
            p = img[i, :l]
            if self._append_latent and not prune:
                p = torch.cat((p, r.latents[i, :l]), dim=-1)      # cem_simulator.py:54-59: image ++ latent
            elif prune:
                p = r.images[i, :l]
            preds.append(p.cpu().numpy())
        cap = lambda t, off=0: [t[i, :max(l - off, 0)].cpu().numpy() for i, l in enumerate(lens)]
        return Outputs(predictions=preds, actions=cap(r.actions, 1) if r.actions is not None else None,
                       states=cap(r.states) if r.states is not None else None, latents=cap(r.latents))


class ActCondGCPImageSimulator(GCPImageSimulator):
    """cem_simulator.py:99-104: the planner's samples are ACTION sequences (they arrive in the `z` slot), rolled out by an
    action-conditioned flat predictor (`action_conditioned_pred`, sequential.py:24-25,45-49; base_configs/vmpc.py) —
    `GCPSequentialModel`.  Selected by the policy's `act_cond` flag (planner_policy.py:197,231).  Such a model never draws its length
    (base_gcp.py:224-226): every rollout has `rollout_len` frames, frame 0 being the start image (sequential.py:57)."""

    supports_latent_only = True      # rollout_device(..., decode=False): the flat predictor's plan without decoder and head launches

    def __init__(self, model, append_latent=True, pred_length=False):
        assert model._hp.action_conditioned_pred, "the action-conditioned simulator needs an action-conditioned predictor"
        super().__init__(model, append_latent=append_latent, pred_length=False)

    def rollout_device(self, state, goal_state, samples, rollout_len, decode=True, len_u=None):
        """samples [n, max_seq_len - 1, n_actions]: action t leads from frame t to frame t + 1"""
        m = self._model
        hp = m._hp
        a = torch.as_tensor(samples, dtype=torch.float32, device=m.device)
        if a.dim() == 5:
            a = a[..., 0, 0]                                      # (cem_simulator.py:102: the image simulator appended two unit axes)
        n = a.shape[0]
        assert tuple(a.shape[1:]) == (hp.max_seq_len - 1, hp.n_actions), "one action per predicted frame"
        inp = dict(I_0=self._bcast(state, n), I_g=self._bcast(goal_state, n), actions=a,
                   end_ind=torch.full((n,), rollout_len - 1, dtype=torch.long, device=m.device))
        with m.val_mode(pred_length=False, decode=decode):
            out = m(inp, "train")
        raw = out.raw
        return Outputs(images=raw.get("images"), latents=raw["model_enc_seq_padded"], lengths=raw["seq_len"],
                       actions=raw.get("actions_padded"), states=raw.get("regressed_state_padded"), e_goal=raw["e_g"], out=out)


class LearnedCostEstimate:
    """Learned pairwise cost on latents (cost_fcn.py:79-101) backed by the model's `cost_mdl.cost_pred` Predictor."""

    def __init__(self, model):
        self._model = model
        self.lib = model.lib

    @property
    def input_dim(self):
        return self._model._hp.nz_enc

    def pair_cost(self, enc1, enc2):
        """cost of moving from enc1 to enc2, rows [R, nz] -> [R, 1]."""
        return self._model.predictor_rows("cost_mdl", torch.as_tensor(enc1), torch.as_tensor(enc2))

    def __call__(self, start_enc, goal_enc):
        if isinstance(start_enc, np.ndarray):                       # single start/goal pairs
            return self.pair_cost(start_enc, goal_enc).cpu().numpy()
        if isinstance(start_enc, list):                             # summed cost per sequence
            T = max(s.shape[0] for s in start_enc)
            n, nz = len(start_enc), start_enc[0].shape[-1]
            lat = torch.zeros(n, T, nz)
            for i, s in enumerate(start_enc):
                lat[i, :s.shape[0]] = torch.as_tensor(s)
            goal = torch.stack([torch.as_tensor(g).reshape(-1, nz)[0] for g in goal_enc])
            lens = torch.tensor([s.shape[0] for s in start_enc], dtype=torch.int32)
            dev = self._model.device
            return self.sequence_cost_device(lat.to(dev), lens.to(dev), goal.to(dev)).cpu().numpy()
        raise ValueError("Dimensionality of input to learned cost function not supported!")

    def sequence_cost_device(self, lat, lengths, goal=None):
        """sum_t cost(lat[i,t], next) over the first len_i steps, next = lat[i,t+1] or the goal latent after the last
        step (cost_fcn.py:91-94).  lat [n,T,nz], lengths int32 [n], goal [n,nz] -> [n]."""
        n, T, nz = lat.shape
        dev = lat.device
        lat = lat.contiguous()
        nxt = torch.empty_like(lat)
        stream = torch.cuda.current_stream(dev).cuda_stream
        g = goal.contiguous() if goal is not None else None
        rt.check(self.lib.gcpx_seq_pairs(lat.data_ptr(), lengths.data_ptr(), g.data_ptr() if g is not None else None,
                                         nxt.data_ptr(), n, T, nz, stream), "seq_pairs")
        per_step = self._model.predictor_rows("cost_mdl", lat.reshape(n * T, nz), nxt.reshape(n * T, nz))
        out = torch.empty(n, device=dev)
        rt.check(self.lib.gcpx_masked_row_sum(per_step.data_ptr(), lengths.data_ptr(), out.data_ptr(), n, T, stream),
                 "masked_row_sum")
        return out


class CostFcn:
    """Hand-written CEM costs (cost_fcn.py:10-77).  Host contract of the reference: `cost(cem_outputs, goal)` with `cem_outputs` a list of
    per-candidate arrays [len_i, D] -> one score per candidate; a subclass says what ONE rollout costs per step (`per_step`), this class
    turns the step costs into the score: the last step weighted by `final_step_weight`, then either everything summed (`dense_cost`) or
    the last step alone.  `rollout_cost_device` scores a padded device rollout ([n, T, D] + lengths) with one HIP launch
    (gcpx_rollout_cost, same four kinds) for the device-resident planner."""
    KIND = None

    def __init__(self, dense_cost, final_step_weight=1.0, *unused_args):
        self._dense_cost = dense_cost
        self._final_step_weight = final_step_weight

    def per_step(self, rollout, goal):
        """[len] step costs of one rollout [len, D]"""
        raise NotImplementedError

    def _prepare_goal(self, goal):
        return goal

    def __call__(self, cem_outputs, goal):
        # (cost_fcn.py:15-22: the step costs keep the rollout's dtype — float32 for model rollouts — through the final-step weight and
        # the sum, and so do the scores: near-tied candidates rank as in the reference)
        goal = self._prepare_goal(goal)
        scores = []
        for rollout in self._prepare_rollouts(cem_outputs):
            steps = np.array(self.per_step(rollout, goal))
            steps[-1] *= self._final_step_weight
            scores.append(np.sum(steps) if self._dense_cost else steps[-1])
        return np.array(scores)

    def _prepare_rollouts(self, cem_outputs):
        return cem_outputs

    def _device_goal(self, goal, D, device):
        return torch.as_tensor(np.asarray(goal, dtype=np.float32).reshape(-1)[:D].copy(), device=device)

    def rollout_cost_device(self, x, lengths, goal):
        """x [n, T, ld] device rollouts (predictions), lengths int32 [n], goal: what the host contract takes -> costs [n]"""
        from . import runtime as rt_
        n, T, ld = x.shape
        D = self._device_columns(ld)
        g = self._device_goal(goal, D, x.device)
        out = torch.empty(n, device=x.device)
        x = x.contiguous()
        rt_.check(rt_.load_library().gcpx_rollout_cost(x.data_ptr(), ld, lengths.data_ptr(), g.data_ptr(), 0, out.data_ptr(), n, T, D, self.KIND,
                                                       int(bool(self._dense_cost)), float(self._final_step_weight),
                                                       torch.cuda.current_stream(x.device).cuda_stream), "rollout_cost")
        return out

    def rollout_cost_rows_device(self, x, lengths, goals, repeat=1):
        """`rollout_cost_device` with a goal of its own per row (the rows of several planning tasks in one rollout): goals holds one goal,
        each what the host contract takes, per `repeat` consecutive rows of x [n, T, ld] -> costs [n].  One launch; a candidate's
        cost is computed by its own workgroup from its own rows and goal (csrc/misc.hip: rollout_cost_kernel), so it is the number
        `rollout_cost_device` gives that row among any other rows."""
        from . import runtime as rt_
        n, T, ld = x.shape
        D = self._device_columns(ld)
        if len(goals) * repeat != n:
            raise ValueError(f"{len(goals)} goals x {repeat} rows for {n} rollouts")
        g = torch.stack([self._device_goal(goal, D, x.device) for goal in goals])
        if repeat > 1:
            g = g.repeat_interleave(repeat, dim=0)
        g = g.contiguous()
        out = torch.empty(n, device=x.device)
        x = x.contiguous()
        rt_.check(rt_.load_library().gcpx_rollout_cost(x.data_ptr(), ld, lengths.data_ptr(), g.data_ptr(), g.shape[1], out.data_ptr(), n, T, D,
                                                       self.KIND, int(bool(self._dense_cost)), float(self._final_step_weight),
                                                       torch.cuda.current_stream(x.device).cuda_stream), "rollout_cost")
        return out

    def _device_columns(self, ld):
        return ld


class ImageCost:
    """cost_fcn.py:26-39: a rollout row is an image (3 x S x S, flattened) followed by `input_dim` latent columns"""

    def _split_state_rollout(self, rollouts):
        images, latents = [], []
        for r in rollouts:
            r = np.asarray(r)
            assert r.ndim == 2
            n_pix = r.shape[1] - self.input_dim
            side = int(np.sqrt(n_pix / 3))                        # three colour planes of side x side pixels
            images.append(r[:, :n_pix].reshape(r.shape[0], 3, side, side))
            latents.append(r[:, n_pix:])
        return Outputs(image_rollout=images, latent_rollout=latents)


def _row_norms(a):
    return np.sqrt(np.square(a).sum(axis=-1))


class EuclideanDistance(CostFcn):
    """distance of every step to the goal (cost_fcn.py:42-46)"""
    KIND = 0

    def per_step(self, rollout, goal):
        return _row_norms(rollout - np.asarray(goal).reshape(1, -1))


class EuclideanPathLength(CostFcn):
    """length of the path through the steps and on to the goal (cost_fcn.py:49-54); only meaningful summed over the steps"""
    KIND = 1

    def per_step(self, rollout, goal):
        assert self._dense_cost, "a path length is the sum over its steps: dense_cost must be set"
        successor = np.vstack([rollout[1:], np.asarray(goal).reshape(1, -1)])
        return _row_norms(successor - rollout)


class StepPathLength(CostFcn):
    """the number of steps, charged to the last one (cost_fcn.py:57-62)"""
    KIND = 2

    def per_step(self, rollout, goal):
        steps = np.zeros(len(rollout))
        steps[-1] = float(len(rollout))
        return steps

    def _device_goal(self, goal, D, device):
        return torch.zeros(1, device=device)


class L2ImageCost(CostFcn, ImageCost):
    """pixel-space distance of every predicted image to the goal image (cost_fcn.py:65-77); goal_raw: env image [1, H, W, 3] in [0, 1]"""
    KIND = 3
    LATENT_SIZE = 128

    @property
    def input_dim(self):
        return self.LATENT_SIZE

    @staticmethod
    def _goal_planes(goal_raw, dtype=None):
        g = np.asarray(goal_raw)
        if g.dtype == np.uint8:                                   # a recorded frame (control.ControlRunner's goals): bytes, as env2planner
            g = g.astype(np.float32) / np.float32(255.0)
        g = g.astype(dtype) if dtype is not None else g
        return np.moveaxis(g, 3, 1) * 2 - 1.0                     # HWC in [0, 1] -> CHW in [-1, 1]

    def _prepare_goal(self, goal_raw):
        return self._goal_planes(goal_raw)

    def _prepare_rollouts(self, cem_outputs):
        return self._split_state_rollout(cem_outputs).image_rollout

    def per_step(self, images, goal):
        return np.sqrt(np.square(images - goal).sum(axis=(1, 2, 3)))

    def _device_columns(self, ld):
        return ld - self.input_dim

    def _device_goal(self, goal_raw, D, device):
        return torch.as_tensor(self._goal_planes(goal_raw, np.float32).reshape(-1)[:D].copy(), device=device)


class FlatCEMSampler:
    """Gaussian sampler over [n_steps, dim] (sampler.py:33-48), on the device, seedable so that all ranks of a
    sharded planner draw the same population."""

    def __init__(self, clip_val, n_steps, action_dim, initial_std, device="cuda", seed=0, n_shards=None, dtype=torch.float32):
        """dtype: of the distribution and its draws (the reference's sampler is float64 numpy; float32 on the device by default).
        n_shards: the population is the concatenation of n_shards independently seeded sub-streams (seed, shard); default = the
        number of ranks, so that under a process group every rank draws ONLY its own 1/world of the candidates ("each GPU
        samples its slice (seed = base + rank)").  A single process asked for n_shards = k draws the same population a k-rank
        group does, which is how the sharded planner is checked against the unsharded one."""
        self._clip_val, self._n_steps, self._action_dim, self._initial_std = clip_val, n_steps, action_dim, initial_std
        self.device = torch.device(device)
        self._seed, self._n_shards, self._dtype = seed, n_shards, dtype
        self._gen = torch.Generator(device=self.device)             # rank-shared stream (length draws, one-shard populations)
        self._gen.manual_seed(seed)
        self._shard_gens = {}
        self.init()

    def init(self):
        self.mean = torch.zeros(self._n_steps, self._action_dim, device=self.device, dtype=self._dtype)
        self.std = self._initial_std * torch.ones(self._n_steps, self._action_dim, device=self.device, dtype=self._dtype)

    def n_shards(self):
        if self._n_shards is not None:
            return self._n_shards
        return D.dist.get_world_size() if D.dist.is_initialized() else 1

    def _draw(self, n, gen):
        return self.from_unit_noise(torch.randn(n, self._n_steps, self._action_dim, device=self.device, generator=gen, dtype=self._dtype))

    def from_unit_noise(self, eps):
        """the population that standard-normal numbers eps [n, n_steps, action_dim] stand for (sampler.py:40-42: np.random.normal(loc=mean,
        scale=std) = mean + std * eps, clipped) — the deterministic part of `sample`, pinned to the reference's on its own draws"""
        raw = self.mean[None] + self.std[None] * eps
        return raw.clamp(-self._clip_val, self._clip_val) if np.isfinite(self._clip_val) else raw

    def sample_shard(self, n_samples, shard):
        """rows [shard * n / n_shards, (shard + 1) * n / n_shards) of the population of n_samples candidates"""
        ns = self.n_shards()
        assert n_samples % ns == 0, "candidate population must divide evenly over the shards"
        if ns == 1:
            return self._draw(n_samples, self._gen)
        g = self._shard_gens.get(shard)
        if g is None:
            g = self._shard_gens[shard] = torch.Generator(device=self.device)
            g.manual_seed(self._seed * 1000003 + 7919 * (shard + 1))
        return self._draw(n_samples // ns, g)

    def sample(self, n_samples):
        """the whole population (every shard, in order)"""
        ns = self.n_shards()
        if ns == 1:
            return self._draw(n_samples, self._gen)
        return torch.cat([self.sample_shard(n_samples, s_) for s_ in range(ns)], 0)

    def sample_uniform(self, n_samples):
        """one uniform number per candidate from the sampler's own (rank-shared) stream: the length draw of a rollout"""
        return torch.rand(n_samples, device=self.device, generator=self._gen)

    def fit(self, data, scores=None):
        self.mean = data.mean(0)                                    # np.mean / np.std(axis=0), sampler.py:44-46
        self.std = data.std(0, unbiased=False)

    def get_dists(self):
        return Outputs(mean=self.mean, std=self.std)


class PDDMSampler(FlatCEMSampler):
    """Correlated noise + path-integral refit (sampler.py:52-71): n_i = BETA u_i + (1 - BETA) n_{i-1} along the steps, the mean refit
    as the exp(-GAMMA score)-weighted average of the candidates (scores: lower is better); the std is never refit."""
    BETA = 0.5      # noise correlation factor
    GAMMA = 1.0     # reward weighting factor

    def from_unit_noise(self, eps):
        noise = self.std[None] * eps
        # the recurrence unrolled: n_i = BETA sum_{k <= i} (1 - BETA)^(i - k) u_k — one lower-triangular mixing of the step axis
        i = torch.arange(self._n_steps, device=self.device)
        w = self.BETA * (1.0 - self.BETA) ** (i[:, None] - i[None]).clamp(min=0).to(torch.float32) * (i[:, None] >= i[None])
        raw = torch.einsum("ik,nkd->nid", w, noise) + self.mean[None]
        return raw.clamp(-self._clip_val, self._clip_val) if np.isfinite(self._clip_val) else raw

    def fit(self, actions, scores):
        wgt = torch.exp(-self.GAMMA * torch.as_tensor(scores, dtype=actions.dtype, device=actions.device))
        self.mean = (actions * wgt[:, None, None]).sum(0) / wgt.sum()


class SimpleTreeCEMSampler(FlatCEMSampler):
    """All 2^L - 1 tree latents optimised at once (sampler.py:68-76)."""

    def __init__(self, clip_val, n_steps, action_dim, initial_std, n_level_hierarchy, **kw):
        super().__init__(clip_val, 2 ** n_level_hierarchy - 1, action_dim, initial_std, **kw)


def select_elites(scores, n_elite):
    """cem_planner.py:129-130: indices of the n_elite lowest scores (stable, like numpy argsort on ties)."""
    return torch.argsort(scores, stable=True)[:n_elite]


# ---- the flat CEM loop for K tasks at once: csrc/cem_batch.hip and its torch mirrors -----------------------------------------------------
# Each mirror is the kernel's checker (tests/test_gpu_cem_batch.py: equal bit for bit) and what runs when the tensors are on the CPU
# (tests/test_cem_batch_cpu.py); tensors on a device always go through the library.  cem_warm_start and cem_population_ex are what
# receding-horizon planning adds (tests/test_cem_warm_cpu.py, tests/test_gpu_cem_warm.py); the default loop does not call them.
def cem_population_torch(mean, std, eps, clip):
    """gcpx_cem_population: mean, std [K, ...], eps [K, n, ...] -> clamp(mean + std * eps, -clip, clip) [K, n, ...]; block k is
    FlatCEMSampler.from_unit_noise(eps[k]) of a sampler holding task k's mean and std"""
    raw = mean[:, None] + std[:, None] * eps
    return raw.clamp(-clip, clip) if np.isfinite(clip) else raw


def cem_elites_torch(scores, n_elite):
    """gcpx_cem_elites: scores [K, n] -> idx int32 [K, n_elite], elite_scores [K, n_elite]: `select_elites` per task"""
    idx = torch.argsort(scores, dim=1, stable=True)[:, :n_elite]
    return idx.to(torch.int32), torch.gather(scores, 1, idx)


def cem_refit_torch(samples, idx):
    """gcpx_cem_refit: samples [K, n, ...], idx int32 [K, n_elite] -> mean, std, best [K, ...].  The elites are accumulated one at a
    time in their order, each operation a float32 tensor operation of its own: the kernel's sequence of IEEE operations.  A task with an
    index outside [0, n) gets NaN."""
    K, n = samples.shape[:2]
    n_elite = idx.shape[1]
    i = idx.long()
    bad = ((i < 0) | (i >= n)).any(dim=1)
    i = i.clamp(0, n - 1)
    ar = torch.arange(K, device=samples.device)
    x = [samples[ar, i[:, j]] for j in range(n_elite)]
    acc = x[0]
    for j in range(1, n_elite):
        acc = acc + x[j]
    mean = acc / n_elite
    d = x[0] - mean
    sq = d * d
    for j in range(1, n_elite):
        d = x[j] - mean
        sq = sq + d * d
    # the correctly rounded float32 root, as the kernel's sqrtf: through float64 (53 >= 2 * 24 + 2 bits: rounding twice is rounding
    # once), because torch's vectorised float32 sqrt on the CPU is not correctly rounded everywhere (0.7 % of its results are 1 ulp off)
    std = torch.sqrt((sq / n_elite).double()).float()
    best = x[0].clone()
    if bool(bad.any()):
        mean[bad] = std[bad] = best[bad] = float("nan")
    return mean, std, best


def cem_warm_start_torch(prev, shift, init_std, warm_std):
    """gcpx_cem_warm_start: prev [K, S, ...] the previous best samples, shift int [K] the steps executed since -> mean, std [K, S, ...].
    Task k with s = shift[k] >= 0: mean[k, t] = prev[k, t + s] and std = warm_std * init_std (one float32 product) where t + s < S; mean = 0
    and std = init_std behind that, and everywhere for s < 0, whose prev is not looked at (a NaN there does not spread)."""
    K, S = prev.shape[:2]
    s = torch.as_tensor(shift, device=prev.device).long()
    src = torch.arange(S, device=prev.device)[None] + s[:, None]
    take = ((s[:, None] >= 0) & (src < S)).reshape((K, S) + (1,) * (prev.ndim - 2)).expand(prev.shape)
    moved = prev[torch.arange(K, device=prev.device)[:, None], src.clamp(0, S - 1)]
    f32 = lambda v: torch.tensor(v, dtype=torch.float32, device=prev.device)
    mean = torch.where(take, moved, f32(0.0))
    std = torch.where(take, f32(warm_std) * f32(init_std), f32(init_std))
    return mean, std


def cem_noise_c(rho):
    """the weight of the fresh draw in the AR(1) noise: (float) sqrt(1 - (double) rho * rho) of the float32 rho, as the entry point forms it"""
    r = float(np.float32(rho))
    return float(np.float32(np.sqrt(1.0 - r * r)))


def cem_population_ex_torch(mean, std, eps, clip, rho=0.0, prev_pop=None, prev_idx=None, m=0):
    """gcpx_cem_population_ex: mean, std [K, S, ...], eps [K, n, S, ...] -> the K populations [K, n, S, ...].
    rows j >= m: clamp(mean + std * xi, -clip, clip) with xi_0 = eps_0, xi_t = (rho * xi_{t-1}) + (c * eps_t) along the steps, each a
    float32 operation of its own; rho = 0: xi = eps, cem_population_torch.
    rows j < m:  prev_pop[k, prev_idx[k, j]] (prev_pop [K, n_prev, S, ...], prev_idx int32 [K, m]) as they are; a task with an index outside
    [0, n_prev) gets NaN in these rows."""
    K, n, S = eps.shape[:3]
    if not 0.0 <= rho < 1.0:
        raise ValueError(f"rho = {rho} outside [0, 1)")
    if not 0 <= m <= n or (m > 0 and (prev_pop is None or prev_idx is None or m > prev_pop.shape[1] or prev_idx.shape[1] != m)):
        raise ValueError(f"m = {m} carried rows need 0 <= m <= n, m <= n_prev and prev_idx [K, m]")
    if float(np.float32(rho)) == 0.0:
        xi = eps
    else:
        r, c = (torch.tensor(v, dtype=torch.float32, device=eps.device) for v in (float(np.float32(rho)), cem_noise_c(rho)))
        steps = [eps[:, :, 0]]
        for t in range(1, S):
            steps.append((r * steps[-1]) + (c * eps[:, :, t]))
        xi = torch.stack(steps, dim=2)
    raw = mean[:, None] + std[:, None] * xi
    out = raw.clamp(-clip, clip) if np.isfinite(clip) else raw
    if m > 0:
        i, n_prev = prev_idx.long(), prev_pop.shape[1]
        bad = ((i < 0) | (i >= n_prev)).any(dim=1)
        out[:, :m] = prev_pop[torch.arange(K, device=eps.device)[:, None], i.clamp(0, n_prev - 1)]
        if bool(bad.any()):
            out[bad, :m] = float("nan")
    return out


def _stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream


def cem_warm_start(prev, shift, init_std, warm_std):
    """the K Gaussians mean, std [K, S, ...] a re-plan starts from: the previous best samples prev moved up by shift int32 [K] steps"""
    if not prev.is_cuda:
        return cem_warm_start_torch(prev, shift, init_std, warm_std)
    K, S = prev.shape[:2]
    prev, shift = prev.contiguous(), torch.as_tensor(shift).to(device=prev.device, dtype=torch.int32).contiguous()
    mean, std = torch.empty_like(prev), torch.empty_like(prev)
    rt.check(rt.load_library().gcpx_cem_warm_start(prev.data_ptr(), shift.data_ptr(), float(init_std), float(warm_std), mean.data_ptr(),
                                                   std.data_ptr(), K, S, prev[0, 0].numel(), _stream(prev)), "cem_warm_start")
    return mean, std


def cem_population_ex(mean, std, eps, clip, rho=0.0, prev_pop=None, prev_idx=None, m=0, inplace=False):
    """the K populations [K, n, S, ...] with m carried rows and AR(1) noise along the steps; inplace: written over eps"""
    if not eps.is_cuda:
        return cem_population_ex_torch(mean, std, eps, clip, rho, prev_pop, prev_idx, m)
    K, n, S = eps.shape[:3]
    mean, std, eps = mean.contiguous(), std.contiguous(), eps.contiguous()
    out = eps if inplace else torch.empty_like(eps)
    pp = pi = n_prev = 0
    if m > 0:
        prev_pop, prev_idx = prev_pop.contiguous(), prev_idx.contiguous()
        if prev_idx.shape[1] != m or prev_idx.dtype != torch.int32:
            raise ValueError("prev_idx is int32 [K, m]")
        pp, pi, n_prev = prev_pop.data_ptr(), prev_idx.data_ptr(), prev_pop.shape[1]
    rt.check(rt.load_library().gcpx_cem_population_ex(mean.data_ptr(), std.data_ptr(), eps.data_ptr(), float(clip), float(rho), pp, pi, int(m),
                                                      n_prev, out.data_ptr(), K, n, S, eps[0, 0, 0].numel(), _stream(eps)), "cem_population_ex")
    return out


def cem_population(mean, std, eps, clip, inplace=False):
    """the K populations [K, n, ...] that the noise blocks eps stand for; inplace: written over eps"""
    if not eps.is_cuda:
        return cem_population_torch(mean, std, eps, clip)
    K, n = eps.shape[:2]
    mean, std, eps = mean.contiguous(), std.contiguous(), eps.contiguous()
    out = eps if inplace else torch.empty_like(eps)
    rt.check(rt.load_library().gcpx_cem_population(mean.data_ptr(), std.data_ptr(), eps.data_ptr(), float(clip), out.data_ptr(), K, n,
                                                   mean[0].numel(), _stream(eps)), "cem_population")
    return out


def cem_elites(scores, n_elite):
    if not scores.is_cuda:
        return cem_elites_torch(scores, n_elite)
    K, n = scores.shape
    scores = scores.contiguous()
    idx, best = torch.empty(K, n_elite, dtype=torch.int32, device=scores.device), torch.empty(K, n_elite, device=scores.device)
    rt.check(rt.load_library().gcpx_cem_elites(scores.data_ptr(), idx.data_ptr(), best.data_ptr(), K, n, n_elite, _stream(scores)), "cem_elites")
    return idx, best


def cem_refit(samples, idx):
    if not samples.is_cuda:
        return cem_refit_torch(samples, idx)
    K, n = samples.shape[:2]
    samples, idx = samples.contiguous(), idx.contiguous()
    mean, std, best = (torch.empty((K,) + tuple(samples.shape[2:]), device=samples.device) for _ in range(3))
    rt.check(rt.load_library().gcpx_cem_refit(samples.data_ptr(), idx.data_ptr(), mean.data_ptr(), std.data_ptr(), best.data_ptr(), K, n,
                                              idx.shape[1], mean[0].numel(), _stream(samples)), "cem_refit")
    return mean, std, best


def rollout_chunks(sim, max_seq_len, states, goals, z, n, max_rows, decode, len_u, each=None, decode_device=False):
    """The rollout of K * n rows, task k's n rows with its own start and goal image, whole tasks per forward of at most `max_rows` rows.
    decode: sim.rollout (host lists), one Outputs per forward.  Otherwise sim.rollout_device: without `each` latents only, and the
    (latents, lengths) of all rows come back as one pair; with `each`, each(r, goals of the forward's tasks) is called on every
    forward's device rollout r before the next forward reuses its buffers (decode_device: with the images), and the list of what it
    returned comes back.  len_u: f(rows) -> the length draws of a forward of that many rows, or None."""
    K = states.shape[0]
    per = max(int(max_rows) // n, 1)
    parts = []
    for lo in range(0, K, per):
        hi = min(lo + per, K)
        rows = slice(lo * n, hi * n)
        kw = {} if len_u is None else dict(len_u=len_u((hi - lo) * n))
        if hasattr(sim, "task_frames"):                  # each task's images converted once, repeated on the device
            s, g = sim.task_frames(states[lo:hi], n), sim.task_frames(goals[lo:hi], n)
        else:
            s, g = np.repeat(states[lo:hi], n, axis=0), np.repeat(goals[lo:hi], n, axis=0)
        if decode:
            parts.append(sim.rollout(s, g, z[rows], max_seq_len, **kw))
            continue
        if each is not None:
            if getattr(sim, "supports_latent_only", False):
                kw["decode"] = decode_device
            parts.append(each(sim.rollout_device(s, g, z[rows], max_seq_len, **kw), goals[lo:hi]))
            continue
        r = sim.rollout_device(s, g, z[rows], max_seq_len, decode=False, **kw)
        # (the forward's buffers are reused by the next rollout of the same size)
        parts.append((r.latents.clone(), r.lengths.clone()) if K > per else (r.latents, r.lengths))
    if decode or each is not None or len(parts) == 1:
        return parts
    return [(torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts]))]


def elite_log_entry(goal_state, scores, images=None, latents=None, goal_rows=None, states=None):
    """One iteration of a verbose planner log (cem_planner.py:72-78: elite_rollouts, elite_scores, goal_state, elite_states).
    images: per elite [len, 3, H, W] in [-1, 1] (device tensors or numpy), or None when the elites were scored on latents only; then
    latents: per elite [len, nz_enc] on the device, what the decoder turns into those images, and goal_rows: per elite the rows that
    stand for the raw goal image (a hierarchical plan ends in it).  states: per trajectory [len, state_dim], or None."""
    return Outputs(elite_images=images, elite_latents=latents, goal_rows=goal_rows, elite_states=states, goal_state=np.asarray(goal_state),
                   elite_scores=scores)


def final_log_entry(final, goal_state, scores, n_latent):
    """the last entry of a call's log (cem_planner.py:81-88): the final rollout, its image part split off the appended latent"""
    imgs = []
    for p in final.predictions:
        p = np.asarray(p)
        if p.ndim == 2:                                             # flat image (++ latent) rows (cem_simulator.py:54-59)
            p = p[:, :p.shape[1] - n_latent]
            side = int(round(np.sqrt(p.shape[1] / 3)))
            p = p.reshape(p.shape[0], 3, side, side)
        imgs.append(p)
    st = final.get("states")
    return elite_log_entry(goal_state, scores, images=imgs, states=None if st is None else [np.asarray(x) for x in st])


class CEMPlanner:
    """Flat CEM over tree latents with device-resident rollouts and sharded candidates (cem_planner.py:55-135)."""

    def __init__(self, simulator, cost, sampler, n_iters=3, batch_size=512, elite_frac=0.1, max_seq_len=80,
                 goal_in_cost=True, decode_candidates=False, verbose=False, horizon=None, use_inferred_actions=True,
                 noise_rho=0.0, keep_elites=0.0, warm_std=1.0):
        # decode_candidates: also decode the images of every candidate while scoring (what the reference's simulator does,
        # cem_simulator.py:29-59).  The learned cost reads latents only, so by default the images are decoded once, for the
        # plan that is returned; scores, elites and the returned plan are the same either way.
        self.decode_candidates = decode_candidates or not hasattr(cost, "sequence_cost_device")     # hand-written costs read the images
        # horizon (cem_planner.py:115-122,151-155: _cap_to_horizon): every rollout's predictions, actions, states and latents are cut to
        # their first `horizon` entries before they are scored, and the returned plan likewise.  On the device: the rollout still runs
        # max_seq_len steps, its lengths are clamped in front of the cost (which reads the first `length` steps only), and the final
        # rollout is sliced.  None: nothing is cut.
        # use_inferred_actions (cem_planner.py:143-149): True, the plan's actions are the final rollout's (inverse-model) actions; False,
        # the action plan is the best sample itself, uncut -- meaningful when the samples are actions (ActCondGCPImageSimulator).
        assert horizon is None or horizon >= 1
        self.horizon, self.use_inferred_actions = horizon, bool(use_inferred_actions)
        self._sim, self._cost, self._sampler = simulator, cost, sampler
        self.n_iters, self.batch_size, self.elite_frac, self.max_seq_len = n_iters, batch_size, elite_frac, max_seq_len
        self.goal_in_cost = goal_in_cost
        self.logs = []
        # verbose (cem_params.verbose, cem_planner.py:72-88): every call appends to `verbose_logs` one list holding, per iteration, the
        # elites' rollouts and states, and last the final rollout (`elite_log_entry`).  Off: nothing is kept, copied or launched for it
        self.verbose, self.verbose_logs, self._last_eval = bool(verbose), [], None
        # receding-horizon options of plan_batch, which the reference's CEM does not have (all off by default):
        # noise_rho in [0, 1): AR(1) correlation of the noise along the steps; keep_elites in [0, 1): the fraction of the elites carried
        # into the next iteration's population; warm_std in (0, 1]: the std, in units of the initial one, on the steps of a warm start
        self.noise_rho, self.keep_elites, self.warm_std = 0.0, 0.0, 1.0
        self.set_receding(noise_rho=noise_rho, keep_elites=keep_elites, warm_std=warm_std)
        self.batch_best = None

    def set_receding(self, noise_rho=None, keep_elites=None, warm_std=None):
        """the receding-horizon options, validated; None leaves one as it is"""
        for name, v, ok, rng in (("noise_rho", noise_rho, lambda x: 0.0 <= x < 1.0, "[0, 1)"), ("keep_elites", keep_elites, lambda x: 0.0 <= x < 1.0, "[0, 1)"),
                                 ("warm_std", warm_std, lambda x: 0.0 < x <= 1.0, "(0, 1]")):
            if v is None:
                continue
            if not ok(float(v)):                             # (a NaN fails every comparison)
                raise ValueError(f"CEMPlanner: {name} = {v} outside {rng}")
            setattr(self, name, float(v))

    def _shard(self, n):
        world = D.dist.get_world_size() if D.dist.is_initialized() else 1
        rank = D.dist.get_rank() if D.dist.is_initialized() else 0
        assert n % world == 0, "candidate population must divide evenly over ranks"
        per = n // world
        return rank * per, per

    def _cap(self, r):
        """_cap_to_horizon on a padded device rollout: the cost and the logs read the first min(length, horizon) steps"""
        if self.horizon is not None:
            r.lengths = r.lengths.clamp(max=self.horizon)
        return r

    def _cap_list(self, seqs):
        """_cap_to_horizon (cem_planner.py:151-155) on the host lists of the final rollout"""
        if self.horizon is None or seqs is None:
            return seqs
        return [x[:self.horizon] for x in seqs]

    def _action_plan(self, final_actions, best_sample):
        """_get_action_plan (cem_planner.py:143-149) for one plan: the final rollout's actions, or the best sample itself (numpy)"""
        if self.use_inferred_actions:
            return final_actions
        b = best_sample.detach().cpu().numpy() if torch.is_tensor(best_sample) else np.asarray(best_sample)
        return b

    def evaluate(self, state, goal_state, samples):
        """costs [n] of all candidates given the WHOLE population: this rank rolls out its slice, one all-gather assembles the vector."""
        lo, per = self._shard(samples.shape[0])
        return self._evaluate_local(state, goal_state, samples[lo:lo + per], lo, samples.shape[0])

    def _evaluate_local(self, state, goal_state, local, lo, n_total):
        per = local.shape[0]
        if getattr(self._sim, "supports_latent_only", False):
            kw = {}
            if getattr(self._sim, "pred_length", False) and hasattr(self._sampler, "sample_uniform"):
                # every rank draws the population's length numbers (n floats) from the shared stream and keeps its slice
                kw["len_u"] = self._sampler.sample_uniform(n_total)[lo:lo + per]
            r = self._sim.rollout_device(state, goal_state, local, self.max_seq_len, decode=self.decode_candidates, **kw)
        else:                                            # any simulator with the reference's interface
            r = self._sim.rollout_device(state, goal_state, local, self.max_seq_len)
        self._cap(r)
        if hasattr(self._cost, "sequence_cost_device"):
            cost = self._cost.sequence_cost_device(r.latents, r.lengths, r.e_goal if self.goal_in_cost else None)
        else:
            # a hand-written CostFcn scores the rollouts' `predictions` against the goal state (cem_planner.py:126): image ++ latent
            # rows of the padded device rollout, one launch
            cost = self._cost.rollout_cost_device(self._sim.predictions_device(r), r.lengths, goal_state)
        return D.all_gather_costs(cost), r

    def iterate(self, state, goal_state):
        """One CEM iteration (cem_planner.py:68-79): draw, roll out, score, pick elites, refit.  Under a process group every rank
        draws and rolls out ONLY its own shard of the population (1 / world of the work), the costs are all-gathered, every rank
        picks the same elites from the full cost vector, and the elite latents — rows of whichever rank drew them — are assembled by
        one all-reduce of the rank's masked contribution (exactly one non-zero contributor per row: x + 0 + ... = x bit-exactly;
        n_elite x N x nz floats, 6.6 MB at 51 x 127 x 256).  Returns (elite samples, elite scores, all scores)."""
        n = self.batch_size
        n_elite = max(int(n * self.elite_frac), 1)
        world = D.dist.get_world_size() if D.dist.is_initialized() else 1
        if world == 1:
            samples = self._sampler.sample(n)
            scores, r = self._evaluate_local(state, goal_state, samples, 0, n)
            idx = select_elites(scores, n_elite)
            best = samples[idx]
            if self.verbose:
                self._last_eval = (r, idx)
        else:
            assert self._sampler.n_shards() == world, "one shard of the population per rank"
            lo, per = self._shard(n)
            local = self._sampler.sample_shard(n, D.dist.get_rank())
            scores, _ = self._evaluate_local(state, goal_state, local, lo, n)
            idx = select_elites(scores, n_elite)
            mine = (idx >= lo) & (idx < lo + per)
            best = torch.zeros((n_elite,) + tuple(local.shape[1:]), device=local.device, dtype=local.dtype)
            best[mine] = local[idx[mine] - lo]
            D.dist.all_reduce(best)
        best_scores = scores[idx]
        self._sampler.fit(best, best_scores)
        return best, best_scores, scores

    def __call__(self, state, goal_state):
        """the reference's contract (cem_planner.py:96): (image_plan, actions, latents, cost)"""
        r = self.plan(state, goal_state)
        return r.predictions, r.actions, r.latents, r.cost

    def plan(self, state, goal_state):
        """the plan as Outputs(predictions, actions, latents, cost, states): `states` are the final rollout's regressed states
        [len, state_dim], None when the simulator's model has no state regressor"""
        self._sampler.init()
        n_elite = max(int(self.batch_size * self.elite_frac), 1)
        best_samples = best_scores = None
        self.logs = []
        if self.verbose:
            assert not D.dist.is_initialized() or D.dist.get_world_size() == 1, "verbose planner logs: one process (the elites' rollouts " \
                                                                                   "live on the rank that drew them)"
            vlog = []
        for _ in range(self.n_iters):
            best_samples, best_scores, scores = self.iterate(state, goal_state)
            self.logs.append(Outputs(elite_scores=best_scores.clone(), mean_score=scores.mean()))
            if self.verbose:
                r, idx = self._last_eval
                lens = r.lengths[idx].tolist()
                vlog.append(elite_log_entry(
                    goal_state, best_scores,
                    images=None if r.images is None else [r.images[i, :l].clone() for i, l in zip(idx.tolist(), lens)],
                    latents=[r.latents[i, :l].clone() for i, l in zip(idx.tolist(), lens)],
                    states=None if r.states is None else [r.states[i, :l].clone() for i, l in zip(idx.tolist(), lens)]))
                self._last_eval = None
        # final rollout of the best candidate (cem_planner.py:81-96); every rank computes it (tiny batch)
        kw = {}
        if getattr(self._sim, "pred_length", False) and hasattr(self._sampler, "sample_uniform"):
            kw["len_u"] = self._sampler.sample_uniform(1)             # the plan's own length draw, from the rank-shared stream
        final = self._sim.rollout(state, goal_state, best_samples[:1].cpu().numpy(), self.max_seq_len, **kw)
        if self.horizon is not None:
            final = Outputs({k: self._cap_list(v) for k, v in final.items()})
        actions = self._action_plan(final.actions[0] if final.actions is not None else None, best_samples[0])
        states = final.get("states")
        if self.verbose:
            vlog.append(final_log_entry(final, goal_state, best_scores, final.latents[0].shape[-1] if self._sim._append_latent else 0))
            self.verbose_logs.append(vlog)
        return Outputs(predictions=final.predictions[0], actions=actions, latents=final.latents[0], cost=float(best_scores[0]),
                       states=states[0] if states is not None else None)

    # K tasks per forward: at most this many candidate rows in one scoring forward (HierarchicalCEMPlanner.MAX_ROWS)
    MAX_ROWS = 1000
    device_plans = True           # plan_batch(device=True) hands the plans over on the device (control.ControlRunner(keep_plans=False))

    def plan_batch(self, states, goals, record=False, max_rows=None, len_u=None, device=False, latents=True, warm=None):
        """K tasks planned together: states, goals [K, H, W, 3] env images -> a list of K Outputs with the fields of `plan`.
        device: the plans stay on the device (`_device_plans`: no decoded final rollout, no host lists; states and goals may be device
        tensors, which then never visit the host); latents: whether the caller reads the plans' latents (closed-loop acting).
        The K Gaussians mean, std [K, n_steps, dim] live in this call, initialised as `sampler.init()` does; the sampler's own mean / std
        are not touched.  Every iteration is one noise draw [K, n, n_steps, dim] from the sampler's rank-shared generator, one launch
        for the K populations (gcpx_cem_population), the scoring rollout of the K * n rows -- task k's rows with its own start and goal
        image, whole tasks per forward, at most `max_rows` rows (default MAX_ROWS), each forward scored before the next -- one launch
        for the elites of all tasks (gcpx_cem_elites) and one for the refit (gcpx_cem_refit); nothing is read back inside the loop.
        Then one decoded rollout of the K best candidates, and the K costs in one copy.

        Not the bits of `plan` task by task: the generator is consumed in another order, a forward of K * n rows need not equal one
        of n rows in the last bits (HierarchicalCEMPlanner.plan_batch), and the refit sums the elites one at a time where `fit` calls
        torch.mean / torch.std -- the same search on another sample.
        Out of scope, ValueError: verbose logs (defined per plan); a population sharded over ranks or sampler shards; PDDMSampler,
        whose correlated draw and score-weighted refit the kernels do not compute.
        record: `self.batch_record` keeps, per iteration, the noise blocks, populations, per-row scores, elite indices, the means and
        stds after the refit, the scoring rollouts' (latents, lengths) and goal latents, and `best_samples` [K, n_steps, dim].
        len_u: f(rows) -> the length draws of a forward of that many rows; default, for a simulator that predicts lengths:
        sampler.sample_uniform(rows) per forward.
        self.logs: per iteration Outputs(elite_scores [K, n_elite], mean_score [K]).  self.batch_best: `best` [K, n_steps, dim] of the call,
        on the sampler's device.

        Receding-horizon options (none in the reference; all off by default, and then the launches and draws are the ones above):
        warm = (prev [K, n_steps, dim] float32 on the sampler's device, shift int32 [K]): the search starts at the previous best samples
        moved up by the steps executed since (gcpx_cem_warm_start: std warm_std * initial_std on the steps the old plan covers, the cold
        start behind them and for a task with shift < 0); prev None: nobody has a previous plan, a cold start for all.
        keep_elites: from the second iteration on, rows 0 .. m-1 of a task's population, m = floor(keep_elites * n_elite), are the previous
        iteration's elites in rank order, read from the previous population (kept alive until then) through the previous idx; in a call
        with `warm` and m >= 1, row 0 of the first population is the task's starting mean itself.  Carried rows are rolled out and scored
        like every other row.  noise_rho: the noise of a candidate is an AR(1) sequence along the steps.  Both through
        gcpx_cem_population_ex; the noise draw stays randn(K, n, n_steps, dim) per iteration whatever m is (rows < m of it are ignored), so
        the generator's position does not depend on the options.  record also keeps `start_mean`, `start_std` and `m`."""
        s = self._sampler
        if self.verbose:
            raise ValueError("plan_batch keeps no verbose logs (they are defined per plan): use plan()")
        if isinstance(s, PDDMSampler):
            raise ValueError("plan_batch does not implement PDDMSampler (correlated draws, score-weighted refit): use plan()")
        if not isinstance(s, FlatCEMSampler):
            raise ValueError(f"plan_batch needs a FlatCEMSampler, not {type(s).__name__}")
        if s.n_shards() != 1:
            raise ValueError(f"plan_batch does not shard its populations ({s.n_shards()} sampler shards / ranks): use plan()")
        if s._dtype != torch.float32:
            raise ValueError("plan_batch keeps its distributions in float32")
        if not (device and torch.is_tensor(states) and torch.is_tensor(goals)):
            states, goals = np.asarray(states), np.asarray(goals)
        if states.ndim != 4 or states.shape != goals.shape:
            raise ValueError("plan_batch takes states and goals [K, H, W, 3]")
        # (a hand-written cost takes its goal on the host, cost_fcn.py's contract: the goal frames, not the start frames, come back once)
        cost_goals = goals.cpu().numpy() if torch.is_tensor(goals) and not hasattr(self._cost, "sequence_cost_device") else goals
        K, n = states.shape[0], self.batch_size
        n_elite = max(int(n * self.elite_frac), 1)
        max_rows = self.MAX_ROWS if max_rows is None else int(max_rows)
        sim, dev = self._sim, s.device
        if len_u is None and getattr(sim, "pred_length", False):
            len_u = s.sample_uniform
        elif not getattr(sim, "pred_length", False):
            len_u = None
        learned = hasattr(self._cost, "sequence_cost_device")
        m = int(self.keep_elites * n_elite)
        extended = self.noise_rho != 0.0 or m > 0                # the default goes through gcpx_cem_population, as it always has
        if warm is not None and warm[0] is not None:
            prev, shift = warm
            if not torch.is_tensor(prev) or prev.dtype != torch.float32 or tuple(prev.shape) != (K, s._n_steps, s._action_dim) \
                    or prev.device.type != dev.type:
                raise ValueError(f"plan_batch: warm[0] is the previous best samples, float32 [K, n_steps, dim] = {(K, s._n_steps, s._action_dim)} "
                                 f"on {dev}")
            if not torch.is_tensor(shift) or shift.dtype != torch.int32 or tuple(shift.shape) != (K,):
                raise ValueError("plan_batch: warm[1] is the executed steps of every task, int32 [K]")
            mean, std = cem_warm_start(prev, shift.to(dev), s._initial_std, self.warm_std)
        else:
            mean = torch.zeros(K, s._n_steps, s._action_dim, device=dev)
            std = s._initial_std * torch.ones(K, s._n_steps, s._action_dim, device=dev)
        rec = Outputs(noise=[], populations=[], scores=[], elite_idx=[], means=[], stds=[], rollouts=[], goal_latents=[], best_samples=None,
                      start_mean=mean, start_std=std, m=m)
        kept, task0 = [], [0]

        def score(r, chunk_goals):
            lo = task0[0]                                    # the forwards of an iteration take the tasks in order
            task0[0] = (lo + len(chunk_goals)) % K
            self._cap(r)
            if record:
                kept.append((r.latents.clone(), r.lengths.clone(), r.e_goal.clone()))
            if learned:
                return self._cost.sequence_cost_device(r.latents, r.lengths, r.e_goal if self.goal_in_cost else None)
            return self._cost.rollout_cost_rows_device(sim.predictions_device(r), r.lengths,
                                                       [g[None] for g in cost_goals[lo:lo + len(chunk_goals)]], repeat=n)

        self.logs, best, elite_scores = [], None, None
        pop = idx = None
        for it in range(self.n_iters):
            eps = torch.randn(K, n, s._n_steps, s._action_dim, device=dev, generator=s._gen)
            if not extended:
                pop = cem_population(mean, std, eps, s._clip_val, inplace=not record)
            else:
                # `pop` and `idx` are still the previous iteration's here: eps is a buffer of its own, and the old population stays
                # referenced until the launch that reads it has been issued
                if it > 0:
                    carry = (pop, idx[:, :m], m)
                elif warm is not None and m >= 1:            # the starting mean itself is a candidate: one row, index 0
                    carry = (mean[:, None], torch.zeros(K, 1, dtype=torch.int32, device=dev), 1)
                else:
                    carry = (None, None, 0)
                pop = cem_population_ex(mean, std, eps, s._clip_val, self.noise_rho, *carry, inplace=not record)
            parts = rollout_chunks(sim, self.max_seq_len, states, goals, pop.reshape((K * n,) + tuple(pop.shape[2:])), n, max_rows, False,
                                   len_u, each=score, decode_device=self.decode_candidates)
            scores = (parts[0] if len(parts) == 1 else torch.cat(parts)).reshape(K, n)
            idx, elite_scores = cem_elites(scores, n_elite)
            mean, std, best = cem_refit(pop, idx)
            self.logs.append(Outputs(elite_scores=elite_scores, mean_score=scores.mean(dim=1)))
            if record:
                for key, v in (("noise", eps), ("populations", pop), ("scores", scores), ("elite_idx", idx), ("means", mean), ("stds", std),
                               ("rollouts", (torch.cat([p[0] for p in kept]), torch.cat([p[1] for p in kept]))),
                               ("goal_latents", torch.cat([p[2] for p in kept]))):
                    rec[key].append(v)
                kept.clear()
        rec.best_samples = self.batch_best = best
        self.batch_record = rec if record else None
        if device:
            return self._device_plans(states, goals, best, elite_scores[:, 0], max_rows, len_u, latents)
        costs = elite_scores[:, 0].cpu().numpy()
        out = []
        for k0, final in zip(range(0, K, max(max_rows, 1)), rollout_chunks(sim, self.max_seq_len, states, goals, best, 1, max_rows, True, len_u)):
            if self.horizon is not None:
                final = Outputs({k: self._cap_list(v) for k, v in final.items()})
            st = final.get("states")
            for j in range(len(final.predictions)):
                out.append(Outputs(predictions=final.predictions[j],
                                   actions=self._action_plan(final.actions[j] if final.actions is not None else None, best[k0 + j]),
                                   latents=final.latents[j], cost=float(costs[k0 + j]), states=st[j] if st is not None else None))
        return out

    def _device_plans(self, states, goals, best, costs, max_rows, len_u, latents):
        """plan_batch(device=True): the K plans as device tensors, nothing decoded and nothing copied to the host.
        Outputs(best [K, n_steps, dim], costs [K], lengths int32 [K] (frames of each plan, the horizon applied), actions [K, A, n_actions]
        with n_actions [K] valid rows each (the final rollout's inverse-model actions, or the best samples themselves), and latents
        [K, T, nz_enc] or None).  The final rollout of the K best candidates runs only when something reads it: the caller's `latents`,
        the inverse-model actions, or a simulator that draws its lengths (whose draws are then consumed as the host path consumes them)."""
        sim, K, dev = self._sim, best.shape[0], best.device
        pred_length = bool(getattr(sim, "pred_length", False))
        lat = act = lens = None
        if latents or self.use_inferred_actions or pred_length:
            keep = lambda r, _goals: (r.latents.clone(), r.lengths.clone(), None if r.actions is None else r.actions.clone())
            parts = rollout_chunks(sim, self.max_seq_len, states, goals, best, 1, max_rows, False, len_u, each=keep, decode_device=False)
            lat, lens = torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
            if parts[0][2] is not None:
                act = torch.cat([p[2] for p in parts])
        else:
            lens = torch.full((K,), self.max_seq_len, dtype=torch.int32, device=dev)
        # the host contract: one action per frame transition (GCPImageSimulator.rollout: actions[:length - 1]), then frames, latents and
        # actions alike cut to their first `horizon` entries
        n_act = (lens - 1).clamp(min=0)
        if self.horizon is not None:
            lens, n_act = lens.clamp(max=self.horizon), n_act.clamp(max=self.horizon)
        if self.use_inferred_actions:
            if act is None:                                  # no inverse model: an empty action plan (ImageCEMPolicy.get_action)
                act, n_act = torch.zeros(K, 1, 2, device=dev), torch.zeros_like(lens)
        else:
            act, n_act = best, torch.full((K,), best.shape[1], dtype=torch.int32, device=dev)
        return Outputs(best=best, costs=costs, lengths=lens, actions=act, n_actions=n_act, latents=lat if latents else None)


class ImageHierarchicalTreeCEMSampler:
    """sampler.py:79-143: draws come from the hierarchical latent optimizer, one tree level is fixed per iteration."""

    def __init__(self, clip_val, n_steps, action_dim, initial_std, n_level_hierarchy, sampling_rates_per_layer,
                 subgoal_cost_fcn, ll_cost_fcn, n_ll_samples, device_resident=False, rng=None):
        from .tree_latent_search import ImageHierarchicalTreeLatentOptimizer, DeviceHierarchicalTreeLatentOptimizer
        self._cls = DeviceHierarchicalTreeLatentOptimizer if device_resident else ImageHierarchicalTreeLatentOptimizer
        self.device_resident = device_resident
        self._clip_val, self._action_dim, self._n_levels = clip_val, action_dim, n_level_hierarchy
        self._rates, self._sub_cost, self._ll_cost, self._n_ll = list(sampling_rates_per_layer), subgoal_cost_fcn, ll_cost_fcn, n_ll_samples
        self._rng = rng                  # None: the reference's np.random stream; a np.random.Generator: tree_latent_search._draw
        assert n_level_hierarchy >= len(self._rates)
        self.init()

    def init(self):
        self._optimizer = self._cls(self._action_dim, self._rates.copy(), self._n_levels, self._sub_cost, self._ll_cost, self._n_ll,
                                    rng=self._rng)

    def sample(self, n_samples=None):
        z = self._optimizer.sample()
        if torch.is_tensor(z):                                      # (generator mode on the device)
            return z.clamp(-self._clip_val, self._clip_val) if np.isfinite(self._clip_val) else z
        return np.clip(z, -self._clip_val, self._clip_val)

    def optimize(self, rollouts, goal):
        best_rollout, best_cost = self._optimizer.optimize(rollouts, goal)
        if (best_rollout[-1] != goal[0].transpose(2, 0, 1)).any():      # sampler.py:138-139
            best_rollout = np.concatenate((best_rollout, goal.transpose(0, 3, 1, 2)))
        if not hasattr(best_cost, "__len__"):
            best_cost = [best_cost]
        return [best_rollout], best_cost

    def optimize_device(self, rollout, goal_image=None):
        """device-resident variant (tree_latent_search.DeviceHierarchicalTreeLatentOptimizer): `rollout` is what
        GCPImageSimulator.rollout_device returns; the plan comes back as (row, frame) references + its cost"""
        plan, best_cost = self._optimizer.optimize(rollout)
        return [plan], [best_cost]

    def materialize(self, plan, goal_image=None):
        return self._optimizer.materialize(plan, goal_image)

    def fit(self, *args, **kwargs):
        pass

    append_latent = True

    @property
    def fully_optimized(self):
        return self._optimizer.fully_optimized


class HierarchicalCEMPlanner:
    """HierarchicalImageCEMPlanner (cem_planner.py:166-218 with :55-96): n_iters = len(sampling_rates) + 1 rounds of
    sample -> rollout -> optimise one level.  Populations are tiny (10, 10, 5 in the 25-room config), so ranks run
    replicas; the flat `CEMPlanner` is the sharded one."""

    def __init__(self, simulator, cost, n_level_hierarchy, sampling_rates_per_layer, n_ll_samples=5, action_dim=256,
                 max_seq_len=80, clip_val=float("inf"), device_resident=True, fast_draws=False, seed=0, verbose=False):
        # device_resident: the rollouts of every iteration stay on the device — subgoal pair costs, segment costs and the
        # selections are computed there and only the final plan crosses to the host.  False = the reference's data flow (every
        # rollout, image ++ latent, to numpy: cem_simulator.py:68-70), kept as the checker: both give the same search.
        self._sim, self.max_seq_len = simulator, max_seq_len
        self.n_iters = len(sampling_rates_per_layer) + 1
        self.device_resident = bool(device_resident and hasattr(simulator, "rollout_device") and hasattr(cost, "sequence_cost_device"))
        # fast_draws: the search draws from np.random.default_rng(seed) and only the rows it keeps (tree_latent_search._draw) instead
        # of replaying the reference's np.random call sequence — same distribution of searches, a call is no longer bound by the host's
        # Gaussian generator.  False (default) = the reference's stream, draw for draw.
        self._sampler = ImageHierarchicalTreeCEMSampler(clip_val, max_seq_len, action_dim, 1.0, n_level_hierarchy,
                                                        sampling_rates_per_layer, cost, cost, n_ll_samples,
                                                        device_resident=self.device_resident,
                                                        rng=self._make_rng(fast_draws, seed))
        self.logs = []
        self.verbose, self.verbose_logs = bool(verbose), []         # as CEMPlanner's

    def _make_rng(self, fast_draws, seed):
        """fast_draws: False -> None (the reference's np.random stream); True -> a seeded generator — on the model's device when the
        search is device-resident (the population is then drawn where the rollout reads it), numpy's otherwise"""
        if not fast_draws:
            return None
        dev = getattr(getattr(self._sim, "_model", None), "device", None)
        if self.device_resident and dev is not None and dev.type == "cuda":
            g = torch.Generator(device=dev)
            g.manual_seed(int(seed))
            return g
        return np.random.default_rng(seed)

    def __call__(self, state, goal_state):
        """the reference's contract (cem_planner.py:218): (image_plan, actions, latents, cost)"""
        r = self.plan(state, goal_state)
        return r.predictions, r.actions, r.latents, r.cost

    def plan(self, state, goal_state):
        """the plan as Outputs(predictions, actions, latents, cost, states), as CEMPlanner.plan"""
        self._sampler.init()
        self.logs = []
        goal = np.asarray(goal_state)
        best_samples = best_scores = None
        vlog = []
        for it in range(self.n_iters):
            samples = self._sampler.sample()
            if self.device_resident:
                # the learned cost reads latents only (cost_fcn.py:84-97): the scoring rollouts skip the image decoder
                r = self._sim.rollout_device(state, goal, samples, self.max_seq_len, decode=False)
                best_rollouts, best_scores = self._sampler.optimize_device(r)
            else:
                rollouts = self._sim.rollout(state, goal, samples, self.max_seq_len)
                best_rollouts, best_scores = self._sampler.optimize(rollouts.predictions, goal)     # cem_planner.py:215
            # :216 draws the population again after every round; only the last one (everything optimised: no randomness left in it) is
            # used.  The reference's stream has to consume the others' Gaussians to stay draw-for-draw; the generator mode skips them.
            if self._sampler._rng is None or it == self.n_iters - 1:
                best_samples = self._sampler.sample()
            self.logs.append(Outputs(elite_rollouts=best_rollouts, elite_scores=best_scores))
            if self.verbose:
                vlog.append(self._verbose_entry(r if self.device_resident else rollouts, best_rollouts, best_scores, goal))
        final = self._sim.rollout(state, goal, best_samples, self.max_seq_len)
        actions = final.actions[0] if final.actions is not None else None
        states = final.get("states")
        if self.verbose:
            vlog.append(final_log_entry(final, goal, best_scores, final.latents[0].shape[-1] if self._sim._append_latent else 0))
            self.verbose_logs.append(vlog)
        return Outputs(predictions=final.predictions[0], actions=actions, latents=final.latents[0],
                       cost=float(np.asarray(best_scores[0]).reshape(-1)[0]), states=states[0] if states is not None else None)

    # K tasks per forward: measured at the 25-room control shape — the scoring rollouts of whole tasks are chunked so
    # that one forward carries at most this many candidate rows
    MAX_ROWS = 1000

    def _rollout_chunks(self, states, goals, z, n, max_rows, decode, len_u):
        """sim.rollout_device (decode=False) / sim.rollout (decode=True) of K * n rows, task k's n rows with its own start and goal image,
        whole tasks per forward (`rollout_chunks`, shared with CEMPlanner.plan_batch)"""
        return rollout_chunks(self._sim, self.max_seq_len, states, goals, z, n, max_rows, decode, len_u)

    def plan_batch(self, states, goals, record=False, max_rows=None, len_u=None):
        """K tasks planned together: states, goals [K, H, W, 3] env images -> a list of K Outputs with the fields of `plan`.
        One walk of the search tree for all tasks (tree_latent_search.BatchedDeviceTreeLatentOptimizer): every iteration is one
        population draw, the scoring rollout of the K * n candidates (whole tasks per forward, at most `max_rows` rows), and one
        launch per decision over all tasks; nothing of the search is read back before the end.  Then one decoded rollout of the K
        optimised trees.  Under a process group every rank runs the whole batch, as `plan` does.

        Not the bits of `plan` task by task: the generator's draws are consumed in another order, and a forward of K * n rows need
        not equal one of n rows in the last bits (the encoder's split-f16 blocks share a scale among the frames a workgroup
        stages) — the same search on another sample, which is why this is a path of its own.  Needs the device-resident search on a
        device generator (`fast_draws`): the reference's np.random stream is defined per plan, and so are the verbose logs.
        record: keep the draw blocks, the populations, the scoring rollouts' latents and lengths and the optimizer in `self.batch_record`.
        len_u: f(rows) -> the length draws of a rollout of that many rows (default: the model's own), for pred_length simulators."""
        from .tree_latent_search import BatchedDeviceTreeLatentOptimizer
        s = self._sampler
        if self.verbose:
            raise ValueError("plan_batch keeps no verbose logs (they are defined per plan): use plan()")
        if not self.device_resident or not isinstance(s._rng, torch.Generator):
            raise ValueError("plan_batch needs the device-resident search with fast_draws on the model's device; the reference's np.random "
                             "stream is defined per plan: use plan()")
        states, goals = np.asarray(states), np.asarray(goals)
        if states.ndim != 4 or states.shape != goals.shape:
            raise ValueError("plan_batch takes states and goals [K, H, W, 3]")
        K = states.shape[0]
        max_rows = self.MAX_ROWS if max_rows is None else int(max_rows)
        opt = BatchedDeviceTreeLatentOptimizer(s._action_dim, s._rates.copy(), s._n_levels, s._sub_cost, s._ll_cost, s._n_ll, K, s._rng,
                                               record=record)
        clip = (lambda z: z.clamp(-s._clip_val, s._clip_val)) if np.isfinite(s._clip_val) else (lambda z: z)
        self.logs, rollouts, populations = [], [], []
        for it in range(self.n_iters):
            z = clip(opt.sample())                                                 # [K, n, nodes, dim]
            n = z.shape[1]
            (lat, lens), = self._rollout_chunks(states, goals, z.reshape((K * n,) + tuple(z.shape[2:])), n, max_rows, False, len_u)
            if record:
                populations.append(z)
                rollouts.append((lat.clone(), lens.clone()))
            cost = opt.optimize(Outputs(latents=lat, lengths=lens))
            self.logs.append(Outputs(elite_scores=cost))
        opt.record = False
        best = clip(opt.sample())[:, 0]                                            # everything optimised: no randomness left in it
        self.batch_record = Outputs(optimizer=opt, draws=opt.draws, populations=populations, rollouts=rollouts, best_samples=best) if record else None
        costs = cost.cpu().numpy()
        zb = best.cpu().numpy()
        out = []
        for k0, final in zip(range(0, K, max(max_rows, 1)), self._rollout_chunks(states, goals, zb, 1, max_rows, True, len_u)):
            st = final.get("states")
            for j in range(len(final.predictions)):
                out.append(Outputs(predictions=final.predictions[j], actions=final.actions[j] if final.actions is not None else None,
                                   latents=final.latents[j], cost=float(costs[k0 + j]), states=st[j] if st is not None else None))
        return out

    def _verbose_entry(self, r, best_rollouts, best_scores, goal):
        """cem_planner.py:215-218 as logged at :72-78: the elite rollout is the one optimised plan, the elite states are the states of
        ALL rollouts of the iteration.  Device-resident: the plan is (row, frame) references into the scoring rollout, which decoded
        nothing: its latents are gathered (the forward's buffers are reused by the next rollout), (-1, -1) marks the raw goal image."""
        if self.device_resident:
            plan = best_rollouts[0]
            rows = torch.tensor([[max(i, 0), max(t, 0)] for i, t in plan], device=r.latents.device)
            lat = r.latents[rows[:, 0], rows[:, 1]]
            lens = r.lengths.tolist()
            st = None if r.states is None else [r.states[i, :l].clone() for i, l in enumerate(lens)]
            return elite_log_entry(goal, best_scores, latents=[lat], goal_rows=[[k for k, (i, _) in enumerate(plan) if i < 0]], states=st)
        st = r.get("states")
        return elite_log_entry(goal, best_scores, images=[np.asarray(b) for b in best_rollouts],
                               states=None if st is None else [np.asarray(x) for x in st])

    @property
    def fully_optimized(self):
        return self._sampler.fully_optimized


class ImageCEMPolicy:
    """ImageCEMPolicy / CEMPolicy / PlannerPolicy (planner_policy.py:13-241) without the agent infrastructure: plan with the CEM
    planner when there is no plan, the plan is used up, or the re-planning interval comes round (`act`, :89-113); follow the plan
    open loop through its inverse-model actions or closed loop by re-inferring each action from the current image and the next
    planned latent (`_infer_action`, :222-227: `model.encoder(img)[0][:, :, 0, 0]` -> `model.inv_mdl.run_single`).
    batch_encode: `_infer_action` encodes with `model.encode_frames`, the frame-independent encoder (csrc/enc_frames.hip), in place of
    `model.encoder`: the actions a control.ControlRunner(batch_encode=True) computes for all its episodes in one launch, bit for bit
    (not the bits of the default path: exact f32 against split-f16, both within the oracle's tolerance)."""

    def __init__(self, model, planner, replan_interval=1, num_max_replans=10, closed_loop_execution=False, batch_encode=False):
        self.planner_model, self._cem_planner = model, planner
        self.replan_interval, self.num_max_replans, self.closed_loop_execution = replan_interval, num_max_replans, closed_loop_execution
        self.batch_encode = bool(batch_encode)
        if closed_loop_execution and not getattr(getattr(model, "_hp", None), "attach_inv_mdl", True):
            raise ValueError("closed_loop_execution = True needs the model's inverse model (attach_inv_mdl): every action is inferred from "
                             "the current image and the next planned latent (planner_policy.py:222-227)")
        self.reset()

    def reset(self):
        self.current_exec_step = None
        self.image_plan = self.action_plan = self.latent_plan = None
        self.plan_cost = None
        self.num_replans = 0

    def act(self, t=None, i_tr=None, state=None, images=None, goal_image=None):
        """images: the frames executed so far [t+1, 1, H, W, 3] or [t+1, H, W, 3] (env format); goal_image [1, H, W, 3]"""
        imgs = np.asarray(images)
        if imgs.ndim == 5:
            imgs = imgs[:, 0]
        if self.image_plan is None or self.image_plan.shape[0] - 1 <= self.current_exec_step \
                or (t % self.replan_interval == 0 and self.num_replans < self.num_max_replans):
            self._plan(imgs[t][None], goal_image, t)
            self.num_replans += 1
        out = Outputs(actions=self.get_action(imgs[t]))
        self.current_exec_step += 1
        return out

    def _plan(self, state, goal, step):
        self.image_plan, self.action_plan, self.latent_plan, self.plan_cost = self._cem_planner(state, goal)
        self.current_exec_step = 0

    def get_action(self, current_image):
        if self.closed_loop_execution:
            return self._infer_action(current_image, self.latent_plan[self.current_exec_step + 1])
        assert self.action_plan is not None          # need to attach inverse model to planner to get actions!
        if self.action_plan.size < 1:
            return 0.05 * np.random.rand(2, )
        return self.action_plan[self.current_exec_step]

    def _infer_action(self, current_img, target_latent):
        m = self.planner_model
        img = env2planner(np.asarray(current_img)[None]).to(m.device)
        enc_img0 = m.encode_frames(img) if self.batch_encode else m.encoder(img)[0][:, :, 0, 0]
        tl = torch.as_tensor(np.asarray(target_latent)[None], dtype=torch.float32, device=m.device)
        return m.inv_mdl.run_single(enc_img0, tl)[0].cpu().numpy()
