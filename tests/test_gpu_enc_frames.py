"""The frame-independent encoder on the device (csrc/enc_frames.hip: gcpx_encode_frames, GCPTreeModel.encode_frames) and the opt-in
path through ImageCEMPolicy, ControlRunner and the control entry point.

Against the oracle: the entry point called directly, at the project's latent bound 5e-5 + 1e-4 |x| (LAT_ATOL, LAT_RTOL of
tests/test_gpu_api.py), for the nav-env test model (32 x 32, nz_enc 32), c1 (32 x 32, nz_enc 128) and c1 at 64 x 64 (three pyramid layers).
Frame independence: bit for bit (torch.equal) -- F = 70 frames together, each alone, and in reversed order, at both image sizes; and
more frames than the 64 x 64 kernel has workgroups, where a workgroup strides over several frames.  The runner with batch_encode against
ImageCEMPolicy(batch_encode=True) driven one episode at a time: bit for bit as well, which is the point of the kernel."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import video_gcp_amd as V  # noqa: E402
from oracle import gcp_model_oracle as O  # noqa: E402
from video_gcp_amd import control as CT  # noqa: E402
from video_gcp_amd import dataset as DS  # noqa: E402
from video_gcp_amd import nav_env as NE  # noqa: E402
from video_gcp_amd import packing as pk  # noqa: E402
from video_gcp_amd import planning as P  # noqa: E402
from video_gcp_amd import runtime as rt  # noqa: E402
from video_gcp_amd.hparams import GCPHParams  # noqa: E402
from video_gcp_amd.model import GCPTreeModel  # noqa: E402
from helpers import assert_close, maxdiff  # noqa: E402
from nav_env_cases import CONF  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAT_ATOL, LAT_RTOL = 5e-5, 1e-4
T, CW, IMG = 6, 40, 32
NAV_HP = GCPHParams(batch_size=1, max_seq_len=12, img_sz=32, hierarchy_levels=4, nz_mid_lstm=64, n_lstm_layers=2, nz_mid=32, nz_enc=32,
                    nz_vae=32, state_dim=2, ngf=16, n_actions=2)
MODELS = {"nav": lambda: NAV_HP, "c1": lambda: V.config("c1"), "c1_64": lambda: V.config("c1", img_sz=64)}


@pytest.fixture(scope="module")
def lib():
    return rt.load_library()


@pytest.fixture(scope="module")
def models():
    """name -> (hp, state dict on the host, eval-mode model), built on first use and shared by the tests of the module"""
    n = GCPTreeModel._n_models
    cache = {}

    def get(name):
        if name not in cache:
            hp = MODELS[name]()
            sd = V.init_params(hp, seed=1, randomize_affine=True)
            cache[name] = (hp, sd, GCPTreeModel(hp, params=sd, device=torch.device("cuda", 0)).eval())
        return cache[name]
    yield get
    GCPTreeModel._n_models = max(n, GCPTreeModel._n_models) + 8      # later modules' models: streams none of these used


def frames_of(hp, F, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(F, 3, hp.img_sz, hp.img_sz, generator=g) * 2.0 - 1.0


# ---- the entry point against the oracle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(MODELS))
def test_entry_point_equals_the_oracle(lib, models, name):
    hp, sd, model = models(name)
    F, nz = 6, hp.nz_enc
    x = frames_of(hp, F, seed=5)
    x[4], x[5] = -1.0, 0.0                                           # four drawn frames, one all -1, one all 0
    ref = O.encoder(sd, hp, x, training=False)[0][:, :, 0, 0]
    blob = pk.pack_encoder_frames(sd, hp).to(DEV)
    xd = x.to(DEV)
    out = torch.full((F + 1, nz), float("nan"), device=DEV)          # one guard row behind the result
    st = lib.gcpx_encode_frames(xd.data_ptr(), blob.data_ptr(), out.data_ptr(), nz, F, hp.img_sz, hp.ngf, nz, hp.leaky_slope,
                                rt.current_stream())
    assert st == 0, lib.gcpx_last_error()
    torch.cuda.synchronize()
    got = out.cpu()
    old = model.encode(xd).cpu()
    print(f"{name}: max |encode_frames - oracle| = {maxdiff(got[:F], ref):.3e}, max |model.encode - oracle| = {maxdiff(old, ref):.3e}, "
          f"max |latent| = {float(ref.abs().max()):.3e}")
    assert torch.isfinite(got[:F]).all()
    assert torch.isnan(got[F]).all()                                 # the guard row is untouched
    assert_close(got[:F], ref, LAT_ATOL, LAT_RTOL, f"encode_frames {name}")
    assert (ref[4] != ref[5]).any() and (ref[0] != ref[1]).any()     # the rows are those of different frames


def test_strided_output_rows(lib, models):
    """row f goes to out + f * out_stride: the columns between the rows are not written"""
    hp, sd, model = models("nav")
    F, nz, stride = 3, hp.nz_enc, hp.nz_enc + 5
    xd = frames_of(hp, F, seed=6).to(DEV)
    out = torch.full((F, stride), float("nan"), device=DEV)
    assert model.encode_frames(xd, out=out[:, :nz]) is not None
    torch.cuda.synchronize()
    assert torch.isnan(out[:, nz:]).all() and torch.equal(out[:, :nz], model.encode_frames(xd))


# ---- frame independence ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c1", "c1_64"])
def test_a_frames_latent_does_not_depend_on_its_batch(models, name):
    hp, sd, model = models(name)
    F = 70
    xd = frames_of(hp, F, seed=7).to(DEV)
    together = model.encode_frames(xd)
    alone = torch.cat([model.encode_frames(xd[f:f + 1]) for f in range(F)], dim=0)
    rev = model.encode_frames(xd.flip(0).contiguous()).flip(0)
    torch.cuda.synchronize()
    assert together.shape == (F, hp.nz_enc) and torch.isfinite(together).all()
    assert torch.equal(together, alone)
    assert torch.equal(together, rev)
    assert not torch.equal(together[0], together[1])


def test_more_frames_than_workgroups(models):
    """a grid smaller than F: workgroups stride over the frames (the 64 x 64 kernel holds one workgroup per CU)"""
    hp, sd, model = models("c1_64")
    F = model.lib.gcpx_conv_grid() // 2 + 3
    base = frames_of(hp, 4, seed=8).to(DEV)
    xd = base[torch.arange(F, device=DEV) % 4].contiguous()
    got = model.encode_frames(xd)
    want = model.encode_frames(base)
    torch.cuda.synchronize()
    assert torch.equal(got, want[torch.arange(F, device=DEV) % 4])


# ---- no synchronisation between calls -------------------------------------------------------------------------------------------------------
def test_back_to_back_calls_need_no_host_sync(models):
    hp, sd, model = models("c1")
    xa, xb = frames_of(hp, 5, seed=9).to(DEV), frames_of(hp, 7, seed=10).to(DEV)
    want_a = model.encode_frames(xa).clone()
    torch.cuda.synchronize()
    want_b = model.encode_frames(xb).clone()
    torch.cuda.synchronize()
    oa, ob = torch.empty(5, hp.nz_enc, device=DEV), torch.empty(7, hp.nz_enc, device=DEV)
    ra = model.encode_frames(xa, out=oa)
    rb = model.encode_frames(xb, out=ob)                              # no host synchronisation in between
    assert ra is oa and rb is ob
    torch.cuda.synchronize()
    assert torch.equal(oa, want_a) and torch.equal(ob, want_b) and not torch.equal(oa[:5], ob[:5])


# ---- the weights follow the model -----------------------------------------------------------------------------------------------------------
def test_weights_follow_load_state_dict():
    hp = NAV_HP
    n = GCPTreeModel._n_models
    try:
        sd1, sd2 = V.init_params(hp, seed=1, randomize_affine=True), V.init_params(hp, seed=2, randomize_affine=True)
        xd = frames_of(hp, 4, seed=11).to(DEV)
        m = GCPTreeModel(hp, params=sd1, device=torch.device("cuda", 0)).eval()
        first = m.encode_frames(xd).clone()
        m.load_state_dict(sd2)
        fresh = GCPTreeModel(hp, params=sd2, device=torch.device("cuda", 0)).eval()
        got, want = m.encode_frames(xd), fresh.encode_frames(xd)
        torch.cuda.synchronize()
        assert torch.equal(got, want) and not torch.equal(got, first)
    finally:
        GCPTreeModel._n_models = max(n, GCPTreeModel._n_models) + 8


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals(models):
    hp, sd, model = models("nav")
    xd = frames_of(hp, 2, seed=12).to(DEV)
    model.train()
    try:
        with pytest.raises(ValueError):
            model.encode_frames(xd)
    finally:
        model.eval()
    with pytest.raises(ValueError):
        model.encode_frames(xd[:, :, :16, :16])
    with pytest.raises(ValueError):
        model.encode_frames(xd, out=torch.empty(3, hp.nz_enc, device=DEV))
    with pytest.raises(ValueError):
        model.encode_frames(xd[:0])
    assert model.encode_frames(xd).shape == (2, hp.nz_enc)


def test_sequential_model_inherits_it():
    from video_gcp_amd.sequential import GCPSequentialModel
    assert GCPSequentialModel.encode_frames is GCPTreeModel.encode_frames


# ---- the runner -----------------------------------------------------------------------------------------------------------------------------
# ShortPlans, Replay and the body of the closed-loop check are those of tests/test_gpu_nav_env.py: test_runner_record_is_consistent
class ShortPlans:
    """a planner whose plans are cut to n frames: a plan shorter than T, so that the episode has to plan again"""

    def __init__(self, planner, n):
        self.planner, self.n = planner, n

    def __call__(self, state, goal):
        img, act, lat, cost = self.planner(state, goal)
        return img[:self.n], act[:self.n - 1], lat[:self.n], cost


class Replay:
    """hands an ImageCEMPolicy the plans an episode of the runner made, in order, and checks the frame each was made from"""

    def __init__(self, plans, frames):
        self.plans, self.frames, self.calls = plans, frames, 0

    def __call__(self, state, goal):
        p = self.plans[self.calls]
        assert np.array_equal(np.asarray(state)[0], self.frames[p["t"]])
        self.calls += 1
        return p["image_plan"], p["action_plan"], p["latent_plan"], p["cost"]


@pytest.fixture(scope="module")
def nav_model():
    from video_gcp_amd.params import init_params
    n = GCPTreeModel._n_models
    m = GCPTreeModel(NAV_HP, params=init_params(NAV_HP, seed=0), device=torch.device("cuda", 0))
    m.eval()
    yield m
    GCPTreeModel._n_models = max(n, GCPTreeModel._n_models) + 8


def _planner(model):
    return ShortPlans(P.HierarchicalCEMPlanner(P.GCPImageSimulator(model), P.LearnedCostEstimate(model), 4, [3, 3], n_ll_samples=5,
                                               action_dim=32, max_seq_len=12, fast_draws=True, seed=1), 4)


def test_runner_with_batch_encode_equals_the_per_episode_policy(nav_model):
    """every action of the batched runner is what ImageCEMPolicy(batch_encode=True) gives for that episode's recorded frames and plans,
    bit for bit: the encoder's result for a frame does not depend on the frames beside it"""
    model, E = nav_model, 3
    env = NE.NavEnvBatch(9, CW, T, IMG, DEV)
    runner = CT.ControlRunner(model, _planner(model), env, replan_interval=T + 2, num_max_replans=10, closed_loop_execution=True,
                              batch_encode=True)
    tasks = NE.draw_tasks(9, 2, range(E))
    res = runner.run(tasks)
    assert res["full_traj"].shape == (E, T + 1, 3) and res["actions"].shape == (E, T, 2) and np.isfinite(res["actions"]).all()
    frames, goal_frames = env.frames.cpu().numpy(), env.goal_frames.cpu().numpy()
    for e in range(E):
        ref = NE.rollout_numpy(9, tasks["start"][e], tasks["goal"][e], res["actions"][e])
        assert np.array_equal(ref["full_traj"].view(np.uint32), res["full_traj"][e].view(np.uint32))
        replay = Replay(runner.plans[e], frames[e])
        policy = P.ImageCEMPolicy(model, replay, replan_interval=T + 2, num_max_replans=10, closed_loop_execution=True, batch_encode=True)
        planned_at = []
        for t in range(T):
            before = replay.calls
            a = np.asarray(policy.act(t=t, i_tr=0, images=frames[e, :t + 1], goal_image=goal_frames[e][None]).actions, dtype=np.float32)
            if replay.calls != before:
                planned_at.append(t)
            assert np.array_equal(a.view(np.uint32), res["actions"][e, t].view(np.uint32)), (e, t, a, res["actions"][e, t])
        assert planned_at == [p["t"] for p in runner.plans[e]] and replay.calls == len(runner.plans[e]) == res["n_replans"][e]
        # a plan of n <= 4 frames is used up after n - 1 steps: the next plan is made at that step
        lens = [p["image_plan"].shape[0] for p in runner.plans[e]]
        assert planned_at[0] == 0 and all(b - a == n - 1 for a, b, n in zip(planned_at[:-1], planned_at[1:], lens[:-1]))
        assert len(planned_at) >= 2 and planned_at[-1] + lens[-1] - 1 >= T


class Tape:
    """records the plans of a run in call order, then hands a second run the same plans (the planner's draws differ from call to call,
    so two runs are comparable only on the same plans) and checks that each is asked for from the same frame"""

    def __init__(self, planner):
        self.planner, self.tape, self.pos = planner, [], None

    def rewind(self):
        self.pos = 0

    def __call__(self, state, goal):
        if self.pos is None:
            self.tape.append((np.array(state), self.planner(state, goal)))
            return self.tape[-1][1]
        frame, plan = self.tape[self.pos]
        assert np.array_equal(np.asarray(state), frame)
        self.pos += 1
        return plan


def test_open_loop_runner_ignores_batch_encode(nav_model):
    """without closed_loop_execution no frame is encoded: on the same plans the flag changes no action"""
    model, E = nav_model, 3
    tasks = NE.draw_tasks(9, 2, range(E))
    tape, acts = Tape(_planner(model)), []
    for flag in (False, True):
        env = NE.NavEnvBatch(9, CW, T, IMG, DEV)
        runner = CT.ControlRunner(model, tape, env, replan_interval=T + 2, num_max_replans=10, closed_loop_execution=False,
                                  batch_encode=flag)
        acts.append(runner.run(tasks)["actions"])
        tape.rewind()
    assert len(tape.tape) >= 2 * E                                   # every episode planned again when its short plan ran out
    assert np.isfinite(acts[0]).all() and np.array_equal(acts[0].view(np.uint32), acts[1].view(np.uint32))


# ---- the entry point ------------------------------------------------------------------------------------------------------------------------
def test_control_main_with_batch_encode(tmp_path):
    conf = tmp_path / "mod_hyper.py"
    conf.write_text(CONF.format(env_params="n_rooms=9, crop_window=40, heading_smoothing=0.1, init_pos=None, goal_pos=None",
                                env_cls="TopdownMultiroom3dEnv", T=T))
    out = str(tmp_path / "out")
    res = CT.main(["--experiment", str(conf), "--data_dir", str(tmp_path / "data"), "--exp_dir", str(tmp_path / "exp"), "--random_weights", "1",
                   "--n_tasks", "2", "--task_seed", "3", "--out", out, "--batch_encode", "1"])
    with np.load(os.path.join(out, "control_results.npz")) as z:
        assert z["actions"].shape == (2, T, 2) and np.isfinite(z["actions"]).all() and np.array_equal(z["actions"], res["actions"])
        assert z["full_traj"].shape == (2, T + 1, 3) and np.isfinite(z["full_traj"]).all()
