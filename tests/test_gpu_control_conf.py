"""`plan.py --experiment <mod_hyper.py>` on the device: a control configuration in the reference's format gives the same plan as the
planner built by hand with the same arguments and seed, the conf's `verbose` changes nothing in the plan, its pictures equal their
numpy mirrors byte for byte, and `build_policy` hands back a policy that acts.

Model shape of every test: 32 x 32, max_seq_len 12 (4 levels, 15 nodes), nz_enc = nz_mid = nz_vae = 32, nz_mid_lstm 64, 2 LSTM layers,
random weights, one start / goal pair."""
import os
import struct
import sys
import textwrap
import zlib

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from video_gcp_amd import conf_loader as CL  # noqa: E402
from video_gcp_amd import dataset as DS  # noqa: E402
from video_gcp_amd import image_log as IL  # noqa: E402
from video_gcp_amd import planning as P  # noqa: E402
from video_gcp_amd import visualization as V  # noqa: E402
from video_gcp_amd.hparams import GCPHParams  # noqa: E402
import topdown_fixture as TF  # noqa: E402

pytestmark = pytest.mark.gpu

CONF = textwrap.dedent('''
    import os.path
    from blox import AttrDict
    from gcp.planning.infra.agent.benchmarking_agent import BenchmarkAgent
    from gcp.planning.infra.envs.miniworld_env.multiroom3d.multiroom3d_env import TopdownMultiroom3dEnv
    from gcp.planning.planner_policy import ImageCEMPolicy
    from gcp.planning.cem.sampler import {sampler}
    from gcp.planning.cem.cem_planner import HierarchicalImageCEMPlanner
    from gcp.planning.cem.cost_fcn import {cost}
    from experiments.prediction.base_configs import gcp_tree as base_conf

    agent = AttrDict(type=BenchmarkAgent, env=(TopdownMultiroom3dEnv, dict(n_rooms=9)), T=24, image_height=32, image_width=32,
                     start_goal_confs=os.environ['GCP_DATA_DIR'] + '/start_goal')
    h_config = AttrDict(base_conf.model_config)
    h_config.update(dict(state_dim=2, ngf=16, max_seq_len=12, hierarchy_levels=4, nz_mid_lstm=64, n_lstm_layers=2, nz_mid=32, nz_enc=32,
                         nz_vae=32, regress_length=True, attach_state_regressor=True, attach_inv_mdl=True, attach_cost_mdl=True,
                         inv_mdl_params=AttrDict(n_actions=2, use_convs=False, build_encoder=False), untied_layers=True,
                         decoder_distribution='discrete_logistic_mixture'))
    h_config.pop("add_weighted_pixel_copy")
    cem_params = AttrDict(prune_final=True, horizon=12, action_dim=32, verbose={verbose}, n_level_hierarchy=4, sampler={sampler},
                          cost_fcn={cost}, cost_config=AttrDict(checkpt_path=os.environ['GCP_EXP_DIR'] + '/prediction/weights'),
                          {cem_extra})
    policy = AttrDict(type=ImageCEMPolicy, params=h_config, checkpt_path=cem_params.cost_config.checkpt_path,
                      cem_planner=HierarchicalImageCEMPlanner, cem_params=cem_params, replan_interval=agent.T + 2,
                      closed_loop_execution=True)
    config = AttrDict(current_dir=os.path.dirname(os.path.realpath(__file__)), start_index=0, end_index=99, agent=agent, policy=policy,
                      save_format=['raw'], data_save_dir=os.environ['GCP_EXP_DIR'] + '/control', split_train_val_test=False,
                      traj_per_file=1)
''')
HIER = dict(sampler="ImageHierarchicalTreeCEMSampler", cost="ImageLearnedCostEstimate",
            cem_extra="n_iters=3, batch_size=3, sampling_rates_per_layer=[3, 3]")
FLAT = dict(sampler="SimpleTreeCEMSampler", cost="ImageWrappedLearnedCostFcn", cem_extra="n_iters=2, batch_size=8, elite_frac=0.25")
HP = GCPHParams(batch_size=1, max_seq_len=12, img_sz=32, hierarchy_levels=4, nz_mid_lstm=64, n_lstm_layers=2, nz_mid=32, nz_enc=32,
                nz_vae=32, state_dim=2, ngf=16, n_actions=2)
SEED = 0


def _conf(folder, name, verbose, **kw):
    os.makedirs(folder, exist_ok=True)
    path = os.path.join(folder, name)
    with open(path, "w") as f:
        f.write(CONF.format(verbose=verbose, **kw))
    return path


def _argv(conf, folder):
    return ["--experiment", conf, "--data_dir", os.path.join(folder, "data"), "--exp_dir", os.path.join(folder, "exp"),
            "--random_weights", "1", "--nstart_goal_pairs", "1", "--seed", str(SEED)]


def _pair():
    """the seeded start / goal images plan.py makes without --pairs"""
    rng = np.random.RandomState(SEED)
    starts = rng.randint(0, 256, size=(1, 32, 32, 3)).astype(np.uint8)
    goals = rng.randint(0, 256, size=(1, 32, 32, 3)).astype(np.uint8)
    return starts, goals


def _first_stream():
    """Two models of one process draw different in-plan noise on purpose (replay._sync_rng_state mixes the model's index in the process
    into the stream's key), and a rollout's length is such a draw: every model of a comparison is made as the process's first, which
    is what the entry point's model is in a run of its own (see test_gpu_image_log).  Without fed numbers the length draw itself comes
    from torch's default CUDA generator (replay.py: `lu.uniform_()`), which a process seeds at random: it is seeded here."""
    from video_gcp_amd.model import GCPTreeModel
    GCPTreeModel._n_models = 0
    torch.cuda.manual_seed(SEED)


@pytest.fixture(scope="module", autouse=True)
def _model_counter():
    from video_gcp_amd.model import GCPTreeModel
    n = GCPTreeModel._n_models
    yield
    GCPTreeModel._n_models = max(n, GCPTreeModel._n_models) + 8      # later modules' models: streams none of these used


def _main(argv):
    from video_gcp_amd.plan import main
    _first_stream()
    return main(argv)


def _hand_model():
    from video_gcp_amd.model import GCPTreeModel
    from video_gcp_amd.params import init_params
    _first_stream()
    model = GCPTreeModel(HP, params=init_params(HP, seed=SEED), device=torch.device("cuda", 0))
    model.eval()
    return model


def _read_png(path):
    """uint8 [H, W, 3] of a PNG written by image_log.write_png (8-bit RGB, filter type 0 on every row)"""
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, size = 8, b"", None
    while pos < len(data):
        n, tag = struct.unpack(">I", data[pos:pos + 4])[0], data[pos + 4:pos + 8]
        if tag == b"IHDR":
            size = struct.unpack(">II", data[pos + 8:pos + 16])
        if tag == b"IDAT":
            idat += data[pos + 8:pos + 8 + n]
        pos += 12 + n
    W, H = size
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(H, 1 + 3 * W)
    assert (raw[:, 0] == 0).all()
    return raw[:, 1:].reshape(H, W, 3)


def _same_plan(z, r):
    assert np.array_equal(z["image_plan"], r.predictions) and np.array_equal(z["latents"], r.latents)
    assert np.array_equal(z["actions"], r.actions) and float(z["cost"]) == float(r.cost)
    assert np.isfinite(z["image_plan"]).all() and np.isfinite(float(z["cost"])) and z["image_plan"].shape[0] >= 2


@pytest.fixture(scope="module")
def assets(tmp_path_factory):
    folder = str(tmp_path_factory.mktemp("assets"))
    TF.write_assets(folder, TF.make_assets(seed=9, n_rooms=9, scale=48, cw=8, k=7))
    path = os.path.join(folder, "topdown_assets.npz")
    return path, DS.load_topdown_assets(path)


@pytest.fixture(scope="module")
def hier_run(tmp_path_factory, assets):
    """plan.py --experiment on the hierarchical conf with verbose=True, --out and --topdown_assets: (folder, out folder, results)"""
    folder = str(tmp_path_factory.mktemp("hier"))
    conf = _conf(folder, "mod_hyper.py", True, **HIER)
    out = os.path.join(folder, "out")
    res = _main(_argv(conf, folder) + ["--out", out, "--topdown_assets", assets[0]])
    return folder, out, res


def test_hierarchical_conf_plans_like_the_planner_built_by_hand(hier_run):
    folder, out, res = hier_run
    d = CL.planner_from_control_conf(CL.exec_control_conf(os.path.join(folder, "mod_hyper.py"), dict(GCP_DATA_DIR="/d", GCP_EXP_DIR="/e")))
    assert d.hp == HP and d.planner == "hierarchical"
    model = _hand_model()
    planner = P.HierarchicalCEMPlanner(P.GCPImageSimulator(model), P.LearnedCostEstimate(model), 4, [3, 3], n_ll_samples=5, action_dim=32,
                                       max_seq_len=12, fast_draws=True, seed=SEED + 1)
    r = planner.plan(*_pair())
    z = np.load(os.path.join(out, "plan_0.npz"))
    _same_plan(z, r)
    assert len(res) == 1 and res[0]["cost"] == float(r.cost) and res[0]["plan_len"] == r.predictions.shape[0]
    assert planner.verbose_logs == []                                # nothing is kept without verbose


def test_verbose_off_gives_the_same_plan(hier_run, tmp_path):
    folder, out, res = hier_run
    conf = _conf(str(tmp_path), "mod_hyper.py", False, **HIER)
    quiet = str(tmp_path / "out")
    res2 = _main(_argv(conf, str(tmp_path)) + ["--out", quiet])
    assert res2 == res
    assert os.listdir(quiet) == ["plan_0.npz"]                       # and no picture
    a, b = np.load(os.path.join(out, "plan_0.npz")), np.load(os.path.join(quiet, "plan_0.npz"))
    for k in ("image_plan", "actions", "latents", "cost"):
        assert np.array_equal(a[k], b[k]), k


def test_flat_conf_plans_like_the_planner_built_by_hand(tmp_path):
    conf = _conf(str(tmp_path), "mod_hyper.py", False, **FLAT)
    out = str(tmp_path / "out")
    _main(_argv(conf, str(tmp_path)) + ["--out", out])
    model = _hand_model()
    sampler = P.SimpleTreeCEMSampler(float("inf"), 12, 32, 0.3, n_level_hierarchy=4, device=torch.device("cuda", 0), seed=SEED + 1)
    planner = P.CEMPlanner(P.GCPImageSimulator(model), P.LearnedCostEstimate(model), sampler, n_iters=2, batch_size=8, elite_frac=0.25,
                           max_seq_len=12)
    r = planner.plan(*_pair())
    _same_plan(np.load(os.path.join(out, "plan_0.npz")), r)
    # flags the conf decides are refused beside it
    for extra in (["--planner", "hierarchical"], ["--iters", "5"], ["--config", "c1"], ["--candidates", "8"], ["--elite_frac", "0.5"]):
        with pytest.raises(ValueError, match=extra[0]):
            _main(_argv(conf, str(tmp_path)) + extra)
    with pytest.raises(ValueError, match="checkpoint"):              # a checkpoint path that does not resolve
        _main(["--experiment", conf, "--data_dir", str(tmp_path / "data"), "--exp_dir", str(tmp_path / "exp"), "--nstart_goal_pairs", "1"])


@pytest.mark.parametrize("kind", ["hierarchical", "flat"])
def test_verbose_pictures_equal_their_numpy_mirrors(kind, hier_run, assets, tmp_path):
    dev = torch.device("cuda", 0)
    if kind == "hierarchical":
        folder, out, _ = hier_run
    else:
        folder, out = str(tmp_path), str(tmp_path / "out")
        _main(_argv(_conf(folder, "mod_hyper.py", True, **FLAT), folder) + ["--out", out, "--topdown_assets", assets[0]])
    d = CL.planner_from_control_conf(CL.exec_control_conf(os.path.join(folder, "mod_hyper.py"), dict(GCP_DATA_DIR="/d", GCP_EXP_DIR="/e")))
    _first_stream()
    model, planner, _ = CL.build_policy(d, dev, seed=SEED, random_weights=True)
    assert planner.verbose
    starts, goals = _pair()
    r = planner.plan(starts, goals)
    _same_plan(np.load(os.path.join(out, "plan_0.npz")), r)          # the same call as the entry point's
    assert len(planner.verbose_logs) == 1
    n_iters = 3 if kind == "hierarchical" else 2
    vlog = planner.verbose_logs[0]
    assert len(vlog) == n_iters + 1                                  # every iteration, then the final rollout
    pics = IL.planner_pictures(model, vlog, starts, d.horizon, IL.TrajectoryRenderer(assets[1], dev))
    n_elites = [1] * 4 if kind == "hierarchical" else [2, 2, 1]      # hierarchical: the one optimised plan; flat: 8 * 0.25
    # hierarchical: the states of ALL rollouts of the iteration (cem_planner.py:218), 3 in the first (rates[0]); last: the final rollout
    n_trajs = [3, None, None, 1] if kind == "hierarchical" else [2, 2, 1]
    expected = set()
    for i, p in enumerate(pics):
        elites, states = p["sources"]["elites"], p["sources"]["states"]
        assert len(elites) == n_elites[i] and len(states) == (n_trajs[i] or len(states)) >= 1, (i, len(elites), len(states))
        assert all(e.shape[1:] == (3, 32, 32) and 2 <= e.shape[0] <= 13 and np.isfinite(e).all() for e in elites)
        want = dict(overview=V.plan_overview_numpy(elites, d.horizon), goal=goals[0],
                    inferStateTraj=V.render_trajectory_dist_numpy(assets[1], states[:1]),
                    inferStateTrajDist=V.render_trajectory_dist_numpy(assets[1], states))
        assert want["overview"].shape == (32 * len(elites), 32 * 12, 3)
        assert set(p["pictures"]) == set(want)
        for name, canvas in want.items():
            assert np.array_equal(p["pictures"][name], canvas), (i, name)
            path = os.path.join(out, f"plan_0_r0_iter{i}_{name}.png")
            assert np.array_equal(_read_png(path), canvas), path      # the file the entry point wrote
            expected.add(os.path.basename(path))
        S = assets[1]["S"]
        cw = assets[1]["cw"]
        assert not np.array_equal(want["inferStateTrajDist"], assets[1]["background"][cw:cw + S, cw:cw + S])     # something was drawn
    assert set(os.listdir(out)) == expected | {"plan_0.npz", "plan_0_inferStateTraj.png"}
    # the last entry is the final rollout: the plan that was returned
    flat = pics[-1]["sources"]["elites"][0].reshape(r.predictions.shape[0], -1)
    assert np.array_equal(flat, r.predictions[:, :flat.shape[1]])


def test_build_policy_acts(hier_run):
    folder, _, _ = hier_run
    d = CL.planner_from_control_conf(CL.exec_control_conf(os.path.join(folder, "mod_hyper.py"), dict(GCP_DATA_DIR="/d", GCP_EXP_DIR="/e")))
    with pytest.raises(ValueError, match="checkpoint"):
        CL.build_policy(d, torch.device("cuda", 0))
    model, planner, policy = CL.build_policy(d, torch.device("cuda", 0), seed=SEED, random_weights=True, verbose=False)
    assert policy.closed_loop_execution and policy.replan_interval == 26 and not planner.verbose
    starts, goals = _pair()
    out = policy.act(t=0, i_tr=0, images=starts, goal_image=goals)
    a = np.asarray(out.actions)
    assert a.shape == (model._hp.n_actions,) and np.isfinite(a).all()
    assert policy.image_plan is not None and policy.current_exec_step == 1 and policy.num_replans == 1
