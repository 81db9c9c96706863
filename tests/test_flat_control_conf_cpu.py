"""Control configurations that name the flat predictor (policy.model_cls = SequentialModel), no GPU.

1. a visual-MPC conf (base_configs.vmpc, act_cond, FlatCEMSampler, L2ImageCost, use_inferred_actions = False, horizon 5, replan_interval 1)
   and a latent-CEM conf over base_configs.gcp_sequential load to the descriptions conf_loader.build_policy builds from; every
   inconsistent combination raises a ValueError that names its key.
2. the horizon cap of the flat planner against the EXECUTED reference (tests/golden/make_ref_cem_horizon_goldens.py ->
   ref_cem_horizon.npz: cem_planner.py:115-122,143-155): horizon below, between, at and above the rollout lengths, with the inferred
   actions and with the best sample as the action plan.  planning.CEMPlanner replays the recorded draws on the CPU in float64, with the
   bounds of tests/test_planning_cpu.py's uncapped loop: the first population's scores and every elite index equal; everything after the
   first refit within 1e-13 relative (1e-12 for the std), because torch's and numpy's float64 mean / std sum in different orders."""
import os
import sys
import textwrap

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import video_gcp_amd  # noqa: E402,F401
from video_gcp_amd import conf_loader as CL  # noqa: E402
from test_planning_cpu import _FlatStubSim, _HostCostOnPadded, _ReplaySampler  # noqa: E402

T = 12
FLAT_CONF = textwrap.dedent('''
    from blox import AttrDict
    from gcp.planning.infra.agent.benchmarking_agent import BenchmarkAgent
    from gcp.planning.infra.envs.miniworld_env.multiroom3d.multiroom3d_env import TopdownMultiroom3dEnv
    from gcp.planning.planner_policy import ImageCEMPolicy
    from gcp.planning.cem.sampler import {sampler}
    from gcp.planning.cem.cem_planner import {planner}
    from gcp.planning.cem.cost_fcn import {cost}
    from gcp.prediction.models.sequential import SequentialModel
    from experiments.prediction.base_configs import {base} as base_conf

    agent = AttrDict(type=BenchmarkAgent, env=(TopdownMultiroom3dEnv, dict(n_rooms=9, crop_window=40)), T={agent_T}, image_height=32,
                     image_width=32)
    h_config = AttrDict(base_conf.model_config)
    h_config.update(dict(state_dim=2, ngf=16, max_seq_len=12, {widths}, {params}))
    h_config.pop("add_weighted_pixel_copy")
    cem_params = AttrDict(horizon={horizon}, action_dim={action_dim}, verbose=False, sampler={sampler}, cost_fcn={cost},
                          sampler_clip_val=2.0, initial_std=0.5, n_iters=2, batch_size=5, elite_frac=0.4{cem_extra})
    policy = AttrDict(type=ImageCEMPolicy, params=h_config, {model_cls}checkpt_path='none', cem_planner={planner},
                      cem_params=cem_params, replan_interval=1, num_max_replans=agent.T{policy_extra})
    config = AttrDict(start_index=0, end_index=99, agent=agent, policy=policy)
''')
SMALL = "nz_mid_lstm=64, n_lstm_layers=2, nz_mid=32, nz_enc=32"
# visual MPC (planner_policy.py:191-235 with act_cond, cem_simulator.py:99-104, base_configs/vmpc.py)
VMPC = dict(widths=SMALL, base="vmpc", sampler="FlatCEMSampler", planner="ImageCEMPlanner", cost="L2ImageCost", agent_T=6, horizon=5, action_dim=2,
            params="attach_inv_mdl=False, inv_mdl_params=AttrDict(n_actions=2, use_convs=False, build_encoder=False)",
            cem_extra=", use_inferred_actions=False, dense_cost=True, final_step_cost_weight=2.0", model_cls="model_cls=SequentialModel, ",
            policy_extra=", act_cond=True")
# CEM in the latents of the goal-conditioned flat predictor
SEQ_LATENT = dict(widths=SMALL, base="gcp_sequential", sampler="FlatCEMSampler", planner="ImageCEMPlanner", cost="ImageLearnedCostEstimate", agent_T=6,
                  horizon=12, action_dim=8,
                  params="nz_vae=8, attach_inv_mdl=True, inv_mdl_params=AttrDict(n_actions=2, use_convs=False, build_encoder=False)",
                  cem_extra="", model_cls="model_cls=SequentialModel, ", policy_extra=", closed_loop_execution=True")


def load(tmp_path, **kw):
    p = tmp_path / "mod_hyper.py"
    p.write_text(FLAT_CONF.format(**kw))
    return CL.planner_from_control_conf(CL.exec_control_conf(str(p), {}))


def test_visual_mpc_conf(tmp_path):
    d = load(tmp_path, **VMPC)
    hp = d.hp
    assert d.model_kind == "sequential" and d.planner == "flat" and d.sampler == "FlatCEMSampler" and d.cost == "L2ImageCost"
    assert hp.action_conditioned_pred and hp.non_goal_conditioned and hp.deterministic and hp.nz_vae == 0 and hp.n_actions == 2
    assert (hp.max_seq_len, hp.img_sz, hp.nz_enc, hp.nz_mid_lstm) == (T, 32, 32, 64) and not hp.attach_inv_mdl
    assert d.sampler_args == dict(clip_val=2.0, n_steps=T - 1, action_dim=2, initial_std=0.5)
    assert d.planner_args == dict(n_iters=2, batch_size=5, elite_frac=0.4, max_seq_len=T)
    assert d.act_cond is True and d.action_source == "samples" and d.horizon == 5
    assert d.cost_args == dict(dense_cost=True, final_step_weight=2.0)
    assert d.policy_args == dict(replan_interval=1, num_max_replans=6, closed_loop_execution=False)
    assert not [k for k in d.ignored if "act_cond" in k or "use_inferred_actions" in k]       # both take part now


def test_latent_conf(tmp_path):
    d = load(tmp_path, **SEQ_LATENT)
    assert d.model_kind == "sequential" and d.planner == "flat" and d.act_cond is False and d.action_source == "inverse_model"
    assert not d.hp.action_conditioned_pred and d.hp.nz_vae == 8 and d.hp.attach_inv_mdl
    assert d.sampler_args == dict(clip_val=2.0, n_steps=T - 1, action_dim=8, initial_std=0.5)
    assert d.horizon == T and d.policy_args == dict(replan_interval=1, num_max_replans=6, closed_loop_execution=True)
    # PDDMSampler is a flat sampler too
    assert load(tmp_path, **dict(SEQ_LATENT, sampler="PDDMSampler")).sampler == "PDDMSampler"


def test_key_classes():
    assert CL.key_classes("policy", "act_cond") == ["mapped"] and CL.key_classes("cem", "use_inferred_actions") == ["mapped"]
    assert CL.key_classes("cem", "use_delta_state_actions") == ["unbuilt"] and CL.key_classes("cem", "LL_cost_fcn") == ["unbuilt"]


TREE_EXTRA = ", n_level_hierarchy=4"
ERRORS = [
    # act_cond with no model_cls: the tree model takes no actions
    ("act_cond", dict(VMPC, model_cls="")),
    # act_cond over a predictor that is not action-conditioned
    ("act_cond|action_conditioned_pred", dict(VMPC, base="gcp_sequential", params=VMPC["params"] + ", nz_vae=8")),
    # action_dim of the wrong kind: the latent's width under act_cond, the action's width without
    ("action_dim", dict(VMPC, action_dim=8)),
    ("action_dim", dict(SEQ_LATENT, action_dim=2)),
    # a tree sampler with the flat predictor
    ("sampler", dict(SEQ_LATENT, sampler="SimpleTreeCEMSampler", cem_extra=TREE_EXTRA)),
    ("sampler", dict(SEQ_LATENT, sampler="ImageHierarchicalTreeCEMSampler", planner="HierarchicalImageCEMPlanner",
                     cem_extra=TREE_EXTRA + ", sampling_rates_per_layer=[3]")),
    ("sampler", dict(VMPC, sampler="SimpleTreeCEMSampler", cem_extra=VMPC["cem_extra"] + TREE_EXTRA)),
    # the best sample as the action plan, where the samples are latents
    ("use_inferred_actions", dict(SEQ_LATENT, cem_extra=", use_inferred_actions=False")),
    # closed-loop execution without an inverse model
    ("closed_loop_execution", dict(VMPC, policy_extra=", act_cond=True, closed_loop_execution=True")),
    # still not built
    ("use_delta_state_actions", dict(VMPC, cem_extra=VMPC["cem_extra"] + ", use_delta_state_actions=True")),
]


@pytest.mark.parametrize("key,conf", ERRORS, ids=[f"{i}-{k.split('|')[0]}" for i, (k, _) in enumerate(ERRORS)])
def test_inconsistent_confs_raise_and_name_the_key(tmp_path, key, conf):
    with pytest.raises(ValueError, match=key):
        load(tmp_path, **conf)


def test_horizon_with_the_hierarchical_sampler_raises(tmp_path):
    from nav_env_cases import CONF
    text = CONF.format(env_params="n_rooms=9, crop_window=40", env_cls="TopdownMultiroom3dEnv", T=6)
    assert "horizon=12" in text
    p = tmp_path / "mod_hyper.py"
    p.write_text(text.replace("horizon=12", "horizon=5"))
    env = dict(GCP_DATA_DIR="/nowhere/data", GCP_EXP_DIR="/nowhere/exp")
    with pytest.raises(ValueError, match="horizon"):
        CL.planner_from_control_conf(CL.exec_control_conf(str(p), env))
    # the same conf with the flat sampler over all tree latents caps its rollouts
    flat = text.replace("horizon=12", "horizon=5").replace("ImageHierarchicalTreeCEMSampler", "SimpleTreeCEMSampler") \
        .replace("n_iters=3, batch_size=3, sampling_rates_per_layer=[3, 3]", "n_iters=1, batch_size=5, elite_frac=1.0")
    p.write_text(flat)
    d = CL.planner_from_control_conf(CL.exec_control_conf(str(p), env))
    assert d.planner == "flat" and d.horizon == 5 and d.model_kind == "tree" and d.action_source == "inverse_model" and d.act_cond is False
    assert d.sampler_args["n_steps"] == 12                           # the tree model's confs are unchanged


def test_policy_checks_closed_loop_when_it_is_built():
    from video_gcp_amd.hparams import GCPHParams
    from video_gcp_amd.planning import ImageCEMPolicy

    class Model:
        _hp = GCPHParams(max_seq_len=12, img_sz=32, attach_inv_mdl=False)
    with pytest.raises(ValueError, match="closed_loop_execution"):
        ImageCEMPolicy(Model(), None, closed_loop_execution=True)
    assert ImageCEMPolicy(Model(), None, closed_loop_execution=False).current_exec_step is None


# ---- the horizon cap against the executed reference ----------------------------------------------------------------------------------------
def _golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "ref_cem_horizon.npz"))


def test_golden_covers_the_cases():
    g = _golden()
    steps, ad, n_iters, batch = (int(v) for v in g["shape"])
    lens = g["c0_it0_lengths"]
    assert [tuple(c) for c in g["cases"]] == [(h, i) for h in (2, 4, 6, 9) for i in (1, 0)]
    raw = g[f"c{len(g['cases']) - 1}_it0_lengths"]                   # horizon 9 caps nothing: the rollouts' own lengths
    assert raw.min() < 4 < raw.max() == steps and (lens == 2).all()  # 2 is below, 4 between, 6 at, 9 above
    assert np.array_equal(g["c2_it0_lengths"], np.minimum(raw, 4))   # the same first population in every case


@pytest.mark.parametrize("ci", range(8))
def test_horizon_cap_matches_executed_reference(ci):
    from video_gcp_amd.planning import CEMPlanner, EuclideanPathLength
    g = _golden()
    steps, ad, n_iters, batch = (int(v) for v in g["shape"])
    horizon, inferred = (int(v) for v in g["cases"][ci])
    goal, efrac = g["goal"], float(g["elite_frac"][0])
    eps = [g[f"it{it}_eps"] for it in range(n_iters)]
    sampler = _ReplaySampler(eps, float("inf"), steps, ad, 0.6, device="cpu", dtype=torch.float64)
    planner = CEMPlanner(_FlatStubSim(np.float64), _HostCostOnPadded(EuclideanPathLength(True, 2.0), goal), sampler, n_iters=n_iters,
                         batch_size=batch, elite_frac=efrac, max_seq_len=steps, horizon=horizon, use_inferred_actions=bool(inferred))
    sampler.init()
    for it in range(n_iters):
        best, best_scores, scores = planner.iterate(None, goal)
        if it == 0:                                                  # the first population is 0 + 0.6 eps on both sides: the same numbers
            assert np.array_equal(scores.numpy(), g[f"c{ci}_it{it}_scores"]), (ci, it)
        np.testing.assert_allclose(scores.numpy(), g[f"c{ci}_it{it}_scores"], rtol=1e-13, atol=0)
        n_elite = len(g[f"c{ci}_it{it}_elite_idx"])
        assert np.array_equal(torch.argsort(scores, stable=True)[:n_elite].numpy(), g[f"c{ci}_it{it}_elite_idx"]), (ci, it)
        np.testing.assert_allclose(best_scores.numpy(), g[f"c{ci}_it{it}_elite_scores"], rtol=1e-13)
        np.testing.assert_allclose(sampler.mean.numpy(), g[f"c{ci}_it{it}_mean"], rtol=1e-13, atol=1e-15)
        np.testing.assert_allclose(sampler.std.numpy(), g[f"c{ci}_it{it}_std"], rtol=1e-12, atol=1e-15)
    sampler._eps = list(eps)
    pred, actions, latents, score = planner(None, goal)
    want_pred, want_act, want_lat = g[f"c{ci}_plan_pred"], g[f"c{ci}_plan_actions"], g[f"c{ci}_plan_latents"]
    assert len(want_pred) <= horizon and len(want_lat) == len(want_pred)
    np.testing.assert_allclose(pred, want_pred, rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(actions, want_act, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(latents, want_lat, rtol=1e-13, atol=1e-15)
    assert np.asarray(pred).shape == want_pred.shape and np.asarray(actions).shape == want_act.shape
    assert abs(score - float(g[f"c{ci}_plan_score"][0])) <= 1e-12 * abs(score)
    if not inferred:
        assert np.asarray(actions).shape == (steps, ad)              # cem_planner.py:149: the best sample itself, not capped
