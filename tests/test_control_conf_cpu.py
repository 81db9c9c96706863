"""Control configurations in the reference's format (gcp/planning/run.py <experiments/control/*/mod_hyper.py>): the loader
(conf_loader.exec_control_conf / planner_from_control_conf), the key table every reference hyper-parameter goes through
(conf_loader.KEY_TABLE against tests/golden/ref_hparam_defaults.json, the keys and defaults of the reference's `_default_hparams`
functions), and the numpy mirrors of the planner's verbose pictures.  No GPU."""
import glob
import json
import os
import sys
import textwrap

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import video_gcp_amd  # noqa: E402,F401
from video_gcp_amd import conf_loader as CL  # noqa: E402
from video_gcp_amd import dataset as DS  # noqa: E402
from video_gcp_amd import visualization as V  # noqa: E402
import topdown_fixture as TF  # noqa: E402

REFERENCE = "/root/reference"

CONTROL_CONF = textwrap.dedent('''
    import os.path
    from blox import AttrDict
    from gcp.planning.infra.agent.benchmarking_agent import BenchmarkAgent
    from gcp.planning.infra.envs.miniworld_env.multiroom3d.multiroom3d_env import TopdownMultiroom3dEnv
    from gcp.planning.planner_policy import {policy_cls}
    from gcp.planning.cem.sampler import {sampler}
    from gcp.planning.cem.cem_planner import HierarchicalImageCEMPlanner
    from gcp.planning.cem.cost_fcn import {cost}
    from experiments.prediction.base_configs import gcp_tree as base_conf

    agent = AttrDict(type=BenchmarkAgent, env=(TopdownMultiroom3dEnv, dict(n_rooms=25)), T=400, image_height=32, image_width=32,
                     start_goal_confs=os.environ['GCP_DATA_DIR'] + '/start_goal')
    h_config = AttrDict(base_conf.model_config)
    h_config.update(dict(state_dim=2, ngf=16, max_seq_len=200, hierarchy_levels=8, nz_mid_lstm=512, n_lstm_layers=3, nz_mid=128,
                         nz_enc=128, nz_vae=256, regress_length=True, attach_state_regressor=True, attach_inv_mdl=True,
                         inv_mdl_params=AttrDict(n_actions=2, use_convs=False, build_encoder=False), untied_layers=True,
                         decoder_distribution='discrete_logistic_mixture'))
    h_config.pop("add_weighted_pixel_copy")
    cem_params = AttrDict(prune_final=True, horizon=200, action_dim=256, verbose=True, n_level_hierarchy=8, sampler={sampler},
                          cost_fcn={cost}, cost_config=AttrDict(checkpt_path=os.environ['GCP_EXP_DIR'] + '/prediction/weights'),
                          {cem_extra})
    policy = AttrDict(type={policy_cls}, params=h_config, checkpt_path=cem_params.cost_config.checkpt_path,
                      cem_planner=HierarchicalImageCEMPlanner, cem_params=cem_params, replan_interval=agent.T + 2,
                      closed_loop_execution=True)
    config = AttrDict(current_dir=os.path.dirname(os.path.realpath(__file__)), start_index=0, end_index=99, agent=agent, policy=policy,
                      save_format=['raw'], data_save_dir=os.environ['GCP_EXP_DIR'] + '/control', split_train_val_test=False,
                      traj_per_file=1)
''')
ENV = dict(GCP_DATA_DIR="/nowhere/data", GCP_EXP_DIR="/nowhere/exp")
HIER = dict(policy_cls="ImageCEMPolicy", sampler="ImageHierarchicalTreeCEMSampler", cost="ImageLearnedCostEstimate",
            cem_extra="n_iters=3, batch_size=10, sampling_rates_per_layer=[10, 10]")
FLAT = dict(policy_cls="ImageCEMPolicy", sampler="SimpleTreeCEMSampler", cost="ImageWrappedLearnedCostFcn",
            cem_extra="n_iters=1, batch_size=5, elite_frac=1.0")


def _write(tmp_path, **kw):
    p = tmp_path / "mod_hyper.py"
    p.write_text(CONTROL_CONF.format(**kw))
    return str(p)


def test_hierarchical_conf(tmp_path):
    d = CL.planner_from_control_conf(CL.exec_control_conf(_write(tmp_path, **HIER), ENV))
    hp = d.hp
    assert (hp.img_sz, hp.max_seq_len, hp.hierarchy_levels, hp.batch_size) == (32, 200, 8, 1)
    assert (hp.nz_enc, hp.nz_mid, hp.nz_vae, hp.nz_mid_lstm, hp.n_lstm_layers, hp.ngf, hp.n_actions) == (128, 128, 256, 512, 3, 16, 2)
    assert hp.untied_layers and hp.attach_inv_mdl and hp.attach_state_regressor and hp.regress_length and hp.matching_type == "balanced"
    assert d.model_kind == "tree" and d.planner == "hierarchical" and d.cost == "ImageLearnedCostEstimate"
    assert d.planner_args == dict(n_level_hierarchy=8, sampling_rates_per_layer=[10, 10], n_ll_samples=5, action_dim=256, max_seq_len=200,
                                  clip_val=float("inf"))
    assert d.policy_args == dict(replan_interval=402, num_max_replans=10, closed_loop_execution=True)
    assert d.pairs == (0, 99) and d.verbose is True and d.horizon == 200
    assert d.weights["path"] == "/nowhere/exp/prediction/weights" and d.weights["file"] is None and d.weights["cost_path"] is None
    reasons = dict(k.split(":") for k in d.ignored)
    assert reasons["agent.env"] == "simulator" and "agent.type" in reasons and reasons["data_save_dir"] == "path"
    assert reasons["save_format"] == "saver" and reasons["cem_params.prune_final"] == "unread"
    assert reasons["cem_params.batch_size"] == "unread"              # the hierarchical sampler draws its own populations


def test_hierarchical_conf_errors(tmp_path, monkeypatch):
    path = _write(tmp_path, **HIER)
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    for missing in ENV:
        with pytest.raises(ValueError, match=missing):
            CL.exec_control_conf(path, {k: v for k, v in ENV.items() if k != missing})
    bad = _write(tmp_path, **dict(HIER, cem_extra="n_iters=2, batch_size=10, sampling_rates_per_layer=[10, 10]"))
    with pytest.raises(ValueError, match=r"n_iters.*len\(rates\) \+ 1"):
        CL.planner_from_control_conf(CL.exec_control_conf(bad, ENV))
    for cls in ("CEMPolicy", "BehavioralCloningPolicy"):
        with pytest.raises(ValueError, match=cls):
            CL.planner_from_control_conf(CL.exec_control_conf(_write(tmp_path, **dict(HIER, policy_cls=cls)), ENV))
    with pytest.raises(ValueError, match="MadeUpCost"):
        CL.planner_from_control_conf(CL.exec_control_conf(_write(tmp_path, **dict(HIER, cost="MadeUpCost")), ENV))
    with pytest.raises(ValueError, match="action_dim"):
        CL.planner_from_control_conf(CL.exec_control_conf(_write(tmp_path, **HIER), ENV), nz_vae=64)
    unknown = _write(tmp_path, **dict(HIER, cem_extra=HIER["cem_extra"] + ", made_up_switch=3"))
    with pytest.raises(ValueError, match="made_up_switch"):
        CL.planner_from_control_conf(CL.exec_control_conf(unknown, ENV))
    changes = _write(tmp_path, **dict(HIER, cem_extra=HIER["cem_extra"] + ", use_delta_state_actions=True"))
    with pytest.raises(ValueError, match="use_delta_state_actions"):
        CL.planner_from_control_conf(CL.exec_control_conf(changes, ENV))


def test_flat_conf(tmp_path):
    d = CL.planner_from_control_conf(CL.exec_control_conf(_write(tmp_path, **FLAT), ENV))
    assert d.planner == "flat" and d.sampler == "SimpleTreeCEMSampler" and d.cost == "ImageWrappedLearnedCostFcn"
    assert d.planner_args == dict(n_iters=1, batch_size=5, elite_frac=1.0, max_seq_len=200)
    assert d.sampler_args == dict(clip_val=float("inf"), n_steps=200, action_dim=256, initial_std=0.3, n_level_hierarchy=8)
    assert d.hp.hierarchy_levels == 8 and d.hp.max_seq_len == 200 and d.cost_args == {}


def test_environment_is_restored(tmp_path, monkeypatch):
    path = _write(tmp_path, **HIER)
    monkeypatch.setenv("GCP_EXP_DIR", "/kept")
    monkeypatch.delenv("GCP_DATA_DIR", raising=False)
    before = dict(os.environ)
    c = CL.exec_control_conf(path, ENV)
    assert dict(os.environ) == before
    assert c["data_save_dir"] == "/nowhere/exp/control"              # the given name won during the execution
    c = CL.exec_control_conf(path, dict(GCP_DATA_DIR="/d"))
    assert c["data_save_dir"] == "/kept/control" and dict(os.environ) == before       # the process's name is seen too
    with pytest.raises(ValueError, match="GCP_DATA_DIR"):
        CL.exec_control_conf(path, {})
    assert dict(os.environ) == before                                # also after a failure
    assert "blox" not in sys.modules and "experiments" not in sys.modules


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="the reference checkout is not on this machine")
def test_shipped_control_confs_load():
    files = sorted(glob.glob(os.path.join(REFERENCE, "experiments", "control", "*", "*", "mod_hyper.py")))
    assert len(files) == 4
    for f in files:
        d = CL.planner_from_control_conf(CL.exec_control_conf(f, ENV))
        rooms25, tree = "25room" in f, "gcp_tree" in f
        assert d.hp.max_seq_len == (200 if rooms25 else 100) and d.hp.hierarchy_levels == (8 if rooms25 else 7) and d.hp.img_sz == 32
        assert d.model_kind == "tree"                                # no model_cls: planner_policy.py:36 builds the tree model
        assert d.planner == ("hierarchical" if tree else "flat") and d.verbose and d.pairs == (0, 99)
        if tree:
            assert d.planner_args["sampling_rates_per_layer"] == [10, 10]
        else:
            assert (d.planner_args["n_iters"], d.planner_args["batch_size"], d.planner_args["elite_frac"]) == (1, 5, 1.0)


# what the four shipped prediction confs loaded to before the key table (values recorded from the loader as it was)
_PREDICTION = {
    "25room/gcp_tree": dict(hierarchy_levels=8, untied_layers=True, nz_mid_lstm=512, model="tree", metric="basic"),
    "25room/gcp_sequential": dict(hierarchy_levels=7, untied_layers=True, nz_mid_lstm=1024, model="sequential", metric="basic"),
    "9room/gcp_tree": dict(hierarchy_levels=7, untied_layers=True, nz_mid_lstm=512, model="tree", metric="basic"),
    "9room/gcp_sequential": dict(hierarchy_levels=7, untied_layers=True, nz_mid_lstm=512, model="sequential", metric="basic"),
}


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="the reference checkout is not on this machine")
def test_shipped_prediction_confs_load_as_before():
    """the loader as it was: every model_config key that is a GCPHParams field is taken, the rest is `ignored` -- restated here as the
    expectation for the table-driven one"""
    fields = set(CL.GCPHParams.__dataclass_fields__)
    for name in _PREDICTION:
        f = os.path.join(REFERENCE, "experiments", "prediction", name, "conf.py")
        c, mc = CL.exec_conf_py(f)
        hp, trainer, ignored = CL.hparams_from_conf(c, mc, max_seq_len=80, img_sz=64)
        popped = ("one_step_planner", "binding", "dense_rec_type", "add_weighted_pixel_copy", "inv_mdl_params", "cost_mdl_params")
        want = {k: v for k, v in mc.items() if k in fields and k not in popped}
        want.update(batch_size=int(c["batch_size"]), max_seq_len=80, img_sz=64)
        if "n_actions" in (mc.get("inv_mdl_params") or {}):
            want["n_actions"] = mc["inv_mdl_params"]["n_actions"]
        if want.get("hierarchy_levels") == 0:
            want.pop("hierarchy_levels")
        assert hp == CL.GCPHParams(**want), name
        assert ignored == [k for k in mc if k not in fields and k not in popped] + \
            [k for k in c if k not in CL._TRAINER_KEYS and k != "model"], name
        assert trainer == dict({k: c[k] for k in CL._TRAINER_KEYS if k in c}, model=trainer["model"])
        assert trainer["model"] == ("sequential" if "sequential" in name else "tree")


# ---- the key table ---------------------------------------------------------------------------------------------------------------------
with open(os.path.join(ROOT, "tests", "golden", "ref_hparam_defaults.json")) as _f:
    GOLDEN = json.load(_f)["groups"]
# the reference's tables -> the loader's groups (base_model.py's keys are part of every model's hyper-parameters)
GROUPS = {"model": "model", "base_model": "model", "inv_mdl": "inv_mdl", "cost_mdl": "cost_mdl", "trainer": "trainer", "policy": "policy",
          "cem": "cem"}


def _value(v):
    return float(v) if v in ("inf", "-inf") else v


def test_every_reference_key_is_in_exactly_one_class():
    assert set(GOLDEN) == set(GROUPS)
    n = 0
    for ref_group, group in GROUPS.items():
        for key, default in GOLDEN[ref_group].items():
            classes = CL.key_classes(group, key)
            assert len(classes) == 1, (ref_group, key, classes)
            n += 1
            if classes == ["unbuilt"]:                               # the table's default is the reference's
                assert CL._same(_value(default), CL.KEY_TABLE[group]["unbuilt"][key]), (ref_group, key, default)
    assert n > 200
    for group, t in CL.KEY_TABLE.items():                             # and no key of the loader's own is in two classes
        keys = [k for c in ("mapped", "checked", "inert", "unbuilt") for k in t[c]]
        assert len(keys) == len(set(keys)), group
    must_be_unbuilt = ["use_conv_lstm", "separate_cnn_start_goal_encoder", "states_inference", "act_cond_inference", "train_on_action_seqs",
                       "regress_index", "pixel_shift_decoder", "skip_from_parents", "matching_temp_tenthlife", "mask_inf_attention",
                       "one_hot_attn_time_cond", "learn_attn_temp", "n_conv_layers", "nz_vae2"]
    for k in must_be_unbuilt:
        assert CL.key_classes("model", k) == ["unbuilt"], k
    for k in ("logger", "dataset_name", "n_rooms"):
        assert CL.key_classes("trainer", k) == ["inert"], k
    for k in ("device", "dump_encodings", "log_states_2d", "log_cartgripper", "log_d2b_3x3maze"):
        assert CL.key_classes("model", k) == ["inert"], k


@pytest.mark.parametrize("key,value", [("use_conv_lstm", True), ("states_inference", True), ("mask_inf_attention", True),
                                       ("matching_temp_tenthlife", 5000)])
def test_unbuilt_keys_raise_off_their_default(key, value):
    base = dict(max_seq_len=12, img_sz=32)
    with pytest.raises(ValueError, match=key):
        CL.hparams_from_conf({}, dict(base, **{key: value}))
    default = GOLDEN["model"][key]
    hp, _, ignored = CL.hparams_from_conf({}, dict(base, **{key: default}))
    assert hp == CL.GCPHParams(**base) and key in ignored


def test_every_unbuilt_key_loads_at_the_reference_default_and_an_invented_key_raises():
    base = dict(max_seq_len=12, img_sz=32)
    for key, default in CL.KEY_TABLE["model"]["unbuilt"].items():
        hp, _, ignored = CL.hparams_from_conf({}, dict(base, **{key: default}))
        assert hp == CL.GCPHParams(**base) and ignored == [key]
    for key in CL.KEY_TABLE["model"]["inert"]:
        hp, _, ignored = CL.hparams_from_conf({}, dict(base, **{key: "anything"}))
        assert hp == CL.GCPHParams(**base) and ignored == [key]
    with pytest.raises(ValueError, match="invented_key"):
        CL.hparams_from_conf({}, dict(base, invented_key=1))
    with pytest.raises(ValueError, match="invented_trainer_key"):
        CL.hparams_from_conf(dict(invented_trainer_key=1), base)
    with pytest.raises(ValueError, match="invented_inv_key"):
        CL.hparams_from_conf({}, dict(base, inv_mdl_params=dict(n_actions=2, invented_inv_key=1)))
    with pytest.raises(ValueError, match="pred_states"):
        CL.hparams_from_conf({}, dict(base, inv_mdl_params=dict(n_actions=2, pred_states=True)))
    # restating a default is no error (the reference's own rule, base_model.py:27-32, is not copied)
    assert CL.hparams_from_conf({}, dict(base, nz_vae=256))[0].nz_vae == 256


# ---- the numpy mirrors of the verbose pictures --------------------------------------------------------------------------------------------
def test_overview_mirror_equals_the_reference_reshape():
    rng = np.random.RandomState(0)
    horizon, res = 6, 32
    elites = [rng.uniform(-1.3, 1.3, size=(n, 3, res, res)).astype(np.float32) for n in (3, 5)]
    # cem_planner.py:228-239, restated
    stack = []
    for plan in elites:
        time, c, h, w = plan.shape
        plan = np.clip((plan + 1) / 2, 0, 1.0)
        if time < horizon:
            plan = np.concatenate((plan, np.ones((horizon - time, c, h, w))))
        stack.append(plan)
    stack = np.array(stack)
    n_plans = stack.shape[0]
    log_img = stack.transpose(0, 2, 3, 1, 4).reshape(n_plans, c, h, horizon * w).transpose(1, 0, 2, 3).reshape(c, h * n_plans, horizon * w)
    want = V.to_uint8(log_img.transpose(1, 2, 0).astype(np.float32))
    got = V.plan_overview_numpy(elites, horizon)
    assert got.shape == (2 * res, horizon * res, 3) and got.dtype == np.uint8
    assert np.array_equal(got, want)
    assert (got[:res, 3 * res:] == 255).all() and (got[res:, 5 * res:] == 255).all()      # the padding is white
    assert not (got[:res, :3 * res] == 255).all()


def _assets(arrays):
    a = dict(background=arrays["background"], cw=int(arrays["crop_window"]), n_rooms=int(arrays["n_rooms"]),
             scale=int(arrays["render_scale"]), agent_stamp=arrays["agent_stamp"], goal_stamp=arrays["goal_stamp"],
             agent_color=arrays["agent_color"], goal_color=arrays["goal_color"])
    a["S"] = int(DS.topdown_table_size(a["n_rooms"]) * a["scale"])
    return a


def test_trajdist_mirror_equals_successive_single_renders():
    """logger.py:262-269: im = render(trajs[0]); for traj in trajs[1:]: im = render(traj, background=im)"""
    a = _assets(TF.make_assets(seed=5, n_rooms=9, scale=24, cw=4, k=5))
    S, cw = a["S"], a["cw"]
    rng = np.random.RandomState(1)
    trajs = [rng.uniform(-12, 12, size=(n, 2)).astype(np.float32) for n in (4, 1, 6, 3)]      # crossing lines, overlapping stamps
    got = V.render_trajectory_dist_numpy(a, trajs)
    canvas = None
    for t in trajs:
        b = dict(a)
        if canvas is not None:
            b["background"] = a["background"].copy()
            b["background"][cw:cw + S, cw:cw + S] = canvas
        canvas = V.render_trajectories_numpy(b, [dict(states=t[None], length=np.array([len(t)]), color=V.RED)])[0]
    assert np.array_equal(got, canvas)
    single = V.render_trajectories_numpy(a, [dict(states=trajs[0][None], length=np.array([4]), color=V.RED)])[0]
    assert not np.array_equal(got, single)                           # the later trajectories painted something
    # the order matters where they overlap: the reverse order is another picture
    assert not np.array_equal(got, V.render_trajectory_dist_numpy(a, trajs[::-1]))
