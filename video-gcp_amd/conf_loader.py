"""Experiment configuration in the reference's own format.

The reference's trainer loads `<exp_dir>/conf.py` with `imp.load_source` and reads two module-level dicts, `configuration`
(trainer: batch_size, lr, num_epochs, dataset ...) and `model_config` (model hyper-parameters)
(/root/reference/gcp/prediction/training/gcp_builder.py:112-147; e.g. experiments/prediction/25room/gcp_tree/conf.py).  Those files
import `blox.AttrDict`, dataset / logger / cost-function classes and `experiments.prediction.base_configs.*` — none of which is
importable here — but only use them as VALUES of the two dicts.  `load_conf` therefore executes the file with

  * `blox.AttrDict` provided (a dict with attribute access),
  * `experiments.prediction.base_configs.{base_tree, gcp_tree, gcp_adaptive, gcp_sequential, vmpc}` provided with the same entries the
    reference's base configs hold (restated below as data: base_configs/*.py),
  * every other `blox.*` / `gcp.*` / `experiments.*` name resolved to an inert named placeholder,

and maps what it finds onto this build's `GCPHParams` / trainer settings.  Keys without a counterpart on the device path (loggers,
dataset classes, visualisation switches) are returned in `ignored` rather than silently dropped.  A `conf.json`
({"config": "c2", "overrides": {...}, "lr": ...}) is accepted as well."""
import glob
import importlib
import importlib.abc
import importlib.machinery
import json
import os
import sys
import types

from .hparams import GCPHParams, config as named_config


class AttrDict(dict):
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


class _Named(type):
    """placeholder class: `repr` is the dotted name it was imported under; any attribute is another placeholder"""

    def __getattr__(cls, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return _Named(f"{cls.__name__}.{name}", (), {})

    def __repr__(cls):
        return f"<ref {cls.__name__}>"


# experiments/prediction/base_configs/*.py of the reference, as data
_BASE_TREE = dict(one_step_planner="sh_pred", hierarchy_levels=7, binding="loss", seq_enc="conv", tree_lstm="split_linear",
                  lstm_init="mlp", add_weighted_pixel_copy=True, dense_rec_type="node_prob")
_BASE_CONFIGS = {
    "base_tree": (dict(model="TreeModel", logger="HierarchyLogger"), dict(_BASE_TREE)),
    "gcp_tree": (dict(model="TreeModel", logger="HierarchyLogger", metric_pruning_scheme="pruned_dtw"),
                 dict(_BASE_TREE, matching_type="balanced")),
    # (untied_layers: the file does not set it, so the reference's default holds, hyperparameters.py:117 — tied tree levels; stated here
    # because this build's dataclass default is the 25-room conf's True.  A conf on this base may set 'dtw_latent', adaptive.py:45-47)
    "gcp_adaptive": (dict(model="TreeModel", logger="HierarchyLogger"),
                     dict(_BASE_TREE, matching_type="dtw_image", learn_matching_temp=False, attentive_inference=True,
                          untied_layers=False)),
    "gcp_sequential": (dict(model="SequentialModel", logger="HierarchyLogger"),
                       dict(one_step_planner="continuous", dense_rec_type="svg", hierarchy_levels=0, add_weighted_pixel_copy=True)),
    # base_configs/vmpc.py:11-16: gcp_sequential made action-conditioned, deterministic and blind to the goal
    "vmpc": (dict(model="SequentialModel", logger="HierarchyLogger"),
             dict(one_step_planner="continuous", dense_rec_type="svg", hierarchy_levels=0, add_weighted_pixel_copy=True,
                  action_conditioned_pred=True, non_goal_conditioned=True, nz_vae=0, var_inf="deterministic")),
}


class _Module(types.ModuleType):
    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        if name == "AttrDict":
            return AttrDict
        if self.__name__ == "experiments.prediction.base_configs" and name in _BASE_CONFIGS:
            return importlib.import_module(f"{self.__name__}.{name}")     # `from ...base_configs import gcp_tree as base_conf`
        v = _Named(name, (), {})
        setattr(self, name, v)
        return v


class _Finder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    ROOTS = ("blox", "gcp", "experiments")

    def find_spec(self, fullname, path, target=None):
        if fullname.split(".")[0] in self.ROOTS:
            return importlib.machinery.ModuleSpec(fullname, self, is_package=True)
        return None

    def create_module(self, spec):
        m = _Module(spec.name)
        parts = spec.name.split(".")
        if parts[:3] == ["experiments", "prediction", "base_configs"] and len(parts) == 4 and parts[3] in _BASE_CONFIGS:
            c, mc = _BASE_CONFIGS[parts[3]]
            m.configuration, m.model_config = AttrDict(c), AttrDict(mc)
        return m

    def exec_module(self, module):
        pass


def exec_conf_py(path):
    """Run a reference-style conf.py; returns (configuration, model_config) as plain dicts."""
    ns = _exec_with_placeholders(path, "conf")
    if "configuration" not in ns or "model_config" not in ns:
        raise ValueError(f"{path}: a configuration file defines `configuration` and `model_config` (gcp_builder.py:136-143)")
    return dict(ns["configuration"]), dict(ns["model_config"])


def exec_dataset_spec(path):
    """Run a reference-style `<data_dir>/dataset_spec.py` (data_loader.py:100-102, gcp_builder.py:149-152) with the same
    placeholder imports as conf.py; returns its `dataset_spec` as a plain dict (a dataset class arrives as a named placeholder)."""
    ns = _exec_with_placeholders(path, "dataset_spec")
    if "dataset_spec" not in ns:
        raise ValueError(f"{path}: a dataset spec file defines `dataset_spec`")
    return dict(ns["dataset_spec"])


def _exec_with_placeholders(path, name):
    finder = _Finder()
    saved = {k: v for k, v in sys.modules.items() if k.split(".")[0] in _Finder.ROOTS}
    for k in saved:
        del sys.modules[k]
    sys.meta_path.insert(0, finder)
    try:
        ns = {"__file__": os.path.abspath(path), "__name__": name}
        with open(path) as f:
            exec(compile(f.read(), path, "exec"), ns)
    finally:
        sys.meta_path.remove(finder)
        for k in [k for k in sys.modules if k.split(".")[0] in _Finder.ROOTS]:
            del sys.modules[k]
        sys.modules.update(saved)
    return ns


# ---- the key table: every key of the reference's hyper-parameter tables is mapped, value-checked, inert or unbuilt ---------------------
# Groups follow the reference's `_default_hparams` functions (tests/golden/ref_hparam_defaults.json holds their keys and defaults):
#   model    hyperparameters.py:4-150 + base_model.py:34-64      (model_config, policy.params)
#   inv_mdl  inverse_mdl.py:32-73   cost_mdl  cost_mdl.py:26-50   (model_config's inv_mdl_params / cost_mdl_params)
#   trainer  gcp_builder.py:249-272                               (configuration)
#   policy   planner_policy.py:69-86,136-145,194-202   cem  cem_planner.py:24-53,173-192   (a control conf's policy / cem_params)
# Per group:  mapped   a GCPHParams field, or a key this loader translates;
#             checked  {key: allowed values}: settled by what this build implements;
#             inert    {key: reason}: cannot change what is computed; still reported in `ignored`;
#             unbuilt  {key: the reference's default}: any other value raises -- the feature is not built, and training or planning with a
#                      different model silently is worse than stopping.
# A key in none of the four raises as unknown.  (The reference's own "an override equal to the default raises" rule,
# base_model.py:27-32, is not copied: a conf may restate a default.)
INF = float("inf")
_LEARNED_COSTS = ("LearnedCostEstimate", "ImageLearnedCostEstimate", "ImageWrappedLearnedCostFcn")
_HAND_COSTS = ("EuclideanDistance", "EuclideanPathLength", "StepPathLength", "L2ImageCost")
_HIERARCHICAL_SAMPLERS = ("ImageHierarchicalTreeCEMSampler", "HierarchicalTreeCEMSampler")
_FLAT_SAMPLERS = ("SimpleTreeCEMSampler", "FlatCEMSampler", "PDDMSampler")
_PLANNER_CLASSES = (None, "HierarchicalImageCEMPlanner", "HierarchicalCEMPlanner", "ImageCEMPlanner", "CEMPlanner")
_FIXED = {"one_step_planner": ("sh_pred", "continuous"), "binding": ("loss",),
          "dense_rec_type": ("node_prob", "svg", "none", None)}
_MODEL_CHECKED = dict(_FIXED, tree_lstm=("split_linear", "linear", "sum", "", None), add_weighted_pixel_copy=(False,))
KEY_TABLE = {
    "model": dict(
        mapped=(set(GCPHParams.__dataclass_fields__) - set(_MODEL_CHECKED)) | {"inv_mdl_params", "cost_mdl_params"},
        checked=_MODEL_CHECKED,
        inert=dict(randomize_length="dataset", randomize_start="dataset", device="placement", dump_encodings="logging",
                   dump_encodings_inv_model="logging", log_states_2d="logging", log_cartgripper="logging", data_dir="logging",
                   log_d2b_3x3maze="logging", dataset_class="dataset", split="dataset", checkpt_path="resume"),
        unbuilt=dict(nz_vae2=256, n_conv_layers=None, action_activation=None, dense_action_rec_weight=1.0, pixel_shift_decoder=False,
                     skip_from_parents=False, regress_actions=False, learn_attn_temp=True, learn_beta=True, initial_sigma=1.0,
                     separate_cnn_start_goal_encoder=False, use_conv_lstm=False, one_hot_attn_time_cond=False,
                     matching_temp_tenthlife=-1, matching_temp_min=1e-3, n_top_bias_nodes=1, supervise_match_weight=0.0,
                     regress_index=False, act_cond_inference=False, train_on_action_seqs=False, states_inference=False,
                     mask_inf_attention=False, use_convs=True, use_batchnorm=True, normalization="batch",
                     predictor_normalization="group", filter_repeated_tail=False, rep_tail=False, standardize=None, subsampler=None,
                     subsample_args=None)),
    # the inverse model runs on the predictor's latents (base_gcp.py builds it with build_encoder=False, use_convs=False)
    "inv_mdl": dict(
        mapped={"n_actions", "temp_dist"},
        checked=dict(use_convs=(False,), build_encoder=(False,)),
        inert=dict(device="placement", log_topdown_maze="logging", randomize_length="dataset", dataset_class="dataset", split="dataset",
                   checkpt_path="resume", batch_size="parent", max_seq_len="parent", state_dim="parent", img_sz="parent",
                   input_nc="parent"),
        unbuilt=dict(ngf=4, nz_enc=128, nz_mid=128, n_processing_layers=3, enc_params_checkpoint=None, take_first_tstep=False,
                     use_states=False, aggregate_actions=False, pred_states=False, finetune_enc=False, add_lstm_state_enc=False,
                     train_full_seq=False, train_im0_enc=True, action_rec_weight=1.0, state_rec_weight=1.0, use_skips=False,
                     dense_rec_type=None, n_conv_layers=None, use_batchnorm=True, normalization="batch",
                     predictor_normalization="group", filter_repeated_tail=False, rep_tail=False, standardize=None, subsampler=None,
                     subsample_args=None)),
    "cost_mdl": dict(
        mapped=set(),
        checked=dict(use_path_dist_cost=(False,), cost_fcn=(None, "EuclideanPathLength"), use_convs=(False,)),
        inert=dict(device="placement", randomize_length="dataset", dataset_class="dataset", split="dataset", checkpt_path="weights",
                   load_epoch="weights", batch_size="parent", max_seq_len="parent", state_dim="parent", img_sz="parent",
                   input_nc="parent", n_actions="parent"),
        unbuilt=dict(nz_enc=128, nz_mid=128, n_processing_layers=3, use_skips=False, dense_rec_type=None, n_conv_layers=None,
                     use_batchnorm=True, normalization="batch", predictor_normalization="group", filter_repeated_tail=False,
                     rep_tail=False, standardize=None, subsampler=None, subsample_args=None)),
    "trainer": dict(
        mapped={"model", "batch_size", "lr", "num_epochs", "adam_beta", "epoch_cycles_train", "seed", "gradient_clip", "top_of_100_eval",
                "metric_pruning_scheme", "optimizer", "momentum"},
        checked={},
        inert=dict(logger="logging", dataset_name="dataset", exp_path="path", n_rooms="logging", data_dir="dataset",
                   randomize_length="dataset", randomize_start="dataset"),
        unbuilt={}),
    "policy": dict(
        mapped={"type", "params", "model_cls", "checkpt_path", "load_epoch", "cem_params", "replan_interval", "num_max_replans",
                "closed_loop_execution", "act_cond"},
        checked=dict(cem_planner=_PLANNER_CLASSES),
        inert=dict(logger="logging", verbose="logging", max_dump_rollouts="logging", ncam="cameras"),
        unbuilt={}),
    "cem": dict(
        mapped={"horizon", "action_dim", "n_iters", "batch_size", "elite_frac", "cost_fcn", "cost_config", "dense_cost",
                "final_step_cost_weight", "sampler", "sampler_clip_val", "initial_std", "verbose", "max_seq_len", "n_level_hierarchy",
                "sampling_rates_per_layer", "n_ll_samples", "use_inferred_actions"},
        checked={},
        # prune_final: set by every shipped control conf, read nowhere in the reference.  max_rollout_bs: how the reference chunks a
        # population; this build evaluates every candidate (planning.py, deviation D2)
        inert=dict(prune_final="unread", max_rollout_bs="chunking", dump_planning_data="logging"),
        unbuilt=dict(LL_cost_fcn=None, use_delta_state_actions=False)),
}
# trainer keys (gcp_builder.py:_default_hparams) that the device trainer reads
_TRAINER_KEYS = ("batch_size", "lr", "num_epochs", "adam_beta", "epoch_cycles_train", "seed", "gradient_clip", "top_of_100_eval",
                 "metric_pruning_scheme", "optimizer", "momentum")


def class_name(v):
    """a class in a conf arrives as a named placeholder (or, from a JSON fixture, as its name): the bare class name; None stays None"""
    if v is None or isinstance(v, (bool, int, float, dict, list, tuple)):
        return v
    name = v if isinstance(v, str) else getattr(v, "__name__", repr(v))
    return name.rsplit(".", 1)[-1]


def key_classes(group, key):
    """the classes of the group's table that hold `key`: exactly one for every key of the reference"""
    return [c for c in ("mapped", "checked", "inert", "unbuilt") if key in KEY_TABLE[group][c]]


def _same(v, default):
    """a conf's value equals the reference's default (classes by name; an empty dict / list equals any empty one; True is not 1)"""
    v = class_name(v)
    if isinstance(v, (dict, list, tuple)) or isinstance(default, (dict, list, tuple)):
        return v == default or (not v and not default)
    if isinstance(v, bool) != isinstance(default, bool):
        return False
    return v == default


def screen_keys(group, d, where):
    """Every key of dict `d` against the group's table.  Returns the keys that take no part (inert ones, unbuilt ones at the reference's
    default); raises ValueError for an unknown key, a checked key with a value that is not built, and an unbuilt key off its default."""
    t = KEY_TABLE[group]
    passed = []
    for k, v in d.items():
        if k in t["mapped"]:
            continue
        if k in t["checked"]:
            if class_name(v) not in t["checked"][k]:
                raise ValueError(f"{where}[{k!r}] = {v!r}: only {t['checked'][k]} is built")
        elif k in t["inert"]:
            passed.append(k)
        elif k in t["unbuilt"]:
            if not _same(v, t["unbuilt"][k]):
                raise ValueError(f"{where}[{k!r}] = {v!r}: not built (only the reference's default, {t['unbuilt'][k]!r}, is); "
                                 "a different model would be run silently otherwise")
            passed.append(k)
        else:
            raise ValueError(f"{where}[{k!r}]: unknown key (in none of the reference's hyper-parameter tables, and no field of this build)")
    return passed


def model_kind(configuration):
    """configuration['model'] (gcp_builder.py:75: the class the trainer instantiates) -> 'sequential' (SequentialModel, the flat
    VRNN baseline) or 'tree' (TreeModel).  The class arrives as a placeholder named like the reference's class, or as a string."""
    v = configuration.get("model", "TreeModel")
    name = v if isinstance(v, str) else getattr(v, "__name__", repr(v))
    return "sequential" if "sequential" in name.lower() else "tree"


def hparams_from_conf(configuration, model_config, **over):
    """(GCPHParams, trainer settings, ignored keys).  max_seq_len / img_sz come from the dataset spec in the reference
    (data_loader.py); here they are overrides or the c2 defaults (T=80, 64x64).  Every key goes through KEY_TABLE (above)."""
    fields = set(GCPHParams.__dataclass_fields__)
    kw, ignored = {}, []
    mc = dict(model_config)
    if (mc.get("tree_lstm", "split_linear") or "") not in ("split_linear", "linear", "sum", ""):      # tree_lstm.py:52-60; '' / None = the
        raise ValueError(f"model_config['tree_lstm'] = {mc['tree_lstm']!r}: split_linear, linear, sum and '' are built")   # non-LSTM predictor
    if mc.get("add_weighted_pixel_copy", False):
        # hyperparameters.py:54; base_configs/base_tree.py and gcp_sequential.py set it, every room conf pops it again
        # (25room/gcp_tree/conf.py:43).  A conf that keeps it asks for a decoder with a pixel-copy stream, which is not built: training
        # a different decoder silently is worse than stopping
        raise ValueError("model_config['add_weighted_pixel_copy'] = True: the weighted pixel-copy decoder stream is not built "
                         "(the 25-room / 9-room confs pop the key: `model_config.pop('add_weighted_pixel_copy')`)")
    if (mc.get("cost_mdl_params") or {}).get("use_path_dist_cost"):
        raise ValueError("cost_mdl_params.use_path_dist_cost: the fast path needs state sequences; image trajectories use the "
                         "generic cost (cost_mdl.py:81-117)")
    unused = set(screen_keys("model", mc, "model_config"))
    for k in list(_FIXED) + ["add_weighted_pixel_copy"]:
        mc.pop(k, None)
    inv = mc.pop("inv_mdl_params", None) or {}
    screen_keys("inv_mdl", inv, "model_config['inv_mdl_params']")
    if "n_actions" in inv:
        kw["n_actions"] = int(inv["n_actions"])
    if "temp_dist" in inv:
        kw["inv_mdl_temp_dist"] = int(inv["temp_dist"])
    screen_keys("cost_mdl", mc.pop("cost_mdl_params", None) or {}, "model_config['cost_mdl_params']")
    for k, v in mc.items():
        if k in fields and k not in unused:
            kw[k] = v
        else:
            ignored.append(k)
    if "batch_size" in configuration:
        kw["batch_size"] = int(configuration["batch_size"])
    kw.update(over)
    if "hierarchy_levels" in kw and "max_seq_len" in kw and 2 ** int(kw["hierarchy_levels"]) - 1 < int(kw["max_seq_len"]):
        kw.pop("hierarchy_levels")        # a tree too small for the sequence length: fall back to ceil(log2(T)) (train.py:80-81)
    if kw.get("hierarchy_levels", 1) == 0:
        kw.pop("hierarchy_levels")        # the flat model's base config (base_configs/gcp_sequential.py) has no tree
    hp = GCPHParams(**kw)
    screen_keys("trainer", configuration, "configuration")
    trainer = {k: configuration[k] for k in _TRAINER_KEYS if k in configuration}
    trainer["model"] = model_kind(configuration)
    ignored += [k for k in configuration if k not in _TRAINER_KEYS and k != "model"]
    return hp, trainer, ignored


def load_conf(exp_dir, default="c2", name=None, **over):
    """`<exp_dir>/*.py` (the reference's rule, gcp_builder.py:112-118: the one configuration file in the directory) or
    `<exp_dir>/conf.json`.  Returns (GCPHParams, trainer settings dict, ignored keys).  `name`: a named configuration given
    explicitly (the --config flag): it wins over conf.json's "config" entry; `default` is used only when neither names one.
    A reference-style conf.py carries no dataset spec: `max_seq_len` / `img_sz` not given as overrides fall back to the dataclass
    defaults and are reported among the ignored keys as "defaulted:<key>"."""
    if exp_dir and os.path.isdir(exp_dir):
        py = sorted(glob.glob(os.path.join(os.path.abspath(exp_dir), "*.py")))
        if len(py) > 1:
            raise ValueError(f"Multiple configuration files found at {exp_dir}!")
        if py:
            c, mc = exec_conf_py(py[0])
            hp, trainer, ignored = hparams_from_conf(c, mc, **over)
            # the reference takes these from the dataset spec (data_loader.py), which a conf.py does not hold
            ignored += [f"defaulted:{k}" for k in ("max_seq_len", "img_sz") if k not in over and k not in mc]
            return hp, trainer, ignored
        js = os.path.join(exp_dir, "conf.json")
        if os.path.exists(js):
            conf = json.load(open(js))
            ov = dict(conf.get("overrides", {}), **over)
            hp = named_config(name or conf.get("config", default), **ov)
            tr = {k: conf[k] for k in conf if k not in ("config", "overrides")}
            tr["model"] = model_kind(tr)
            return hp, tr, []
    return named_config(name or default, **over), {}, []


# ---- control configurations: the reference's run.py <experiments/control/*/mod_hyper.py> -----------------------------------------------
def exec_control_conf(path, environ=None):
    """Run a reference-style `mod_hyper.py` (gcp/planning/run.py loads it and reads `config`) under the placeholder imports of
    exec_conf_py; returns its `config` as plain dicts, classes as named placeholders.  The shipped files read
    os.environ['GCP_DATA_DIR'] / ['GCP_EXP_DIR'] while they execute: the names given in `environ` are visible to the conf during the
    execution only (the process environment is restored afterwards), and a name found in neither place raises ValueError."""
    saved = dict(os.environ)
    try:
        os.environ.update({k: str(v) for k, v in (environ or {}).items()})
        try:
            ns = _exec_with_placeholders(path, "mod_hyper")
        except KeyError as e:
            name = e.args[0] if e.args else None
            tb = e.__traceback__
            while tb.tb_next is not None:
                tb = tb.tb_next
            if isinstance(name, str) and tb.tb_frame.f_code.co_filename == os.__file__:          # raised by os.environ[name]
                raise ValueError(f"{path}: the configuration reads the environment variable {name}, which is not set "
                                 f"(give it through `environ`, or --data_dir / --exp_dir of the planner)") from None
            raise
    finally:
        for k in [k for k in os.environ if k not in saved]:
            del os.environ[k]
        os.environ.update(saved)
    if "config" not in ns:
        raise ValueError(f"{path}: a control configuration defines `config` (gcp/planning/run.py)")
    return _plain(ns["config"])


def _plain(v):
    if isinstance(v, dict):
        return {k: _plain(x) for k, x in v.items()}
    if isinstance(v, list):
        return [_plain(x) for x in v]
    if isinstance(v, tuple):
        return tuple(_plain(x) for x in v)
    return v


def _resolve_weights(path, epoch):
    """the weights file of a checkpoint directory (checkpoint_handler.py:31-42), None when it does not resolve"""
    from .checkpoint import get_resume_ckpt_file, NoCheckpointsException
    if not path or not os.path.isdir(path):
        return None
    try:
        f = get_resume_ckpt_file("latest" if epoch is None else epoch, path)
    except NoCheckpointsException:
        return None
    return f if os.path.isfile(f) else None


def planner_from_control_conf(config, **over):
    """A control conf's `config` (exec_control_conf) as a plain description of what to build:
        hp           GCPHParams of the planner's model (policy.params through hparams_from_conf; `over` overrides fields)
        model_kind   'tree' / 'sequential' (policy.model_cls, else the tree model: planner_policy.py:36)
        planner      'hierarchical' (planning.HierarchicalCEMPlanner) or 'flat' (planning.CEMPlanner), decided by cem_params.sampler
        planner_args keyword arguments of that planner; sampler / sampler_args (flat); cost / cost_args; verbose
        horizon      cem_params.horizon (default: max_seq_len); below max_seq_len the flat planner caps its rollouts to it
        act_cond     policy.act_cond: the samples are action sequences for the action-conditioned flat predictor (visual MPC)
        action_source  'inverse_model' (the plan's actions are the final rollout's inverse-model actions) or 'samples'
                     (cem_params.use_inferred_actions = False: the action plan is the best sample itself)
        policy_args  replan_interval, num_max_replans, closed_loop_execution of planning.ImageCEMPolicy
        weights      dict(path, epoch, file, cost_path, cost_file): `file` / `cost_file` are None where nothing resolves
        pairs        (start_index, end_index)
        ignored      ['<key>:<reason>'] of everything that takes no part
    Follows planner_policy.py:15-57,69-86,127-145,191-202 and cem_planner.py:24-53,166-218."""
    ignored = []
    for k, v in config.items():
        if k not in ("agent", "policy", "start_index", "end_index"):
            ignored.append(f"{k}:{'path' if k in ('current_dir', 'data_save_dir') else 'saver'}")
    agent, policy = dict(config.get("agent") or {}), dict(config.get("policy") or {})
    ptype = class_name(policy.get("type"))
    if ptype != "ImageCEMPolicy":
        raise ValueError(f"policy.type = {ptype}: only ImageCEMPolicy is built (the state-space CEMPolicy and the BC policy are not)")
    ignored += [f"policy.{k}:{KEY_TABLE['policy']['inert'].get(k, 'default')}" for k in screen_keys("policy", policy, "policy")]
    for k in agent:
        if k not in ("T", "image_height", "image_width"):
            ignored.append(f"agent.{k}:{'simulator' if k == 'env' else 'infrastructure'}")

    # ---- the model (planner_policy.py:30-38) ----
    params = dict(policy.get("params") or {})
    H, W = agent.get("image_height"), agent.get("image_width")
    if H is None or H != W:
        raise ValueError(f"agent.image_height = {H}, agent.image_width = {W}: the planner's model takes square images")
    if "img_sz" in params and params["img_sz"] != W:
        raise ValueError(f"policy.params['img_sz'] = {params['img_sz']} but agent.image_width = {W} (planner_policy.py:38)")
    params["img_sz"] = int(W)
    if "max_seq_len" not in params:
        if "T" not in agent:
            raise ValueError("max_seq_len is neither in policy.params nor given as agent.T (planner_policy.py:32-33)")
        params["max_seq_len"] = int(agent["T"])
    kind = model_kind({"model": policy["model_cls"]} if policy.get("model_cls") is not None else {})
    hp, _, ign = hparams_from_conf({"batch_size": 1}, params, **over)              # planner_policy.py:30: batch_size 1
    ignored += [f"policy.params.{k}:{KEY_TABLE['model']['inert'].get(k, 'default')}" for k in ign if k != "batch_size"]

    # ---- the planner (cem_planner.py:24-53,166-218) ----
    cem = dict(policy.get("cem_params") or {})
    unused = screen_keys("cem", cem, "cem_params")
    ignored += [f"cem_params.{k}:{KEY_TABLE['cem']['inert'].get(k, 'default')}" for k in unused]
    planner_cls = class_name(policy.get("cem_planner"))
    sampler = class_name(cem.get("sampler", "HierarchicalTreeCEMSampler"))
    # what the planner samples (planner_policy.py:231, cem_simulator.py:99-104): the model's latents, or, under act_cond, action sequences
    # for the action-conditioned flat predictor
    act_cond = bool(policy.get("act_cond", False))
    flat_only = tuple(s_ for s_ in _FLAT_SAMPLERS if s_ != "SimpleTreeCEMSampler")
    if act_cond:
        if kind != "sequential":
            raise ValueError(f"policy.act_cond = True with policy.model_cls = {class_name(policy.get('model_cls'))}: action sequences are "
                             "rolled out by the flat predictor, model_cls = SequentialModel (cem_simulator.py:99-104)")
        if not hp.action_conditioned_pred:
            raise ValueError("policy.act_cond = True but policy.params has action_conditioned_pred = False: the predictor takes no actions "
                             "(base_configs/vmpc.py sets it)")
        if sampler not in flat_only:
            raise ValueError(f"cem_params.sampler = {sampler} with policy.act_cond: action sequences are drawn by a flat sampler {flat_only}")
        if cem.get("action_dim") != hp.n_actions:
            raise ValueError(f"cem_params.action_dim = {cem.get('action_dim')}: under policy.act_cond the planner samples the model's "
                             f"actions, n_actions = {hp.n_actions}")
    else:
        if kind == "sequential" and hp.action_conditioned_pred:
            raise ValueError("policy.act_cond = False but policy.params has action_conditioned_pred = True: the predictor needs the "
                             "planner's samples as actions (set act_cond)")
        if kind == "sequential" and sampler not in flat_only:
            raise ValueError(f"cem_params.sampler = {sampler} with policy.model_cls = SequentialModel: the flat predictor has no tree; its "
                             f"latents are drawn by a flat sampler {flat_only}")
        if cem.get("action_dim") != hp.nz_vae:
            raise ValueError(f"cem_params.action_dim = {cem.get('action_dim')}: the planner samples the model's latents, nz_vae = {hp.nz_vae}")
    use_inferred = bool(cem.get("use_inferred_actions", True))
    if not use_inferred and not act_cond:
        raise ValueError("cem_params.use_inferred_actions = False without policy.act_cond: the best sample is a latent sequence, not an "
                         "action plan (cem_planner.py:143-149)")
    closed_loop = bool(policy.get("closed_loop_execution", False))
    if closed_loop and not hp.attach_inv_mdl:
        raise ValueError("policy.closed_loop_execution = True but policy.params has attach_inv_mdl = False: closed-loop execution infers "
                         "every action with the inverse model (planner_policy.py:222-227)")
    if cem.get("max_seq_len") not in (None, hp.max_seq_len):        # planner_policy.py:132 overwrites it with the model's
        raise ValueError(f"cem_params.max_seq_len = {cem['max_seq_len']}: the policy sets it to the model's, {hp.max_seq_len}")
    horizon = cem.get("horizon")
    if horizon is not None and horizon < hp.max_seq_len and sampler in _HIERARCHICAL_SAMPLERS:
        raise ValueError(f"cem_params.horizon = {horizon} < max_seq_len = {hp.max_seq_len}: the hierarchical planner optimises whole "
                         "trees and does not cap them to a horizon (cem_planner.py:151-155 is built for the flat planner)")
    if horizon is not None and horizon < 1:
        raise ValueError(f"cem_params.horizon = {horizon}: a plan has at least one step")
    cost = class_name(cem.get("cost_fcn", "LearnedCostEstimate"))
    if cost not in _LEARNED_COSTS + _HAND_COSTS:
        raise ValueError(f"cem_params.cost_fcn = {cost}: no counterpart in planning.py ({_LEARNED_COSTS + _HAND_COSTS})")
    learned = cost in _LEARNED_COSTS
    n_iters = cem.get("n_iters", 1)
    clip = cem.get("sampler_clip_val", INF)
    levels = cem.get("n_level_hierarchy")
    if sampler in _HIERARCHICAL_SAMPLERS + ("SimpleTreeCEMSampler",):
        if levels is None:
            raise ValueError(f"cem_params.sampler = {sampler} needs cem_params.n_level_hierarchy")
        if levels != hp.hierarchy_levels:
            raise ValueError(f"cem_params.n_level_hierarchy = {levels} but the model's tree has {hp.hierarchy_levels} levels")
    if sampler in _HIERARCHICAL_SAMPLERS:
        if planner_cls not in (None, "HierarchicalImageCEMPlanner", "HierarchicalCEMPlanner"):
            raise ValueError(f"policy.cem_planner = {planner_cls} cannot drive the hierarchical sampler {sampler} (cem_planner.py:109-113)")
        rates = cem.get("sampling_rates_per_layer")
        if rates is None:
            raise ValueError("cem_params.sampling_rates_per_layer is needed by the hierarchical sampler")
        rates = [int(r) for r in rates]
        if n_iters != len(rates) + 1:                                # cem_planner.py:170-171
            raise ValueError(f"cem_params.n_iters = {n_iters} but sampling_rates_per_layer = {rates}: "
                             f"n_iters == len(rates) + 1 = {len(rates) + 1} (cem_planner.py:170-171)")
        if not learned:
            raise ValueError(f"cem_params.cost_fcn = {cost}: the hierarchical planner scores subgoals with a learned cost")
        for k in ("batch_size", "elite_frac", "initial_std", "dense_cost", "final_step_cost_weight"):
            if k in cem:
                ignored.append(f"cem_params.{k}:unread")         # the hierarchical sampler draws its own populations (sampler.py:101-103)
        planner = "hierarchical"
        planner_args = dict(n_level_hierarchy=int(levels), sampling_rates_per_layer=rates, n_ll_samples=int(cem.get("n_ll_samples", 5)),
                            action_dim=hp.nz_vae, max_seq_len=hp.max_seq_len, clip_val=clip)
        sampler_args = {}
    elif sampler in _FLAT_SAMPLERS:
        # a hierarchical planner class given a flat sampler runs the flat loop (cem_planner.py:211-214)
        for k in ("sampling_rates_per_layer", "n_ll_samples"):
            if k in cem:
                ignored.append(f"cem_params.{k}:unread")
        planner = "flat"
        planner_args = dict(n_iters=int(n_iters), batch_size=int(cem.get("batch_size", 64)), elite_frac=float(cem.get("elite_frac", 0.1)),
                            max_seq_len=hp.max_seq_len)
        # the flat predictor takes one latent / action per predicted frame: sample t leads from frame t to frame t + 1 (sequential.py:50).
        # The reference draws max_seq_len steps (cem_planner.py:109-113) and its model never reads the last one
        sampler_args = dict(clip_val=clip, n_steps=hp.max_seq_len - 1 if kind == "sequential" else hp.max_seq_len,
                            action_dim=hp.n_actions if act_cond else hp.nz_vae, initial_std=float(cem.get("initial_std", 3e-1)))
        if sampler == "SimpleTreeCEMSampler":
            sampler_args["n_level_hierarchy"] = int(levels)
    else:
        raise ValueError(f"cem_params.sampler = {sampler}: no counterpart in planning.py ({_HIERARCHICAL_SAMPLERS + _FLAT_SAMPLERS})")
    cost_args = {} if learned else dict(dense_cost=bool(cem.get("dense_cost", False)),
                                        final_step_weight=float(cem.get("final_step_cost_weight", 1.0)))

    # ---- weights (planner_policy.py:48-50; the cost model's own checkpoint: cost_mdl.py:123-136) ----
    cost_config = dict(cem.get("cost_config") or {})
    ckpt, epoch = policy.get("checkpt_path"), policy.get("load_epoch")
    cost_ckpt = cost_config.get("checkpt_path")
    for k in cost_config:
        if k not in ("checkpt_path", "load_epoch"):
            screen_keys("cost_mdl", {k: cost_config[k]}, "cem_params.cost_config")
    other = bool(cost_ckpt) and bool(ckpt) and os.path.abspath(cost_ckpt) != os.path.abspath(ckpt)
    weights = dict(path=ckpt, epoch=epoch, file=_resolve_weights(ckpt, epoch), cost_path=cost_ckpt if other else None,
                   cost_file=_resolve_weights(cost_ckpt, cost_config.get("load_epoch")) if other else None)
    if not ckpt and cost_ckpt:
        weights.update(path=cost_ckpt, file=_resolve_weights(cost_ckpt, cost_config.get("load_epoch")))
    policy_args = dict(replan_interval=int(policy.get("replan_interval", 1)), num_max_replans=int(policy.get("num_max_replans", 10)),
                       closed_loop_execution=closed_loop)
    return AttrDict(hp=hp, model_kind=kind, planner=planner, planner_args=planner_args, sampler=sampler, sampler_args=sampler_args,
                    cost=cost, cost_args=cost_args, verbose=bool(cem.get("verbose", False)), act_cond=act_cond,
                    action_source="inverse_model" if use_inferred else "samples",
                    horizon=int(horizon) if horizon is not None else hp.max_seq_len, policy_args=policy_args, weights=weights,
                    pairs=(config.get("start_index"), config.get("end_index")), ignored=ignored)


def build_policy(description, device, weights=None, seed=0, random_weights=False, reference_rng=False, verbose=None, use_ema=False):
    """(model, planner, policy) of a planner_from_control_conf description on `device`: the planning.* objects a user who owns an
    environment loop drives through `policy.act(t=..., images=..., goal_image=...)`.
    The model is GCPTreeModel, or GCPSequentialModel for policy.model_cls = SequentialModel: then the simulator is
    ActCondGCPImageSimulator under act_cond (visual MPC) and GCPImageSimulator without drawn lengths otherwise (CEM in its latents).
    weights: a checkpoint file instead of the conf's; random_weights: run on the seeded initialisation when no checkpoint resolves
    (otherwise that raises); seed: of the initialisation, and seed + 1 of the planner's draws; reference_rng: the hierarchical
    planner replays the reference's np.random sequence; verbose: keep the per-iteration elites (default: the conf's `verbose`);
    use_ema: load the checkpoints' averaged weights (checkpoint.load_weights(use_ema=True)), the cost model's own checkpoint included --
    a checkpoint without an average, or no checkpoint at all, raises."""
    from . import planning as P
    from .checkpoint import load_weights
    from .model import GCPTreeModel
    from .params import init_params
    d = description
    hp = d.hp
    if d.model_kind == "sequential":                                 # policy.model_cls = SequentialModel (planner_policy.py:36)
        from .params import init_params_sequential
        from .sequential import GCPSequentialModel
        model = GCPSequentialModel(hp, params=init_params_sequential(hp, seed=seed), device=device)
    else:
        model = GCPTreeModel(hp, params=init_params(hp, seed=seed), device=device)
    main = weights or d.weights["file"]
    if use_ema and not main:
        raise ValueError("use_ema needs a checkpoint: averaged weights exist only in one")
    if main:
        load_weights(main, model, use_ema=bool(use_ema))
        if d.weights["cost_path"] and not weights:
            if not d.weights["cost_file"]:
                raise ValueError(f"no checkpoint of the cost model at cost_config.checkpt_path = {d.weights['cost_path']}")
            load_weights(d.weights["cost_file"], model, submodule_name="cost_mdl", use_ema=bool(use_ema))
    elif not random_weights:
        raise ValueError(f"no checkpoint at policy.checkpt_path = {d.weights['path']!r} (load_epoch = {d.weights['epoch'] or 'latest'}): "
                         "give a weights file, or ask for random weights")
    model.eval()                                                     # planner_policy.py:51
    if d.get("act_cond"):                                            # planner_policy.py:231
        sim = P.ActCondGCPImageSimulator(model)
    else:                                                            # (the flat predictor has no length predictor)
        sim = P.GCPImageSimulator(model, pred_length=d.model_kind != "sequential")
    cost = P.LearnedCostEstimate(model) if d.cost in _LEARNED_COSTS else getattr(P, d.cost)(d.cost_args["dense_cost"],
                                                                                             d.cost_args["final_step_weight"])
    verbose = d.verbose if verbose is None else bool(verbose)
    if d.planner == "hierarchical":
        planner = P.HierarchicalCEMPlanner(sim, cost, fast_draws=not reference_rng, seed=seed + 1, verbose=verbose, **d.planner_args)
    else:
        a = dict(d.sampler_args)
        sampler = getattr(P, d.sampler)(a.pop("clip_val"), a.pop("n_steps"), a.pop("action_dim"), a.pop("initial_std"), device=device,
                                        seed=seed + 1, **a)
        planner = P.CEMPlanner(sim, cost, sampler, verbose=verbose, horizon=d.horizon if d.horizon < hp.max_seq_len else None,
                               use_inferred_actions=d.get("action_source", "inverse_model") != "samples", **d.planner_args)
    return model, planner, P.ImageCEMPolicy(model, planner, **d.policy_args)


# ---- the environment of a control configuration (video-gcp_amd/control.py) -------------------------------------------------------------
# Multiroom3dEnv._default_hparams (multiroom3d_env.py:59-71) and TopdownMultiroom3dEnv's crop_window, with KEY_TABLE's discipline:
#   mapped   a NavEnvBatch parameter;  inert   cannot change what the batched environment computes;  unbuilt  {key: the reference's
#   default}: any other value raises.  A key in none of the three raises as unknown.
ENV_KEY_TABLE = {
    "mapped": {"n_rooms": 9, "crop_window": None},
    "inert": {"heading_smoothing": "the heading is the direction of the step taken, unsmoothed (as the generator records it)",
              "obs_height": "no first-person camera: the observation is the top-down frame",
              "obs_width": "no first-person camera: the observation is the top-down frame"},
    "unbuilt": {"init_pos": None, "goal_pos": None},
}
DEFAULT_CROP_WINDOW = 40      # what the shipped confs and the data collection use (nav_gen.experiment_settings)


def environment_from_control_conf(config):
    """A control conf's `config` (exec_control_conf) -> the batched environment's settings: n_rooms, crop_window, T (agent.T), img_sz
    (agent.image_height == agent.image_width) and `ignored`, ['<key>:<reason>'] of the environment keys that take no part.  Reads
    agent.env = (TopdownMultiroom3dEnv, env_params); any other environment class, an unknown key, and init_pos / goal_pos other than
    None raise.  planner_from_control_conf is not touched: it goes on listing agent.env as the simulator it does not build."""
    agent = dict(config.get("agent") or {})
    env = agent.get("env")
    if not isinstance(env, (list, tuple)) or len(env) != 2 or not isinstance(env[1], dict):
        raise ValueError(f"agent.env = {env!r}: expected (TopdownMultiroom3dEnv, env_params)")
    cls = class_name(env[0])
    if cls != "TopdownMultiroom3dEnv":
        raise ValueError(f"agent.env names {cls}: only TopdownMultiroom3dEnv is built (the observation is the cropped top-down frame)")
    out, ignored = dict(ENV_KEY_TABLE["mapped"]), []
    for k, v in env[1].items():
        if k in ENV_KEY_TABLE["mapped"]:
            out[k] = v
        elif k in ENV_KEY_TABLE["unbuilt"]:
            if v is not ENV_KEY_TABLE["unbuilt"][k]:
                raise ValueError(f"agent.env[{k!r}] = {v!r}: not built (only the reference's default, None, is): the tasks give start and goal")
            ignored.append(f"agent.env.{k}:default")
        elif k in ENV_KEY_TABLE["inert"]:
            ignored.append(f"agent.env.{k}:{ENV_KEY_TABLE['inert'][k]}")
        else:
            raise ValueError(f"agent.env: unknown TopdownMultiroom3dEnv parameter {k!r}")
    H, W = agent.get("image_height"), agent.get("image_width")
    if H is None or H != W:
        raise ValueError(f"agent.image_height = {H}, agent.image_width = {W}: the observation is a square frame")
    if "T" not in agent:
        raise ValueError("agent.T is missing: the number of steps of an episode (GeneralAgent.rollout)")
    crop = out["crop_window"]
    return AttrDict(n_rooms=int(out["n_rooms"]), crop_window=int(crop) if crop else DEFAULT_CROP_WINDOW, T=int(agent["T"]), img_sz=int(W),
                    ignored=ignored)
