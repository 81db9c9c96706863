"""Key names and default values of the REFERENCE's hyper-parameter tables, produced by EXECUTING its own `_default_hparams`
functions (and `get_default_gcp_hyperparameters`) here.

Run from the repo root:  python tests/golden/make_ref_hparam_goldens.py <reference checkout>
Writes tests/golden/ref_hparam_defaults.json: {group: {key: default}} — names and values only, classes by name.

Functions executed (paths relative to the reference checkout):
    gcp/prediction/hyperparameters.py:4-150                          get_default_gcp_hyperparameters      -> "model"
    gcp/prediction/models/auxilliary_models/base_model.py:34-70      BaseModel._default_hparams           -> "base_model"
    gcp/prediction/models/auxilliary_models/inverse_mdl.py:32-73     InverseModel._default_hparams        -> "inv_mdl"
    gcp/prediction/models/auxilliary_models/cost_mdl.py:26-50        CostModel._default_hparams           -> "cost_mdl"
    gcp/prediction/training/gcp_builder.py:249-272                   GCPBuilder._default_hparams          -> "trainer"
    gcp/planning/planner_policy.py:69-86,136-145,194-202             ImageCEMPolicy._default_hparams      -> "policy"
    gcp/planning/cem/cem_planner.py:24-53,173-192                    HierarchicalImageCEMPlanner._default_hparams -> "cem"
The modules import the un-vendored `blox` package, TF-1 `HParams` and simulator packages at module level; an import hook fabricates
placeholder modules / classes for those names so that the files load.  Two placeholders are executed: `HParams` (a bag of
add_hparam'ed values) and `ParamDict` (a dict).  The methods are called on instances made without running any constructor.
"""
import importlib.abc
import importlib.machinery
import json
import os
import sys
import types

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref_hparam_defaults.json")


class _Meta(type):
    def __getattr__(cls, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return _Meta(name, (), {})

    def __call__(cls, *args, **kw):
        """used as a decorator (`@torched`, `@register(...)`) a placeholder hands the function back"""
        if len(args) == 1 and not kw and callable(args[0]):
            return args[0]
        return lambda f: f


class HParams:
    def __init__(self, **kw):
        self.__dict__["_v"] = dict(kw)

    def add_hparam(self, k, v):
        self._v[k] = v

    def __getattr__(self, k):
        try:
            return self.__dict__["_v"][k]
        except KeyError:
            raise AttributeError(k)

    def __setattr__(self, k, v):
        self._v[k] = v

    def values(self):
        return dict(self._v)


class AttrDict(dict):
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


class ParamDict(AttrDict):
    def overwrite(self, other):
        self.update(other)
        return self


class _Placeholder(types.ModuleType):
    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        real = {"AttrDict": AttrDict, "ParamDict": ParamDict, "HParams": HParams}.get(name)
        if real is not None:
            return real
        cls = _Meta(name, (), {})
        setattr(self, name, cls)
        return cls


class _Finder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    ALWAYS = ("blox", "tensorflow")        # un-vendored / TF-1 only: never the installed package

    def find_spec(self, fullname, path, target=None):
        """a placeholder for every top-level package the modules import that is not installed here"""
        root = fullname.split(".")[0]
        if root in self.ALWAYS or (root not in ("gcp", "experiments") and not _importable(root)):
            return importlib.machinery.ModuleSpec(fullname, self, is_package=True)
        return None

    def create_module(self, spec):
        return _Placeholder(spec.name)

    def exec_module(self, module):
        pass


def _importable(root):
    for f in sys.meta_path:
        if isinstance(f, _Finder):
            continue
        try:
            if f.find_spec(root, None) is not None:
                return True
        except Exception:
            pass
    return False


def plain(v):
    if isinstance(v, HParams):
        v = v.values()
    if isinstance(v, dict):
        return {k: plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [plain(x) for x in v]
    if isinstance(v, float) and v in (float("inf"), float("-inf")):
        return "inf" if v > 0 else "-inf"
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    return getattr(v, "__name__", repr(v))


def defaults_of(cls):
    return cls._default_hparams(object.__new__(cls))


def main():
    ref = os.path.abspath(sys.argv[1])
    import numpy, torch  # noqa: F401,E401  (loaded before the hook: their own optional imports must keep failing as they do)
    sys.meta_path.insert(0, _Finder())
    sys.path.insert(0, ref)
    from gcp.prediction import hyperparameters
    from gcp.prediction.models.auxilliary_models import base_model, inverse_mdl, cost_mdl
    from gcp.prediction.training import gcp_builder
    from gcp.planning import planner_policy
    from gcp.planning.cem import cem_planner
    out = {
        "model": hyperparameters.get_default_gcp_hyperparameters(),
        "base_model": defaults_of(base_model.BaseModel),
        "inv_mdl": defaults_of(inverse_mdl.InverseModel),
        "cost_mdl": defaults_of(cost_mdl.CostModel),
        "trainer": defaults_of(gcp_builder.GCPBuilder),
        "policy": defaults_of(planner_policy.ImageCEMPolicy),
        "cem": defaults_of(cem_planner.HierarchicalImageCEMPlanner),
    }
    with open(OUT, "w") as f:
        json.dump({"source": "the reference's _default_hparams functions (see the generator's docstring)",
                   "groups": {g: plain(v) for g, v in out.items()}}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", OUT, {g: len(plain(v)) for g, v in out.items()})


if __name__ == "__main__":
    main()
