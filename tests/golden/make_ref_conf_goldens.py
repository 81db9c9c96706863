"""Settings fixture from the REFERENCE's 25-room gcp_tree experiment: the two dicts its
experiments/prediction/25room/gcp_tree/conf.py defines (`configuration`, `model_config`), read by executing that file with
video_gcp_amd.conf_loader.exec_conf_py (the loader's stand-ins for blox / gcp / experiments.prediction.base_configs).

Run from the repo root:  python tests/golden/make_ref_conf_goldens.py <reference checkout>
Writes tests/golden/ref_25room_gcp_tree_conf.json (settings only).  Values that are classes in the conf (the cost function) are
recorded by name; nested AttrDicts as plain objects.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from video_gcp_amd import conf_loader as CL  # noqa: E402

CONF = os.path.join("experiments", "prediction", "25room", "gcp_tree", "conf.py")
OUT = os.path.join(HERE, "ref_25room_gcp_tree_conf.json")


def plain(v):
    if isinstance(v, dict):
        return {k: plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [plain(x) for x in v]
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    return getattr(v, "__name__", repr(v))


def main():
    ref = sys.argv[1]
    configuration, model_config = CL.exec_conf_py(os.path.join(ref, CONF))
    with open(OUT, "w") as f:
        json.dump({"source": CONF, "configuration": plain(configuration), "model_config": plain(model_config)}, f, indent=1,
                  sort_keys=True)
        f.write("\n")
    print("wrote", OUT)


if __name__ == "__main__":
    main()
