"""Generate the picture-log goldens by EXECUTING the reference's own logger and visualisation functions.

Run from the repo root:  python tests/golden/make_ref_image_log_goldens.py
Writes tests/golden/ref_image_log.npz: the inputs of a small hand-built tree and the f32 canvases the reference computes from them
(no reference source is copied).

Functions executed, from gcp/prediction/utils/logger.py and visualization.py:
    HierarchyLogger.log_hierarchy_image (logger.py:114-182), log_loss_gif (:236-253), log_dense_gif / log_rows_gif (:214-234),
    make_gif (visualization.py:485-497), plot_gt_matching_overview (:365-400, for 'match_dist' and 'gamma'), plot_val_tree (:327-362),
    plot_balanced_tree (:232-262), plot_greyscale_dist (:51-55); SubgoalTreeLayer.depth_first_iter / get_attr_df (tree_utils.py:79-92)
    and get_pad_mask (utils.py:30-50).

Stand-ins, all in memory, for what the reference imports and this machine lacks (the goldens inherit their trivial assumptions):
    blox        AttrDict; rmap over a dict's values; find_tensor = the first tensor; broadcast_final = trailing unit dimensions;
                batchwise_index = t[arange, idx]; ndim.torched as the identity decorator (draw_frame is never called, see below)
    tensorboardX.SummaryWriter   records what add_image / add_video receive (the videos are read back from it)
    cv2, torchvision             empty modules (action arrows and image grids are not on the executed path)
    gcp.prediction.utils.utils   only get_pad_mask, compiled from the reference file (its module imports cv2 / dload at the top)

The `done_mask` shim.  logger.py:144 draws a node only if `'done_mask' in segment`; SubgoalTreeLayer (tree_utils.py:9-100) has
__iter__ and no __contains__, and nothing in gcp/ sets done_mask, so as shipped the test iterates the layers, is never true, and the
tree rows stay empty.  Here SubgoalTreeLayer gets a __contains__ that answers true for 'done_mask' and a class attribute
done_mask = None, so that logger.py:145-154 itself runs: every node of every logged sample at its matched time step, the evident
intent and what video-gcp_amd/visualization.py builds.

draw_frame's colour border (visualization.py:189-207) is not built; the model output here carries neither 'gt_match_dists' nor
'existence_predictor', so plot_balanced_tree takes its own border-less branch (usage_prob None, :246-259).
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref_image_log.npz")
L, RES, T, B = 3, 8, 7, 4
N = 2 ** L - 1


class AttrDict(dict):
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


class Recorder:
    def __init__(self):
        self.images, self.videos = [], []

    def add_image(self, name, img, step):
        self.images.append((name, img))

    def add_video(self, name, vid, step, fps=4):
        self.videos.append((name, vid, fps))


def install_shims():
    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    def slice_tensor(t, start, step, dim):
        idx = [slice(None)] * t.dim()
        idx[dim] = slice(start, None, step)
        return t[tuple(idx)]

    def rmap(fn, x):
        return AttrDict({k: fn(v) for k, v in x.items()}) if isinstance(x, dict) else fn(x)

    def broadcast_final(t, ref):
        return t.view(*t.shape, *([1] * (ref.dim() - t.dim())))

    identity = lambda f: f
    ndim = types.SimpleNamespace(torched=identity, permute=None, copy=None)
    blox = mod("blox", AttrDict=AttrDict)
    blox.torch = mod("blox.torch")
    blox.torch.ops = mod("blox.torch.ops", slice_tensor=slice_tensor, reduce_dim=lambda t, dim: t)
    blox.torch.porch = mod("blox.torch.porch", cat=torch.cat)
    blox.basic_types = mod("blox.basic_types", map_dict=lambda fn, d: {k: fn(v) for k, v in d.items()},
                           listdict2dictlist=lambda l: {k: [d[k] for d in l] for k in l[0]})
    blox.tensor = mod("blox.tensor", ndim=ndim)
    blox.tensor.ops = mod("blox.tensor.ops", batch_apply=lambda *a, **k: None, make_recursive_list=lambda fn: fn, rmap=rmap,
                          broadcast_final=broadcast_final,
                          find_tensor=lambda d: next(v for v in d.values() if isinstance(v, torch.Tensor)),
                          batchwise_index=lambda t, idx: t[torch.arange(t.shape[0]), idx])
    mod("tensorboardX", SummaryWriter=Recorder)
    mod("cv2")
    mod("torchvision")
    import matplotlib
    matplotlib.use("Agg")
    # get_pad_mask alone (utils.py:30-50)
    src = open(os.path.join(REF, "gcp/prediction/utils/utils.py")).read()
    ns = {"torch": torch, "np": np, "partial": __import__("functools").partial}
    exec(compile(src[src.index("def get_pad_mask"):src.index("def datetime_str")], "ref_utils_get_pad_mask", "exec"), ns)
    for name in ("gcp", "gcp.prediction", "gcp.prediction.utils"):
        mod(name)
    mod("gcp.prediction.utils.utils", get_pad_mask=ns["get_pad_mask"])


def load(path, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, path))
    m = importlib.util.module_from_spec(spec)
    sys.modules[name] = m
    spec.loader.exec_module(m)
    return m


def df_index(level, j):
    return (2 * j + 1) * 2 ** (L - 1 - level) - 1


def main():
    np.int, np.float = int, float          # removed aliases the reference still uses (tree_utils.py:225, utils.py:48)
    install_shims()
    tu = load("gcp/prediction/utils/tree_utils.py", "gcp.prediction.utils.tree_utils")
    vis = load("gcp/prediction/utils/visualization.py", "gcp.prediction.utils.visualization")
    lg = load("gcp/prediction/utils/logger.py", "gcp.prediction.utils.logger")
    tu.SubgoalTreeLayer.done_mask = None
    tu.SubgoalTreeLayer.__contains__ = lambda self, key: key == "done_mask"
    vis.PARAMS.hp = AttrDict(use_convs=True, img_sz=RES)

    rng = np.random.RandomState(7)
    # random frames, a little outside [-1, 1] so that the uint8 clip has work to do; drawn from a palette of 256 random f32 values
    # (arbitrary mantissas for the (x + 1) / 2 rounding, and a file that compresses)
    palette = rng.uniform(-1.2, 1.2, size=256).astype(np.float32)
    f32 = lambda *s: palette[rng.randint(0, 256, size=s)]
    inp = dict(traj_seq=f32(B, T, 3, RES, RES), images_df=f32(B, N, 3, RES, RES), dense_rec=f32(B, T, 3, RES, RES),
               soft=f32(B, T, 3, RES, RES), pruned_padded=f32(B, T, 3, RES, RES))
    # matched time steps, depth-first.  Sample 0: the two nodes of level 1 (df 1 and 5) on step 2, and a leaf (df 0) on step 0;
    # sample 1: two leaves (df 2 and 4) on step 3; sample 2: the root on step 0
    inp["node_t"] = np.array([[0, 2, 1, 3, 4, 2, 6], [0, 1, 3, 2, 3, 4, 5], [1, 2, 3, 0, 4, 5, 6], [0, 1, 2, 3, 4, 5, 6]], np.int32)
    inp["end_ind"] = np.array([6, 4, 6, 5], np.int64)                      # below T - 1 for samples 1 and 3
    inp["pruned_len"] = np.array([7, 5, 6, 4], np.int32)
    g = rng.uniform(0, 1, size=(B, N, T)).astype(np.float32)
    inp["gamma_df"] = g / g.sum(-1, keepdims=True)
    m = rng.uniform(0, 1, size=(B, N, T)).astype(np.float32)
    inp["match_dist_df"] = m / m.sum(1, keepdims=True)
    t = {k: torch.tensor(v) for k, v in inp.items()}

    def make_tree(attentive):
        layers = []
        for level in range(L):
            ids = [df_index(level, j) for j in range(2 ** level)]
            sg = AttrDict(images=t["images_df"][:, ids], ind=t["node_t"][:, ids].float(), match_dist=t["match_dist_df"][:, ids])
            if attentive:
                sg["gamma"] = t["gamma_df"][:, ids]
            layer = tu.SubgoalTreeLayer()
            layer.subgoals, layer.depth = sg, L - level
            layers.append(layer)
        leaf = tu.SubgoalTreeLayer()
        leaf.depth = 0
        for a, b in zip(layers, layers[1:] + [leaf]):
            a.child_layer = b
        return layers[0]

    inputs = AttrDict(traj_seq=t["traj_seq"], traj_seq_images=t["traj_seq"], I_0_image=t["traj_seq"][:, 0], end_ind=t["end_ind"])
    out = {}

    def logger():
        return lg.HierarchyLogger("unused", AttrDict(), T, summary_writer=Recorder())

    # hierarchical_splits: plain (balanced, no matching) and full (attentive + dense rec + soft estimates)
    mo = AttrDict(tree=make_tree(False), end_ind=t["end_ind"])
    out["hs_plain"] = logger().log_hierarchy_image(mo, inputs, "hierarchical_splits", 0, "train").numpy()
    mo = AttrDict(tree=make_tree(True), end_ind=t["end_ind"], dense_rec=AttrDict(images=t["dense_rec"]), soft_matched_estimates=t["soft"])
    out["hs_full"] = logger().log_hierarchy_image(mo, inputs, "hierarchical_splits", 0, "train").numpy()
    # match_overview / attention_masks
    with vis.param(n_logged_samples=3):
        out["match_overview"] = vis.plot_gt_matching_overview(mo, inputs)
        out["attention_masks"] = vis.plot_gt_matching_overview(mo, inputs, plot_attr="gamma")
    # output_tree
    out["output_tree"] = vis.plot_val_tree(mo, inputs)
    # pruned_seq_gif: make_gif([pruned_prediction])
    pruned = [t["pruned_padded"][b, :int(inp["pruned_len"][b])] for b in range(B)]
    out["pruned_seq_gif"] = vis.make_gif([pruned])
    # gt_target_gif, train and val
    for phase in ("train", "val"):
        lo = logger()
        lo.log_loss_gif(t["soft"], t["traj_seq"], "gt_target_gif", 0, phase)
        (_, vid, fps), = lo._summ_writer.videos
        assert fps == 4
        out[f"gt_target_gif_{phase}"] = vid[0].numpy()
        # dense_rec gif of the sequential model
        lo = logger()
        lo.log_dense_gif(AttrDict(dense_rec=AttrDict(images=t["dense_rec"])), inputs, "dense_rec", 0, phase)
        (_, vid, fps), = lo._summ_writer.videos
        out[f"dense_rec_{phase}"] = vid[0].numpy()
    out = {"out_" + k: np.asarray(v, np.float32) for k, v in out.items()}
    for k, v in out.items():
        assert np.isfinite(v).all(), k
    out.update({"in_" + k: v for k, v in inp.items()})
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
