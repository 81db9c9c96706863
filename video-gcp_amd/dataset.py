"""Recorded video datasets and the host-fed loader.

Reader: the reference's VarLenVideoDataset family (gcp/datasets/data_loader.py:23-290) over the same group layout,
stored as `.npz` instead of HDF5: one file holds `traj_per_file` and, per trajectory i, `traj{i}/images` (uint8 [T_raw, H, W, 3], or
[T_raw, n_cam, H, W, 3] of which camera 0 is used), `traj{i}/states`, `traj{i}/actions` and `traj{i}/pad_mask`.  The directory
rules are the reference's: FolderSplitVarLenVideoDataset reads `<data_dir>/hdf5/<phase>/*`, GlobalSplitVarLenVideoDataset walks the
tree (sorted here: the reference's order follows the file system's listing) and splits by `dataset_spec['split']`; both shuffle the
file list with `random.Random(2)`.  `<data_dir>/dataset_spec.py` is executed with conf_loader's placeholder imports.

Per item the host makes the reference's draws, in the reference's order and from a numpy RandomState (same generator as the
reference's global np.random): end_ind from pad_mask, randomize_start, the random offset of the train phase, _maybe_pad, actions[:-1],
randomize_length (data_loader.py:131-211).  It does not build f32 images: it packs the raw uint8 window raw[offset : offset + T] and a
few integers per sequence (n_frames, chop, zero_from, end_ind); csrc/batch_assemble.hip turns them into the model's f32 inputs on
the device, in place in `model.input_buffer(...)` (the zero-copy hand-over of replay.py).  `assemble_numpy` is the same assembly in
numpy, bit for bit (tests, and the device-fed comparison of tools/host_fed_loop.py).

Resizing (data_loader.py:213-220, `preprocess_images` -> `resize_video(images, (img_sz, img_sz))`): opt-in, `VideoDataset(...,
resize=True)` / `train.py --resize_frames 1`.  Frames stored at H_s x W_s != img_sz are then uploaded at their stored size and resized
inside the batch assembly (gcpx_resize_assemble_batch), after pad / window / chop / zero and before the conversion, as the reference
orders it.  blox.vis.resize_video is absent from the reference tree; that it is torchvision's `Resize` on a PIL image, i.e. Pillow's
8-bit bilinear `Image.resize`, is inferred from data_loader.py:9,124.  That resampler is integer arithmetic over coefficient tables
that depend on the sizes alone: `resize_coeffs` builds them in float64 as Pillow's Resample.c does, `resize_frames_numpy` is the
integer restatement (bit-identical to Pillow on tests/golden/pil_resize.npz) and the kernel does the same integer arithmetic from the
uploaded tables.  Pillow itself is not imported anywhere in the product.  Without the option a size mismatch raises, as before.

Top-down rendering (data_loader.py:299-319, multiroom3d_env.py:185-219): the nav datasets (`dataset_class` Nav9Rooms, Nav25Rooms or
MazeTopRenderedGlobalSplitVarLenVideoDataset; GlobalSplit file rules) do not train on recorded frames.  Every frame t <= end_ind is a crop
of 2cw x 2cw pixels of a static picture of the maze around the agent's state, with a dot on the agent and one on the goal (the state at
end_ind), resized to img_sz; later frames are zero.  The picture and the dot's shape are made by OpenCV from the dataset's textures in
the reference; both are constant for a dataset and enter as data, `<data_dir>/topdown_assets.npz` (INTEGRATION.md has the recipe).  From
those arrays on the renderer is integer work: `topdown_pixels` is the reference's float32 state -> pixel arithmetic, `render_topdown_numpy`
the crop and the two dots.  Recorded images are neither read nor uploaded: an item carries the agent's pixel per window frame and the
goal's pixel, and gcpx_topdown_assemble_batch (csrc/batch_assemble.hip) renders, resizes and converts in the launch that writes the
model's inputs.  The model gets states[..., :2] (MazeGlobalSplit..., data_loader.py:292-296).

Keeping a whole split on the device and assembling batches from it there, with the same draws and the same bits
(`train.py --device_dataset 1`), is dataset_resident.py.

Not here: reading `.h5` (h5py), building the top-down picture from textures (nav_gen.py writes an untextured one with a whole nav
dataset: `python -m video_gcp_amd.gen_nav`), filters other than bilinear.
"""
import glob
import math
import os
import random
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import runtime as rt

# data_loader.py:222 `images.astype(np.float32) / 255 * 2 - 1` as a table: the kernel's values are these, whatever its build flags
LUT = np.arange(256, dtype=np.uint8).astype(np.float32) / 255 * 2 - 1

_CLASSES = ("FolderSplitVarLenVideoDataset", "GlobalSplitVarLenVideoDataset")
# datasets whose frames are rendered top-down from the states (gcp/datasets/configs/nav_9rooms.py, nav_25rooms.py)
_TOPDOWN_CLASSES = ("MazeTopRenderedGlobalSplitVarLenVideoDataset", "Nav9Rooms", "Nav25Rooms")
TOPDOWN_ASSETS = "topdown_assets.npz"
N_INFO = 8          # int32 per sequence read by gcpx_assemble_batch
PRECISION_BITS = 22  # of the 8-bit resampler's fixed-point coefficients (Pillow, src/libImaging/Resample.c)


def load_spec(data_dir):
    """`<data_dir>/dataset_spec.py` -> dict (data_loader.py:100-102)."""
    from .conf_loader import exec_dataset_spec
    path = os.path.join(data_dir, "dataset_spec.py")
    if not os.path.exists(path):
        raise FileNotFoundError(f"{path}: a dataset directory holds a dataset_spec.py (data_loader.py:100-102)")
    return exec_dataset_spec(path)


def spec_overrides(spec, fields):
    """the spec's non-list entries that are model hyper-parameters (gcp_builder.py:68 copies every non-list entry into the model's
    conf; the ones this build has no field for have nothing to override)"""
    return {k: v for k, v in spec.items() if not isinstance(v, (list, tuple)) and k in fields}


def _spec_class(spec):
    """the last component of the name of the spec's `dataset_class` (a string, or the placeholder class a spec file imports), or None"""
    c = spec.get("dataset_class")
    if c is None:
        return None
    name = c if isinstance(c, str) else getattr(c, "__name__", repr(c))
    return name.rsplit(".", 1)[-1]


def dataset_class_name(spec):
    """the spec's `dataset_class` (gcp_builder.py:105-113; FolderSplit when absent).  Any other class raises: the nav datasets'
    MazeTopRendered... re-renders frames with MiniWorld, and training on un-rendered frames without saying so is worse than stopping."""
    name = _spec_class(spec)
    if name is None:
        return _CLASSES[0]
    if name not in _CLASSES:
        raise ValueError(f"dataset_spec['dataset_class'] = {name}: only {' and '.join(_CLASSES)} are built (the nav datasets' "
                         "top-down re-rendering needs MiniWorld, which is not part of this build)")
    return name


def load_topdown_assets(data_dir):
    """`<data_dir>/topdown_assets.npz` (`data_dir` may also be the path of the `.npz` file itself: plan.py --topdown_assets) -> dict: background uint8 [S + 2cw, S + 2cw, 3], cw, n_rooms, scale, S, agent_stamp / goal_stamp
    bool [k, k], agent_color / goal_color uint8 [3].  S = int(table_size * scale) with table_size = (1 / 3) * int(sqrt(n_rooms)) as the
    reference computes it (multiroom3d layout; 256 for 9 rooms, 426 for 25 at the reference's scale of 256)."""
    path = data_dir if str(data_dir).endswith(".npz") else os.path.join(data_dir, TOPDOWN_ASSETS)
    if not os.path.exists(path):
        raise ValueError(f"{path} not found: a MazeTopRendered... dataset (Nav9Rooms, Nav25Rooms) trains on top-down pictures drawn from "
                         "the states; the static picture and the dot stamps come from the reference's OpenCV renderer and are dumped "
                         "once, with the .h5 -> .npz conversion (INTEGRATION.md, 'Top-down assets')")
    with np.load(path) as z:
        a = dict(background=np.ascontiguousarray(z["background"]), cw=int(z["crop_window"]), n_rooms=int(z["n_rooms"]),
                 scale=int(z["render_scale"]), agent_stamp=np.ascontiguousarray(z["agent_stamp"]).astype(bool),
                 goal_stamp=np.ascontiguousarray(z["goal_stamp"]).astype(bool), agent_color=z["agent_color"].astype(np.uint8).reshape(3),
                 goal_color=z["goal_color"].astype(np.uint8).reshape(3))
    a["S"] = int(topdown_table_size(a["n_rooms"]) * a["scale"])
    side, k = a["S"] + 2 * a["cw"], a["agent_stamp"].shape[0]
    if a["background"].dtype != np.uint8 or a["background"].shape != (side, side, 3):
        raise ValueError(f"{path}: background is {a['background'].dtype} {a['background'].shape}, expected uint8 {(side, side, 3)} "
                         f"(n_rooms {a['n_rooms']}, render_scale {a['scale']}, crop_window {a['cw']})")
    if not 4 <= 2 * a["cw"] <= 128:
        raise ValueError(f"{path}: crop_window {a['cw']}: the window side 2 * crop_window must be in [4, 128]")
    if a["agent_stamp"].shape != (k, k) or a["goal_stamp"].shape != (k, k) or k % 2 == 0 or k > 31:
        raise ValueError(f"{path}: the stamps are {a['agent_stamp'].shape} and {a['goal_stamp'].shape}: both [k, k], k odd, at most 31")
    return a


def topdown_table_size(n_rooms):
    """side of the maze in render units: `(1 / 3) * rooms_per_side`, a Python float as in the reference"""
    return (1 / 3) * int(math.sqrt(n_rooms))


def topdown_pixels(states_xy, n_rooms, scale, S, cw):
    """states [n, >= 2] -> int32 [n, 2]: (x, y) of each state in the padded top-down picture (convert_sim2topdown plus the crop-window
    correction, multiroom3d_env.py:194-208), in float32 as numpy evaluates the reference's expressions on float32 states;
    int() truncates toward zero."""
    p = np.asarray(states_xy, dtype=np.float32)[..., :2].reshape(-1, 2)
    q = (p * np.array([1, -1], dtype=np.float32)) / np.float32(27.0) + np.float32(0.5 * topdown_table_size(n_rooms))
    v = np.trunc(q * np.float32(scale)).astype(np.int64)
    out = np.stack([v[:, 0] + cw, (S + cw) - v[:, 1]], axis=1)
    return np.clip(out, -2 ** 31, 2 ** 31 - 1).astype(np.int32)


def _paint(win, stamp, color, px, py, lx, ly):
    """stamp centred on picture pixel (px, py) into the window whose first pixel is (lx, ly); the window lies inside the picture, so
    clipping to the window clips to the picture as well"""
    k, D = stamp.shape[0], win.shape[0]
    x0, y0 = px - k // 2 - lx, py - k // 2 - ly                     # the stamp's first entry in window coordinates
    xs, xe, ys, ye = max(x0, 0), min(x0 + k, D), max(y0, 0), min(y0 + k, D)
    if xs < xe and ys < ye:
        win[ys:ye, xs:xe][stamp[ys - y0:ye - y0, xs - x0:xe - x0]] = color


def topdown_fits(assets, xy):
    """bool [n]: the crop around pixel (x, y) lies inside the padded picture (where it does not, the reference fails on a shape mismatch)"""
    xy = np.asarray(xy).reshape(-1, 2).astype(np.int64)
    cw, side = assets["cw"], assets["background"].shape[0]
    return (np.maximum(xy, cw) + cw <= side).all(axis=1)


def render_topdown_numpy(assets, xy, goal_xy):
    """agent pixels int [n, 2] and the goal pixel [2] (topdown_pixels) -> uint8 [n, 2cw, 2cw, 3]: render_pos_top_down
    (multiroom3d_env.py:185-219) after its uint8 conversion.  The agent's dot, then the goal's, are painted on the padded picture and
    clipped at its border; the crop is centred on (max(cw, x), max(cw, y)).  Only the crop is copied."""
    xy = np.asarray(xy).reshape(-1, 2)
    if not topdown_fits(assets, xy).all():
        raise ValueError(f"top-down crop outside the padded picture for pixels {xy[~topdown_fits(assets, xy)].tolist()}")
    bg, cw = assets["background"], assets["cw"]
    gx, gy = (int(v) for v in goal_xy)
    out = np.empty((xy.shape[0], 2 * cw, 2 * cw, 3), dtype=np.uint8)
    for i, (x, y) in enumerate(xy.tolist()):
        lx, ly = max(cw, x) - cw, max(cw, y) - cw
        out[i] = bg[ly:ly + 2 * cw, lx:lx + 2 * cw]
        _paint(out[i], assets["agent_stamp"], assets["agent_color"], x, y, lx, ly)
        _paint(out[i], assets["goal_stamp"], assets["goal_color"], gx, gy, lx, ly)
    return out


def topdown_item_pixels(item, T, assets):
    """(raw, plan) of a top-rendered dataset -> (agent pixels int32 [n, 2] of the window states[offset : offset + T], goal pixel int32
    [2]): output frame t <= end_ind shows window frame min(t + chop, T - 1), the goal is the state shown at end_ind.  Raises when a
    frame's crop does not fit the padded picture."""
    raw, p = item
    pix = topdown_pixels(raw["states"][p["offset"]:p["offset"] + T], assets["n_rooms"], assets["scale"], assets["S"], assets["cw"])
    shown = np.minimum(np.arange(p["end_ind"] + 1) + p["chop"], T - 1)
    if shown[-1] >= pix.shape[0]:
        raise ValueError(f"{raw.get('name', 'item')}: end_ind {p['end_ind']} with chop {p['chop']} reads past the {pix.shape[0]} states")
    bad = ~topdown_fits(assets, pix[shown])
    if bad.any():
        t = int(np.argmax(bad))
        raise ValueError(f"{raw.get('name', 'item')}: the top-down crop of frame {t} (state {raw['states'][p['offset'] + shown[t], :2].tolist()}"
                         f", pixel {pix[shown[t]].tolist()}) does not fit the padded {assets['background'].shape[0]} px picture")
    return pix, pix[shown[-1]].copy()


class _FileCache(threading.local):
    def __init__(self):
        self.files = {}

    def get(self, path):
        f = self.files.get(path)
        if f is None:
            f = self.files[path] = np.load(path)
        return f


class VideoDataset:
    """FolderSplit / GlobalSplit VarLenVideoDataset (data_loader.py:104-290) over `.npz` files."""

    def __init__(self, data_dir, spec, phase, img_sz, randomize_length=False, randomize_start=False, dataset_size=-1, resize=False):
        self.data_dir, self.spec, self.phase, self.img_sz = data_dir, spec, phase, int(img_sz)
        self.resize = bool(resize)
        self.T = int(spec["max_seq_len"])
        self.randomize_length, self.randomize_start = bool(randomize_length), bool(randomize_start)
        self.dataset_size = dataset_size
        self.topdown = None
        if _spec_class(spec) in _TOPDOWN_CLASSES:                     # GlobalSplit file rules; frames drawn from the states
            self.kind = _CLASSES[1]
            self.topdown = load_topdown_assets(data_dir)
            self.resize = True                                        # always: the crop is 2cw, the model reads img_sz
        else:
            self.kind = dataset_class_name(spec)
        self.filenames = self._get_filenames()
        self._cache = _FileCache()
        self.traj_per_file = int(self._cache.get(self.filenames[0])["traj_per_file"])
        self.states_mean = self.states_den = None
        if "states_mean" in spec:                                     # data_loader.py:127-129, standardize :97-98
            self.states_mean = np.asarray(spec["states_mean"]).astype(np.float32)
            self.states_den = np.asarray(1e-6 + np.asarray(spec["states_std"])).astype(np.float32)
        # the size the frames are stored at: img_sz unless `resize`, then the size of item 0 (the loader's slots are sized once)
        self.src_size = (self.img_sz, self.img_sz)
        if self.topdown is not None:
            self.src_size = (2 * self.topdown["cw"],) * 2
        elif self.resize:
            im = self._cache.get(self.filenames[0])["traj0/images"]
            self.src_size = tuple(int(x) for x in im.shape[-3:-1])

    def _get_filenames(self):
        if self.kind == _CLASSES[0]:                                  # data_loader.py:264-272
            names = sorted(glob.glob(os.path.join(self.data_dir, "hdf5", self.phase + "/*")))
        else:                                                         # :275-290 (.npz instead of .h5)
            names = [os.path.join(r, f) for r, fs in _sorted_walk(self.data_dir) for f in fs
                     if f.endswith(".npz") and f not in ("dataset_info.npz", TOPDOWN_ASSETS)]
        if not names:
            raise RuntimeError(f"No filenames found in {self.data_dir}")
        random.Random(2).shuffle(names)                               # _shuffle_with_seed, :251-255
        if self.kind == _CLASSES[1]:
            names = self._split_with_percentage(self.spec["split"], names)
        return names

    def _split_with_percentage(self, frac, names):                   # :226-236
        assert sum(frac.values()) <= 1.0 and self.phase in frac
        if self.phase == "train":
            s, e = 0, frac["train"]
        elif self.phase == "val":
            s, e = frac["train"], frac["train"] + frac["val"]
        else:
            s, e = frac["train"] + frac["val"], frac["train"] + frac["val"] + frac["test"]
        return names[int(len(names) * s):int(len(names) * e)]

    def __len__(self):
        return self.dataset_size if self.dataset_size != -1 else len(self.filenames) * self.traj_per_file

    def read(self, index):
        """the raw arrays of item `index` (images uint8 [T_raw, H, W, 3] of camera 0 at their stored size, states / actions /
        pad_mask f32).  A top-rendered dataset reads no images (files may omit them): states[..., :2], actions, pad_mask and the
        trajectory's name for messages."""
        path = self.filenames[index // self.traj_per_file]
        F = self._cache.get(path)
        key = f"traj{index % self.traj_per_file}"
        raw = {}
        for name in ("images", "states", "actions", "pad_mask")[self.topdown is not None:]:
            k = f"{key}/{name}"
            if k in F.files:
                raw[name] = F[k] if name == "images" else F[k].astype(np.float32)
        if self.topdown is not None:
            if "states" not in raw:
                raise ValueError(f"{path}:{key}: a top-rendered dataset draws its frames from the states, which this trajectory lacks")
            raw["states"] = raw["states"][..., :2]                    # only x, y reach the model (data_loader.py:292-296)
            raw["name"] = f"{path}:{key}"
            return raw
        im = raw["images"]
        if im.ndim == 5:
            im = im[:, 0]                                             # number of cameras, data_loader.py:214-216
        if im.dtype != np.uint8:
            raise ValueError(f"{path}:{key}/images: frames are stored as uint8 (data_loader.py:217)")
        if self.resize:
            if im.shape[1:] != self.src_size + (3,):
                raise ValueError(f"{path}:{key}/images: frames are {im.shape[1]}x{im.shape[2]}, item 0 of the dataset has "
                                 f"{self.src_size[0]}x{self.src_size[1]}: every trajectory of a resized dataset has one stored size")
        elif im.shape[1:] != (self.img_sz, self.img_sz, 3):
            raise ValueError(f"{path}:{key}/images: frames are {im.shape[1]}x{im.shape[2]}, the model reads {self.img_sz}x{self.img_sz}. "
                             "The reference resizes with blox.vis.resize_video, which is not part of this build: store the frames "
                             "at the model's resolution. Or pass resize=True (train.py --resize_frames 1): the frames are then "
                             "resized on the device as Pillow's bilinear Image.resize would")
        raw["images"] = im
        return raw

    def pad_mask(self, index):
        """the pad mask of item `index` alone (f32 [T_raw]): all that `draw` reads of an item, and its length is the trajectory's
        (dataset_resident.py sizes its store from these before it reads a frame)"""
        F = self._cache.get(self.filenames[index // self.traj_per_file])
        return F[f"traj{index % self.traj_per_file}/pad_mask"].astype(np.float32)

    def draw(self, raw, rs):
        """the reference's per-item draws (data_loader.py:144-156,175-211) from RandomState rs, in its order.  Returns the plan:
        offset (window start in the raw arrays), chop, zero_from (frames >= it are zero), end_ind and the pad mask [T]."""
        T = self.T
        pm = raw["pad_mask"]
        end_ind = int(np.argmax(pm * np.arange(pm.shape[0], dtype=np.float32), 0))
        start_ind = rs.randint(0, end_ind - 1) if self.randomize_start else 0
        extra = (end_ind - start_ind + 1) - T                         # sample_max_len_video
        offset = max(0, int(rs.rand() * (extra + 1))) + start_ind if self.phase == "train" else 0
        end_ind = min(end_ind - offset, T - 1)
        chop, zero_from = 0, T
        pad_mask = _maybe_pad(pm, offset, T)
        if self.randomize_length:                                     # _randomize_length (start_ind is 0 here by design)
            length = 3 + int(rs.rand() * (end_ind - 2))
            chop = int(rs.rand() * (end_ind + 1 - length))
            end_ind = length - 1
            pad_mask = (np.arange(T) <= end_ind).astype(np.float32)
            zero_from = end_ind + 1
            if chop < 0:
                raise ValueError(f"sequence too short for randomize_length (end_ind {end_ind})")
        return dict(offset=offset, chop=chop, zero_from=zero_from, end_ind=end_ind, pad_mask=pad_mask)

    def item(self, index, rs):
        raw = self.read(index)
        return raw, self.draw(raw, rs)


def _sorted_walk(top):
    for r, ds, fs in os.walk(top):
        ds.sort()
        yield r, sorted(fs)


def _maybe_pad(val, offset, T):                                       # data_loader.py:239-248
    val = val[offset:]
    if val.shape[0] >= T:
        return val[:T]
    return np.concatenate((val, np.zeros([T - val.shape[0]] + list(val.shape[1:]), dtype=val.dtype)))


def _time_map(a, plan, L):
    """randomize_length's chop + repeat of the last step and zeroing after end_ind (data_loader.py:203-206) on a padded array of L"""
    idx = np.minimum(np.arange(L) + plan["chop"], L - 1)
    out = a[idx]
    out[plan["zero_from"]:] = 0
    return out


def resize_ksize(n_in, n_out):
    """taps per output sample of one axis: Pillow's `(int)ceil(support) * 2 + 1` with the bilinear support 1.0 * max(n_in / n_out, 1)"""
    return int(math.ceil(max(n_in / n_out, 1.0))) * 2 + 1


def resize_coeffs(n_in, n_out):
    """One axis of Pillow's 8-bit bilinear resampler (Resample.c: precompute_coeffs + normalize_coeffs_8bpc) -> (k int32 [n_out, ksize],
    bounds int32 [n_out, 2]): output sample xx is clip((2^21 + sum_x in[bounds[xx, 0] + x] * k[xx, x]) >> 22, 0, 255) over
    x < bounds[xx, 1]; taps past that count are 0.  Float64 in Pillow's order of operations (python floats are C doubles)."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 1.0 * fs
    ksize = resize_ksize(n_in, n_out)
    ss = 1.0 / fs
    k = np.zeros((n_out, ksize), dtype=np.int32)
    bounds = np.zeros((n_out, 2), dtype=np.int32)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)                   # int(): C truncation, the operands are positive or clamped
        xmax = min(int(center + support + 0.5), n_in) - xmin
        w = [max(0.0, 1.0 - abs((x + xmin - center + 0.5) * ss)) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        for x in range(xmax):
            v = w[x] / ww if ww != 0.0 else w[x]
            k[xx, x] = int(v * (1 << PRECISION_BITS) + 0.5)
        bounds[xx] = (xmin, xmax)
    return k, bounds


def _resample_axis(a, axis, n_out):
    """one pass of the resampler along `axis` of a uint8 array, rounding to uint8"""
    n_in = a.shape[axis]
    k, bounds = resize_coeffs(n_in, n_out)
    a = np.moveaxis(a, axis, -1)
    acc = np.full(a.shape[:-1] + (n_out,), 1 << (PRECISION_BITS - 1), dtype=np.int32)
    for x in range(k.shape[1]):
        acc += a[..., np.minimum(bounds[:, 0] + x, n_in - 1)].astype(np.int32) * k[:, x]     # k is 0 past bounds[:, 1]
    out = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return np.moveaxis(out, -1, axis)


def resize_frames_numpy(frames, img_sz):
    """uint8 [..., H_s, W_s, 3] -> [..., img_sz, img_sz, 3] as `Image.resize((img_sz, img_sz), BILINEAR)` of Pillow does per frame,
    bit for bit: horizontal pass, then vertical pass, each rounding to uint8; a pass that keeps its length is skipped.  Integer
    arithmetic (the int32 accumulator stays below 2^31: the coefficients of a sample sum to 2^22 up to rounding)."""
    frames = np.asarray(frames)
    assert frames.dtype == np.uint8 and frames.ndim >= 3 and frames.shape[-1] == 3
    if frames.shape[-2] != img_sz:
        frames = _resample_axis(frames, frames.ndim - 2, img_sz)
    if frames.shape[-3] != img_sz:
        frames = _resample_axis(frames, frames.ndim - 3, img_sz)
    return np.ascontiguousarray(frames)


def assemble_numpy(items, T, states_mean=None, states_den=None, img_sz=None, topdown=None):
    """[(raw, plan)] -> the model's inputs as numpy arrays, by the reference's own steps (pad, chop, [resize to img_sz,] convert) —
    what gcpx_assemble_batch (gcpx_resize_assemble_batch when the frames are resized) computes, bit for bit.  With `topdown` (the assets
    of a top-rendered dataset) the frames up to end_ind are rendered from the states and resized to img_sz, the rest is zero:
    gcpx_topdown_assemble_batch."""
    out = {k: [] for k in ("traj_seq", "pad_mask", "end_ind", "start_ind", "traj_seq_states", "actions")}
    for raw, p in items:
        if topdown is not None:
            pix, goal = topdown_item_pixels((raw, p), T, topdown)
            n = p["end_ind"] + 1
            im = np.zeros((T, 2 * topdown["cw"], 2 * topdown["cw"], 3), dtype=np.uint8)
            im[:n] = render_topdown_numpy(topdown, pix[np.minimum(np.arange(n) + p["chop"], T - 1)], goal)
        else:
            im = _time_map(_maybe_pad(raw["images"], p["offset"], T), p, T)
        if img_sz is not None and im.shape[1:3] != (img_sz, img_sz):          # data_loader.py:213-220: after the time map
            im = resize_frames_numpy(im, img_sz)
        im = np.transpose(im, (0, 3, 1, 2)).astype(np.float32) / 255 * 2 - 1
        out["traj_seq"].append(im)
        out["pad_mask"].append(p["pad_mask"].astype(np.float32))
        out["end_ind"].append(p["end_ind"])
        out["start_ind"].append(0)
        if "states" in raw:
            s = _time_map(_maybe_pad(raw["states"], p["offset"], T), p, T)
            if states_mean is not None:
                s = (s - states_mean) / states_den
            out["traj_seq_states"].append(s.astype(np.float32))
        if "actions" in raw:
            out["actions"].append(_time_map(_maybe_pad(raw["actions"], p["offset"], T)[:-1], p, T - 1))
    res = {k: np.stack(v) if k not in ("end_ind", "start_ind") else np.array(v, dtype=np.int64) for k, v in out.items() if len(v)}
    B = len(items)
    res["I_0"] = res["traj_seq"][:, 0].copy()
    res["I_g"] = res["traj_seq"][np.arange(B), res["end_ind"]].copy()
    return res


def item_rng(seed, cycle, pos):
    """the draws of the item at position `pos` of cycle `cycle` of a loader seeded `seed`: keyed, so a resumed run draws the same"""
    return np.random.RandomState(np.random.SeedSequence([int(seed), int(cycle), int(pos)]).generate_state(4))


def batch_schedule(n_items, batch_size, seed, cycle, shuffle, rank=0, world=1):
    """[(dataset index, position)] per batch of this rank for one pass over the data (drop_last): one order shared by all ranks, rank r
    of W takes items [r·B, (r+1)·B) of each global batch of W·B — together they consume what one process with batch W·B would."""
    order = np.arange(n_items)
    if shuffle:
        order = np.random.RandomState(np.random.SeedSequence([int(seed), int(cycle)]).generate_state(4)).permutation(n_items)
    gb = batch_size * world
    return [[(int(order[g * gb + rank * batch_size + j]), g * gb + rank * batch_size + j) for j in range(batch_size)]
            for g in range(n_items // gb)]


def epoch_schedule(n_items, batch_size, n_repeat, seed, epoch, shuffle, rank=0, world=1):
    """one epoch = n_repeat passes (RepeatedDataLoader, data_loader.py:83-88): [[(dataset index, position, cycle)] per batch]"""
    out = []
    for r in range(n_repeat):
        cycle = epoch * n_repeat + r
        out += [[(i, p, cycle) for i, p in b] for b in batch_schedule(n_items, batch_size, seed, cycle, shuffle, rank, world)]
    return out


def accumulate_schedule(n_items, batch_size, n_repeat, seed, epoch, shuffle, rank=0, world=1, accumulate=1):
    """epoch_schedule of a loader that feeds gradient accumulation over `accumulate` = k micro-batches: for each global batch g of a pass
    and j = 0 .. k-1, the batch of virtual rank rank·k + j of a virtual world world·k -- the sequences k times as many ranks would
    read, in the order one trainer folds them.  A pass drops its leftover items as the world·k run drops them, so every pass (n_repeat
    > 1 included) is a whole number of cycles."""
    k = int(accumulate)
    if k == 1:
        return epoch_schedule(n_items, batch_size, n_repeat, seed, epoch, shuffle, rank, world)
    per = [epoch_schedule(n_items, batch_size, n_repeat, seed, epoch, shuffle, rank * k + j, world * k) for j in range(k)]
    return [per[j][g] for g in range(len(per[0])) for j in range(k)]


def numpy_batch(ds, batch, seed):
    """one scheduled batch assembled on the host by assemble_numpy"""
    return assemble_numpy([ds.item(i, item_rng(seed, c, p)) for i, p, c in batch], ds.T, ds.states_mean, ds.states_den,
                          img_sz=ds.img_sz if ds.resize else None, topdown=ds.topdown)


def pack_item(item, j, frames, aux, info, B, T, S, A, topdown=None):
    """sequence j of a staging slot (numpy views): the uint8 window raw[offset : offset + T], pad mask / state / action windows in
    aux = [pad_mask B*T | states B*T*S | actions B*(T-1)*A], and the per-sequence integers of gcpx_assemble_batch.  With `topdown`
    (the assets of a top-rendered dataset) `frames` is the int32 coordinate slot [B*T*2 agent pixels | B*2 goal pixels] instead (the
    kernel renders frames up to end_ind only; states and actions keep the time map of every dataset)."""
    raw, p = item
    o = p["offset"]
    if topdown is not None:
        fr, goal = topdown_item_pixels(item, T, topdown)
        frames[:B * T * 2].reshape(B, T, 2)[j, :fr.shape[0]] = fr
        frames[B * T * 2:].reshape(B, 2)[j] = goal
    else:
        fr = raw["images"][o:o + T]
        frames[j, :fr.shape[0]] = fr
    aux[j * T:(j + 1) * T] = p["pad_mask"]
    n_s = n_a = 0
    if S:
        s = raw["states"][o:o + T]
        aux[B * T:B * T * (1 + S)].reshape(B, T, S)[j, :s.shape[0]] = s
        n_s = s.shape[0]
    if A:
        a = raw["actions"][o:o + T - 1]
        aux[B * T * (1 + S):].reshape(B, T - 1, A)[j, :a.shape[0]] = a
        n_a = a.shape[0]
    info[j] = (fr.shape[0], n_s, n_a, p["chop"], p["zero_from"], p["end_ind"], 0, 0)


# ---- the argument groups the five assembly entry points share (include/gcpx.h), each built in one place ----
def opt_ptr(x):
    return x.data_ptr() if x is not None else None


def aux_args(aux, B, T, S, A):
    """pad_in, states_in, actions_in: the three parts of aux = [pad_mask B*T | states B*T*S | actions B*(T-1)*A] (f32, on the device)"""
    a = aux.data_ptr()
    return a, a + 4 * B * T if S else None, a + 4 * B * T * (1 + S) if A else None


def table_args(tables):
    """kx, bx, ky, by of `tables` = resize_tables on the device; the tap counts ksx, ksy are kx.shape[1], ky.shape[1]"""
    return tuple(t.data_ptr() for t in tables)


def output_args(out, stream):
    """the tail of every entry point: the eight tensors of `out` (the model's input names; absent ones null) and the stream"""
    return tuple(opt_ptr(out.get(k)) for k in ("traj_seq", "I_0", "I_g", "pad_mask", "end_ind", "start_ind", "traj_seq_states",
                                             "actions")) + (stream,)


def assemble_into(lib, frames, aux, info, lut, mean, den, out, S, A, stream):
    """gcpx_assemble_batch from device staging tensors into the device tensors of `out` (the model's input names)"""
    B, T, H, W, _ = frames.shape
    rt.check(lib.gcpx_assemble_batch(frames.data_ptr(), info.data_ptr(), lut.data_ptr(), *aux_args(aux, B, T, S, A), opt_ptr(mean),
                                     opt_ptr(den), B, T, H, W, S, A, *output_args(out, stream)), "assemble_batch")


def resize_tables(Hs, Ws, img_sz):
    """the int32 tables gcpx_resize_assemble_batch reads: (kx [img_sz, ksx], bx [img_sz, 2], ky [img_sz, ksy], by [img_sz, 2])"""
    kx, bx = resize_coeffs(Ws, img_sz)
    ky, by = resize_coeffs(Hs, img_sz)
    return kx, bx, ky, by


def resize_assemble_into(lib, frames, aux, info, lut, tables, mean, den, out, S, A, stream):
    """gcpx_resize_assemble_batch from device staging tensors (frames at their stored size, `tables` = resize_tables on the device)
    into the device tensors of `out` (the model's input names, at the model's size)"""
    B, T, Hs, Ws, _ = frames.shape
    H, W = out["traj_seq"].shape[-2:]
    rt.check(lib.gcpx_resize_assemble_batch(frames.data_ptr(), info.data_ptr(), lut.data_ptr(), *table_args(tables),
                                            *aux_args(aux, B, T, S, A), opt_ptr(mean), opt_ptr(den), B, T, Hs, Ws, H, W, tables[0].shape[1],
                                            tables[2].shape[1], S, A, *output_args(out, stream)), "resize_assemble_batch")


def topdown_device_assets(assets, img_sz, device):
    """what gcpx_topdown_assemble_batch keeps on the device for a dataset: the padded picture, both stamps (uint8) and the resize tables
    for (2cw, 2cw) -> img_sz; plus the host-side integers of the call"""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    rgb = lambda c: int(c[0]) | int(c[1]) << 8 | int(c[2]) << 16
    D = 2 * assets["cw"]
    return dict(background=t(assets["background"]), agent_stamp=t(assets["agent_stamp"].astype(np.uint8)),
                goal_stamp=t(assets["goal_stamp"].astype(np.uint8)), tables=tuple(t(x) for x in resize_tables(D, D, img_sz)),
                cw=assets["cw"], k=int(assets["agent_stamp"].shape[0]), agent_rgb=rgb(assets["agent_color"]),
                goal_rgb=rgb(assets["goal_color"]))


def topdown_assemble_into(lib, dev_assets, coords, aux, info, lut, mean, den, out, S, A, stream):
    """gcpx_topdown_assemble_batch from the device-resident assets (topdown_device_assets) and the staging tensors (coords int32
    [B*T*2 + B*2], aux, info) into the device tensors of `out` (the model's input names)"""
    B, T = out["traj_seq"].shape[:2]
    H, W = out["traj_seq"].shape[-2:]
    d, c = dev_assets, coords.data_ptr()
    tables = d["tables"]
    rt.check(lib.gcpx_topdown_assemble_batch(d["background"].data_ptr(), d["background"].shape[0], d["cw"], d["agent_stamp"].data_ptr(),
                                             d["goal_stamp"].data_ptr(), d["k"], d["agent_rgb"], d["goal_rgb"], c, c + 4 * B * T * 2,
                                             info.data_ptr(), lut.data_ptr(), *table_args(tables), *aux_args(aux, B, T, S, A),
                                             opt_ptr(mean), opt_ptr(den), B, T, H, W, tables[0].shape[1], tables[2].shape[1], S, A,
                                             *output_args(out, stream)), "topdown_assemble_batch")


class _Streams:
    """the H2D copy stream and the ring's events.  copy_done[s]: slot s's last upload finished (its pinned slot may be refilled);
    assembled[s]: the assembly kernel that read device slot s has run (the slot may be overwritten)."""

    def __init__(self, device, n):
        self.copy = torch.cuda.Stream(device=device)
        self.copy_done = [torch.cuda.Event() for _ in range(n)]
        self.assembled = [torch.cuda.Event() for _ in range(n)]


class RingLoader:
    """What HostFedLoader and ResidentLoader (dataset_resident.py) share: the epoch's schedule and a ring of `n_slots` slots, each a set
    of pinned host tensors and their device copies.  Per batch a slot is filled on worker threads, copied up on the copy stream and
    read by one assembly call on the caller's current stream, which writes `model.input_buffer(...)`: the tensors yielded ARE those
    buffers (no staging copy in the forward), and each batch is assembled when the next one is asked for, i.e. behind the previous
    step.  RepeatedDataLoader semantics (n_repeat passes per epoch, data_loader.py:83-88), drop_last, shuffle in the train phase only.

    Slot reuse has two rules, each enforced in one place:
      1. a pinned slot is refilled only after its upload has completed (`_job`, on the worker thread);
      2. a device slot is overwritten only after the assembly that read it has run (`_upload`, on the copy stream).

    A loader supplies three things:
      `_jobs(batch)` -> [(method, *args)]: how a slot is filled, the calls method(slot, *args) of one worker job each;
      `_alloc_slots(dev, n)` -> (Hs, Ws) the frames are stored at, or None: what is copied up, self.pin / self.dev = {name: [per slot]};
      `_launch(slot, out, stream)`: the assembly call that reads device slot `slot` and writes the tensors of `out` on `stream`.
    `__iter__` decides from the fill futures alone (when to wait, when to upload, when to upload the next slot early, when to
    resubmit) and reaches the device only through `_submit`, `_upload` and `_assemble`."""

    def __init__(self, dataset, model, batch_size, n_repeat, seed, rank, world, n_slots, shuffle, n_workers, accumulate=1):
        if rank is None or world is None:
            d = torch.distributed
            on = d.is_available() and d.is_initialized()
            rank = d.get_rank() if on else 0
            world = d.get_world_size() if on else 1
        assert n_slots >= 2
        if int(accumulate) < 1:
            raise ValueError(f"accumulate must be a positive number of micro-batches, not {accumulate!r}")
        self.accumulate = int(accumulate)              # micro-batches per optimizer step (accumulate_schedule)
        self.ds, self.model, self.B = dataset, model, int(batch_size)
        self.n_repeat, self.seed, self.rank, self.world = int(n_repeat), int(seed), int(rank), int(world)
        self.shuffle = (dataset.phase == "train") if shuffle is None else bool(shuffle)
        self.n_slots, self.epoch = n_slots, 0
        self.pool = ThreadPoolExecutor(max_workers=n_workers)
        hp = model._hp
        if hp.max_seq_len != dataset.T or hp.img_sz != dataset.img_sz:
            raise ValueError(f"dataset (T={dataset.T}, {dataset.img_sz}px) and model (T={hp.max_seq_len}, {hp.img_sz}px) differ")
        if hp.batch_size != self.B:
            raise ValueError(f"loader batch {self.B} != model batch {hp.batch_size}")
        self.S = self.A = 0                            # state / action widths: the loader sets them
        self.pin = self.dev = self.streams = None      # the ring, allocated with the first batch (_alloc)

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def __len__(self):
        return self.n_repeat * self.accumulate * (len(self.ds) // (self.B * self.world * self.accumulate))

    def schedule(self):
        """this rank's batches of the current epoch: [(dataset index, position, cycle)]"""
        return accumulate_schedule(len(self.ds), self.B, self.n_repeat, self.seed, self.epoch, self.shuffle, self.rank, self.world,
                                   self.accumulate)

    def numpy_batches(self):
        """the same batches as numpy arrays assembled on the host (the device-fed path of the tests and of tools/host_fed_loop.py)"""
        for b in self.schedule():
            yield numpy_batch(self.ds, b, self.seed)

    # ---- the ring ----
    def _alloc(self):
        dev = self.model.device
        src = self._alloc_slots(dev, self.n_slots)
        self.lut = torch.from_numpy(LUT).to(dev)
        self.mean = self.den = self.tables = None
        if self.ds.states_mean is not None and self.S:
            self.mean = torch.from_numpy(self.ds.states_mean).to(dev)
            self.den = torch.from_numpy(self.ds.states_den).to(dev)
        if src is not None and tuple(src) != (self.ds.img_sz, self.ds.img_sz):
            self.tables = tuple(torch.from_numpy(t).to(dev) for t in resize_tables(src[0], src[1], self.ds.img_sz))
        self.streams = _Streams(dev, self.n_slots)

    def _job(self, slot, fn, *args):
        self.streams.copy_done[slot].synchronize()    # rule 1: the slot's previous upload has completed (the worker thread waits)
        fn(slot, *args)

    def _submit(self, slot, batch):
        """start filling pinned slot `slot` with `batch` -> the futures of its jobs"""
        if self.streams is None:
            self._alloc()
        return [self.pool.submit(self._job, slot, *job) for job in self._jobs(batch)]

    def _upload(self, slot):
        st = self.streams
        with torch.cuda.stream(st.copy):
            st.copy.wait_event(st.assembled[slot])    # rule 2: the assembly that read this device slot has run
            for k in self.pin:
                self.dev[k][slot].copy_(self.pin[k][slot], non_blocking=True)
            st.copy_done[slot].record(st.copy)

    def _assemble(self, slot):
        m, st = self.model, self.streams
        B, T, S, A, H = self.B, self.ds.T, self.S, self.A, self.ds.img_sz
        caller = torch.cuda.current_stream(m.device)
        caller.wait_event(st.copy_done[slot])
        ib = m.input_buffer
        out = dict(traj_seq=ib("traj_seq", (B, T, 3, H, H)), I_0=ib("I_0", (B, 3, H, H)), I_g=ib("I_g", (B, 3, H, H)),
                   pad_mask=ib("pad_mask", (B, T)), end_ind=ib("end_ind", (B,)), start_ind=ib("start_ind", (B,), torch.int64))
        if S:
            out["traj_seq_states"] = ib("traj_seq_states", (B, T, S))
        if A:
            out["actions"] = ib("actions", (B, T - 1, A))
        self._launch(slot, out, caller.cuda_stream)
        st.assembled[slot].record(caller)
        return out

    def __iter__(self):
        batches = self.schedule()
        n = self.n_slots
        futs = {k: self._submit(k % n, batches[k]) for k in range(min(n, len(batches)))}
        uploaded = set()
        for k in range(len(batches)):
            s = k % n
            if k not in uploaded:
                for f in futs.pop(k):
                    f.result()
                self._upload(s)
            out = self._assemble(s)
            if k + n < len(batches):
                futs[k + n] = self._submit(s, batches[k + n])
            # the next batch's upload goes out now if its slot is filled: it then runs under this step
            if k + 1 < len(batches) and all(f.done() for f in futs[k + 1]):
                for f in futs.pop(k + 1):
                    f.result()
                self._upload((k + 1) % n)
                uploaded.add(k + 1)
            yield out


class HostFedLoader(RingLoader):
    """Yields the model's input dicts, assembled on the device from uint8 frames uploaded from the ring's pinned host slots: every
    item is read, sliced and packed by one of `n_workers` threads.  A dataset read with resize=True whose frames are stored at
    another size than the model's is uploaded at that size (the slots hold H_s x W_s frames) and resized in the assembly, over tables
    uploaded once.  A top-rendered dataset (dataset.topdown) has no frame slots at all: a slot holds int32 pixel coordinates
    [B][T][2] + [B][2], and the padded picture, the stamps and the tables for (2cw, 2cw, img_sz) stay on the device."""

    def __init__(self, dataset, model, batch_size, n_repeat=1, seed=0, rank=None, world=None, n_slots=2, n_workers=4, shuffle=None,
                 accumulate=1):
        super().__init__(dataset, model, batch_size, n_repeat, seed, rank, world, n_slots, shuffle, n_workers, accumulate=accumulate)
        raw0 = dataset.read(0)
        self.S = raw0["states"].shape[-1] if "states" in raw0 else 0
        self.A = raw0["actions"].shape[-1] if "actions" in raw0 else 0
        self.topdown = None                            # topdown_device_assets of a top-rendered dataset

    def _alloc_slots(self, dev, n):
        B, T, S, A = self.B, self.ds.T, self.S, self.A
        H, W = self.ds.src_size                        # the slots hold the frames as stored; the resize is part of the assembly
        top = self.ds.topdown is not None
        slot = {"coords": ((B * T * 2 + B * 2,), torch.int32)} if top else {"frames": ((B, T, H, W, 3), torch.uint8)}
        slot.update(aux=((B * T + B * T * S + B * (T - 1) * A,), torch.float32), info=((B, N_INFO), torch.int32))
        self.pin = {k: [torch.zeros(shape, dtype=t, pin_memory=True) for _ in range(n)] for k, (shape, t) in slot.items()}
        self.dev = {k: [torch.empty(shape, dtype=t, device=dev) for _ in range(n)] for k, (shape, t) in slot.items()}
        if top:
            self.topdown = topdown_device_assets(self.ds.topdown, self.ds.img_sz, dev)
        return None if top else (H, W)

    def _jobs(self, batch):
        return [(self._fill_item, j, i, p, c) for j, (i, p, c) in enumerate(batch)]

    def _fill_item(self, slot, j, index, pos, cycle):
        item = self.ds.item(index, item_rng(self.seed, cycle, pos))
        fkey = "coords" if self.ds.topdown is not None else "frames"
        pack_item(item, j, self.pin[fkey][slot].numpy(), self.pin["aux"][slot].numpy(), self.pin["info"][slot].numpy(), self.B,
                  self.ds.T, self.S, self.A, topdown=self.ds.topdown)

    def _launch(self, slot, out, stream):
        lib, d = self.model.lib, {k: v[slot] for k, v in self.dev.items()}
        tail = (self.mean, self.den, out, self.S, self.A, stream)
        if self.topdown is not None:
            topdown_assemble_into(lib, self.topdown, d["coords"], d["aux"], d["info"], self.lut, *tail)
        elif self.tables is None:
            assemble_into(lib, d["frames"], d["aux"], d["info"], self.lut, *tail)
        else:
            resize_assemble_into(lib, d["frames"], d["aux"], d["info"], self.lut, self.tables, *tail)
