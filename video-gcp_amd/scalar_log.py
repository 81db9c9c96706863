"""Scalar logs of the trainer: what the reference writes through its tensorboardX logger on every logging step -- every loss term as
`<name>_loss_<phase>` (base_model.py:104-108, logger.py:43-44), `gradients/mean_norm` / `gradients/max_norm` over the per-parameter
gradient norms (base_model.py:139-146), the layer-wise KL of the tree (tree_module.py:159-169), the validation averages
(train.py:198-230) -- into <exp>/events (gcp_builder.py:41-54): a TensorBoard event file and `scalar_data.json` (logger.py:98-100).

The module imports without a GPU (and without torch): the writer is `struct` alone, as image_log.py writes PNG with zlib + struct.
Event file = TFRecord framing (u64 length, masked CRC-32C of the length, payload, masked CRC-32C of the payload) around hand-encoded
`Event` messages: wall_time = 1 (double), step = 2 (int64), file_version = 3 (first record, "brain.Event:2") or
summary = 5 {value = 1 {tag = 1, simple_value = 2 (float)}}.  No TensorBoard was at hand to read a file back: the format is pinned by
tests/test_scalar_log_cpu.py alone.

The device side (csrc/train_stats.hip): `gcpx_grad_segment_norms` over the trainer's flat gradient, from the chunk table `grad_tables`
builds once per model; `gcpx_kl_layerwise` over the q_z / p_z rows the forward leaves behind.  `segment_norms_numpy` restates the first
in numpy and is its checker, as visualization.compose is the panel kernel's.
"""
import json
import os
import socket
import struct
import time

import numpy as np

# the shape of the kernel's sums (include/gcpx.h; tests/test_scalar_log_cpu.py holds the two files together)
GRAD_NORM_THREADS = 256
GRAD_NORM_CHUNK = 16384
GRAD_NORM_SERIAL = GRAD_NORM_CHUNK // GRAD_NORM_THREADS + 1
GRAD_NORM_TREE_DEPTH = 8
GRAD_CHUNK_DTYPE = np.dtype([("first", "<i8"), ("seg", "<i4"), ("length", "<i4")])        # gcpx_grad_chunk
BUFFER_SUFFIXES = (".running_mean", ".running_var")            # buffers, not parameters: `self.parameters()` does not hold them


# ---- CRC-32C (Castagnoli, reflected polynomial 0x82F63B78) and the TFRecord mask ----
def _crc_table():
    tab = []
    for i in range(256):
        c = i
        for _ in range(8):
            c = (c >> 1) ^ 0x82F63B78 if c & 1 else c >> 1
        tab.append(c)
    return tab


_CRC_TABLE = _crc_table()


def crc32c(data):
    c = 0xFFFFFFFF
    for b in bytes(data):
        c = _CRC_TABLE[(c ^ b) & 0xFF] ^ (c >> 8)
    return c ^ 0xFFFFFFFF


def masked_crc32c(data):
    c = crc32c(data)
    return ((c >> 15 | c << 17) + 0xA282EAD8) & 0xFFFFFFFF


# ---- protobuf wire format: just the five fields above ----
def _varint(v):
    v &= (1 << 64) - 1                       # int64: a negative value travels as its 64-bit two's complement
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def _bytes_field(field, payload):
    return _varint(field << 3 | 2) + _varint(len(payload)) + payload


def encode_event(wall_time, step, tag=None, value=None, file_version=None):
    ev = _varint(1 << 3 | 1) + struct.pack("<d", wall_time) + _varint(2 << 3 | 0) + _varint(int(step))
    if file_version is not None:
        ev += _bytes_field(3, file_version.encode())
    if tag is not None:
        val = _bytes_field(1, tag.encode()) + _varint(2 << 3 | 5) + struct.pack("<f", value)
        ev += _bytes_field(5, _bytes_field(1, val))
    return ev


def tf_record(payload):
    head = struct.pack("<Q", len(payload))
    return head + struct.pack("<I", masked_crc32c(head)) + payload + struct.pack("<I", masked_crc32c(payload))


class ScalarLogger:
    """Logger.log_scalar / dump_scalars of the reference (logger.py:43-44,98-100) over the two sinks of <log_dir>."""

    def __init__(self, log_dir):
        self.log_dir = log_dir
        os.makedirs(log_dir, exist_ok=True)
        now = time.time()
        self.event_path = os.path.join(log_dir, "events.out.tfevents.{:010d}.{}".format(int(now), socket.gethostname()))
        self._file = open(self.event_path, "ab")
        self._file.write(tf_record(encode_event(now, 0, file_version="brain.Event:2")))
        self._file.flush()
        self.scalars = {}                     # {tag: [[wall_time, step, value], ...]}: what export_scalars_to_json writes

    def log_scalar(self, value, name, step, phase):
        tag = "{}_{}".format(name, phase)
        value, step, now = float(value), int(step), time.time()
        self.scalars.setdefault(tag, []).append([now, step, value])
        self._file.write(tf_record(encode_event(now, step, tag=tag, value=value)))

    def flush(self):
        self._file.flush()

    def dump_scalars(self, log_path=None):
        log_path = os.path.join(self.log_dir, "scalar_data.json") if log_path is None else log_path
        tmp = log_path + ".tmp"
        with open(tmp, "w") as f:
            json.dump(self.scalars, f)
        os.replace(tmp, log_path)                # a reader never sees half a file
        return log_path

    def close(self):
        if not self._file.closed:
            self._file.close()


# ---- gradient norms: the tables of gcpx_grad_segment_norms ----
def grad_tables(poff, chunk=GRAD_NORM_CHUNK, buffers=False):
    """(names, chunks, seg_chunk0) from a model's `_poff` {name: (offset, shape)}: the counted segments (parameters; buffers are left
    out by name, empty tensors have no norm) in layout order, each cut into pieces of at most `chunk` elements -- chunks: structured
    array (first, seg, length) with the pieces of one segment adjacent; seg_chunk0 [n_seg + 1]: first chunk of every segment.
    buffers=True keeps the buffers: the table of the weights themselves (health.py scans theta with it before a checkpoint)."""
    names, rows, seg_chunk0 = [], [], [0]
    for name, (off, shape) in poff.items():
        numel = int(np.prod(shape, dtype=np.int64)) if len(shape) else 1
        if (name.endswith(BUFFER_SUFFIXES) and not buffers) or numel == 0:
            continue
        s = len(names)
        names.append(name)
        for lo in range(0, numel, chunk):
            rows.append((off + lo, s, min(chunk, numel - lo)))
        seg_chunk0.append(len(rows))
    return names, np.array(rows, dtype=GRAD_CHUNK_DTYPE), np.array(seg_chunk0, dtype=np.int32)


def _chunk_sqsum_f32(x, aligned):
    """the sum of squares of one chunk in the kernel's shape, in f32: per-thread serial runs, the wavefront butterfly, the four
    wavefronts.  (A product and a sum round twice where the kernel's fmaf rounds once: the mirror equals the kernel to a rounding
    per element, not bit for bit.)"""
    T = GRAD_NORM_THREADS
    acc = np.zeros(T, np.float32)
    x = np.asarray(x, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        if aligned:
            nvec = len(x) // 4
            quads, tail = x[:4 * nvec].reshape(nvec, 4), x[4 * nvec:]
            for v0 in range(0, nvec, T):
                q = quads[v0:v0 + T]
                for k in range(4):
                    acc[:len(q)] += q[:, k] * q[:, k]
            acc[:len(tail)] += tail * tail
        else:
            for e0 in range(0, len(x), T):
                e = x[e0:e0 + T]
                acc[:len(e)] += e * e
        w = acc.reshape(T // 64, 64)
        m = 1
        while m < 64:                          # v += shfl_xor(v, m)
            w = w + w[:, np.arange(64) ^ m]
            m <<= 1
        return np.float32(np.float32(w[0, 0] + w[1, 0]) + np.float32(w[2, 0] + w[3, 0]))


def segment_norms_numpy(grad, chunks, seg_chunk0, grad_scale=1.0, coef=1.0):
    """numpy restatement of gcpx_grad_segment_norms: (seg_norm [n_seg] f32, stats [4] f32)"""
    grad = np.asarray(grad, np.float32)
    n_seg = len(seg_chunk0) - 1
    coef = 1.0 if not coef else coef
    mul = abs(float(np.float32(grad_scale))) * float(np.float32(coef))
    seg_norm, counted = np.zeros(n_seg, np.float32), np.zeros(n_seg, bool)
    with np.errstate(over="ignore", invalid="ignore"):
        for s in range(n_seg):
            q = 0.0
            for c in chunks[seg_chunk0[s]:seg_chunk0[s + 1]]:
                first, length = int(c["first"]), int(c["length"])
                if first < 0 or length <= 0 or length > GRAD_NORM_CHUNK or first + length > len(grad):
                    continue
                x = grad[first:first + length]
                q += float(_chunk_sqsum_f32(x, aligned=first % 4 == 0))       # (the flat vector itself starts on a 16-byte boundary)
                counted[s] |= bool(np.any(x != 0))
            seg_norm[s] = np.float32(np.sqrt(q) * mul)
        v = seg_norm[counted]
        stats = np.zeros(4, np.float32)
        if len(v):
            stats[0] = np.float32(np.sum(v.astype(np.float64)) / len(v))
            stats[1] = np.float32(np.nan) if np.isnan(v).any() else v.max()
        stats[2], stats[3] = len(v), np.count_nonzero(~np.isfinite(v))
    return seg_norm, stats


class GradStats:
    """device half of `GCPTrainStep.gradient_stats()`: the tables of one model, uploaded once, and the buffers of the launch"""

    def __init__(self, model):
        import torch
        self.names, chunks, seg_chunk0 = grad_tables(model._poff)
        dev = model.device
        self.n_chunks, self.n_seg = len(chunks), len(self.names)
        self.chunks = torch.from_numpy(chunks.view(np.uint8).copy()).to(dev)
        self.seg_chunk0 = torch.from_numpy(seg_chunk0).to(dev)
        self.partial = torch.empty(2 * self.n_chunks, device=dev)
        self.seg_norm = torch.empty(self.n_seg, device=dev)
        self.stats = torch.empty(4, device=dev)

    def launch(self, lib, grad, grad_scale, clip_coef_ptr, stream):
        from . import runtime as rt
        rt.check(lib.gcpx_grad_segment_norms(grad.data_ptr(), grad.numel(), self.chunks.data_ptr(), self.n_chunks,
                                             self.seg_chunk0.data_ptr(), self.n_seg, float(grad_scale), clip_coef_ptr,
                                             self.partial.data_ptr(), self.partial.numel(), self.seg_norm.data_ptr(),
                                             self.stats.data_ptr(), stream), "grad_segment_norms")
        return self.seg_norm, self.stats


# ---- the layer-wise KL (tree_module.py:159-169) ----
def kl_layerwise(model, outputs):
    """[L] device floats: per tree level, the mean over (sequence, node of the level) of the non-zero per-node KL means of the
    posterior forward `outputs` -- one gcpx_kl_layerwise on the caller's stream, buffers cached on the model"""
    import torch
    from . import runtime as rt
    from .plan_ops import _addr
    hp, o = model._hp, outputs.raw
    L, nv = hp.hierarchy_levels, hp.nz_vae
    QZ, PZ = o["QZ"], o["PZ"]
    B, PS = QZ.shape[:2]
    assert PS == 2 ** L + 1 and QZ.shape[2] == 2 * nv and QZ.is_contiguous() and PZ.is_contiguous()
    bufs = model.__dict__.setdefault("_kl_layerwise_bufs", {})
    if B not in bufs:
        bufs[B] = (torch.empty(B * (2 ** L - 1), device=model.device), torch.empty(L, device=model.device))
    node_v, out = bufs[B]
    # node n of the depth-first order sits in slot 1 + n of a sequence's PS slots (forward_plan.py: kl_args)
    rt.check(model.lib.gcpx_kl_layerwise(_addr(QZ, 2 * nv), _addr(PZ, 2 * nv), B, L, nv, PS * 2 * nv, 2 * nv, float(hp.free_nats),
                                         node_v.data_ptr(), out.data_ptr(), torch.cuda.current_stream(model.device).cuda_stream),
             "kl_layerwise")
    return out


def log_scalars(model, outputs, losses, step, phase, layerwise=False):
    """the scalar half of `model.log_outputs` (base_model.py:104-108, tree_module.py:159-169): every entry of `losses` as
    `<name>_loss`, the total as `total_loss`, and (tree model, phase train / val) `kl_loss_layerwise/level_<l>`.  Values may be device
    scalars or numbers: the device ones travel in ONE copy."""
    import torch
    log = model.scalar_log
    if log is None or losses is None:
        return
    items = [("total" if k in ("_total", "total") else k, (v.value if isinstance(v, dict) else v)) for k, v in losses.items()]
    if layerwise and phase in ("train", "val") and outputs is not None and "QZ" in outputs.raw and "losses" in outputs.raw:
        kl = kl_layerwise(model, outputs)
        items += [("kl_loss_layerwise/level_{}".format(l), kl[l]) for l in range(kl.numel())]
    on_dev = [i for i, (_, v) in enumerate(items) if torch.is_tensor(v)]
    if on_dev:
        host = torch.stack([items[i][1].detach().reshape(()).to(model.device, torch.float32) for i in on_dev]).cpu()
        for j, i in enumerate(on_dev):
            items[i] = (items[i][0], float(host[j]))
    for name, v in items:
        log.log_scalar(v, name if name.startswith("kl_loss_layerwise/") else name + "_loss", step, phase)
    log.flush()
