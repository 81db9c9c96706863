"""Evaluation harness on the device: alignment of predictions to ground truth, image metrics, top-of-100 evaluation.

Counterparts (paths relative to /root/reference):
  DTWEvalBinding / BalancedEvalBinding / BalancedPrunedDTWBinding     gcp/evaluation/evaluation_matching.py:123-221
  TreeDenseRec.get_sample_with_len / get_all_samples_with_len          gcp/prediction/models/tree/tree_dense_rec.py:13-40
  Evaluator.eval / eval_single / compute_metrics / _get_best_idxs      gcp/evaluation/compute_metrics.py:49-141,236-250
The reference walks the batch on the host (numpy / Cython DTW per sequence, skimage metrics per frame); here a whole batch is
aligned and scored by a handful of launches: image cost matrix (gcpx_cdist, f32 MFMA), DTW wavefront + traceback
(gcpx_dtw_align, float64), per-frame squared error + SSIM map (gcpx_image_metrics).

Metric spec (blox.torch.evaluation is absent — this build's written spec, restated in oracle/metrics_oracle.py): mse over the
[-1, 1] images; psnr = mean over frames of 10 log10(1 / mse_frame) on the [0, 1]-scaled images; ssim = mean over frames and
channels of the 7x7 uniform-window SSIM map (K1 = .01, K2 = .03, data range 1, sample covariance: skimage's defaults).

The alignment below is the counterpart of the reference's
`DTWEvalBinding` (/root/reference/gcp/evaluation/evaluation_matching.py:123-146), which `TreeDenseRec.get_sample_with_len`
(tree_dense_rec.py:13-30) and `Evaluator.eval_single` (compute_metrics.py:89-120) call per sequence on the host with
numpy / Cython DTW (dtw_utils.py:77-115, cutils.pyx).  Here the whole batch is aligned by three launches: image cost
matrix (gcpx_cdist, f32 MFMA), DTW wavefront + traceback (gcpx_dtw_align, float64), gather of the chosen frames.

Also here: the flat model's binding (SequentialRecModule.get_sample_with_len, prediction/models/sequential.py:70-97), the top-of-N
bookkeeping on the device (gcpx_topn_accumulate), the gather of the ranks' shards and the results writer (FileEvalLogger,
dump_metrics, dump_seqs; compute_metrics.py:184-226,327-350) that train.py --metric / --skip_top100_val 0 use."""
import os

import torch

from . import runtime as rt


class DTWEvalBinding:
    def __init__(self, model):
        self.m = model
        self.lib = model.lib

    def __call__(self, outputs, inputs, length, i_ex, targets=None, estimates=None):
        seqs, info = self.get_all_samples(outputs, inputs)
        return seqs[i_ex], info

    def get_all_samples(self, outputs, inputs, estimates=None, est_len=None):
        """estimates: [B, N, 3, H, W] (default: every tree node, depth-first = `_collect_sequence`); targets: traj_seq up to
        end_ind.  Returns (list of gen_images [len_b, 3, H, W], Outputs(inds, dist, path, path_len, acc))."""
        est, t_len, info = self.align(outputs, inputs, estimates, est_len)
        B, N = est.shape[:2]
        T = inputs["traj_seq"].shape[1]
        D = est[0, 0].numel()
        gen = torch.empty((B, T) + tuple(est.shape[2:]), device=est.device)
        rt.check(self.lib.gcpx_gather_rows(est.data_ptr(), info.inds.data_ptr(), gen.data_ptr(), B, T, N, 0, D,
                                           torch.cuda.current_stream(est.device).cuda_stream), "gather")
        lens = t_len.tolist()
        return [gen[b, :lens[b]] for b in range(B)], info

    def align(self, outputs, inputs, estimates=None, est_len=None):
        """the device part of get_all_samples: (estimates [B, N, ...], t_len int32 [B], Outputs(inds, dist, path, path_len, acc, cost,
        pool, pool_rows)) without gathering the frames and without a host sync"""
        m, lib = self.m, self.lib
        est = (outputs.images_df if estimates is None else estimates).contiguous()
        tgt = inputs["traj_seq"].contiguous()
        B, N = est.shape[:2]
        T = tgt.shape[1]
        D = est[0, 0].numel()
        dev = est.device
        st = torch.cuda.current_stream(dev).cuda_stream
        ns = lib.gcpx_cdist_splits(D)
        part = torch.empty(ns, B, N, T, device=dev)
        xn, yn, dsum = torch.empty(B * N, device=dev), torch.empty(B * T, device=dev), torch.empty(B, N, T, device=dev)
        rt.check(lib.gcpx_cdist(est.data_ptr(), tgt.data_ptr(), B, N, T, D, part.data_ptr(), xn.data_ptr(), yn.data_ptr(),
                                dsum.data_ptr(), st), "cdist")
        cost = dsum / float(D)                                   # cdist(..., reduction='mean') (evaluation_matching.py:135)
        t_len = (inputs["end_ind"] + 1).to(torch.int32)
        acc = torch.empty(B, N, T, dtype=torch.float64, device=dev)
        inds = torch.empty(B, T, dtype=torch.int32, device=dev)
        path = torch.empty(B, 2, N + T, dtype=torch.int32, device=dev)
        plen = torch.empty(B, dtype=torch.int32, device=dev)
        dist = torch.empty(B, dtype=torch.float64, device=dev)
        n_len = est_len.to(torch.int32).contiguous() if est_len is not None else None
        rt.check(lib.gcpx_dtw_align(cost.data_ptr(), rt.ptr(n_len), t_len.data_ptr(), B, N, T, acc.data_ptr(), inds.data_ptr(),
                                    path.data_ptr(), plen.data_ptr(), dist.data_ptr(), st), "dtw_align")
        from .model import Outputs
        return est, t_len, Outputs(inds=inds, dist=dist, path=path, path_len=plen, acc=acc, cost=cost,
                                   pool=est.reshape(B * N, *est.shape[2:]), pool_rows=N)


def mse_cropped(gen_list, inputs):
    """Evaluator.eval_single / compute_metrics (compute_metrics.py:96-101,123-130): first and last frame are conditioning
    frames and are cropped; mse over what remains.  Returns a list of floats (host), one per sequence."""
    out = []
    for b, g in enumerate(gen_list):
        tgt = inputs["traj_seq"][b, :g.shape[0]]
        out.append(float(((g[1:-1] - tgt[1:-1]) ** 2).mean()) if g.shape[0] > 2 else float("nan"))
    return out


class BalancedEvalBinding:
    """evaluation_matching.py:180-206: the nodes a balanced tree of the sequence's length keeps (c_n_prime non-zero), in temporal
    order — what the forward already leaves in `pruned_padded` / `model_enc_seq_padded`."""

    def __init__(self, model):
        self.m = model

    def get_all_samples(self, outputs, inputs=None, length=None, name=None):
        o = outputs.raw
        lens = o["pruned_len" if "pruned_len" in o else "seq_len"].tolist()
        name = "images" if name is None else name
        if name == "images":
            src = o["pruned_padded"]
        elif name in ("e_g_prime", "encodings"):
            src = o["model_enc_seq_padded"]
        else:
            raise KeyError(name)
        return [src[b, :lens[b]] for b in range(len(lens))], None

    def __call__(self, outputs, inputs, length, i_ex, name=None):
        seqs, _ = self.get_all_samples(outputs, inputs, length, name)
        return seqs[i_ex], None


class BalancedPrunedDTWBinding:
    """evaluation_matching.py:209-221: prune with the balanced binding, then warp the pruned sequence onto the ground truth"""

    def __init__(self, model):
        self.m = model
        self.dtw = DTWEvalBinding(model)

    def get_all_samples(self, outputs, inputs, length=None, name=None):
        o = outputs.raw
        est = o["pruned_padded"]                               # [B, T, 3, H, W], rows >= pruned length are zero
        n_len = o["pruned_len" if "pruned_len" in o else "seq_len"]
        return self.dtw.get_all_samples(outputs, inputs, estimates=est, est_len=n_len)

    def __call__(self, outputs, inputs, length, i_ex, name=None):
        seqs, info = self.get_all_samples(outputs, inputs, length, name)
        return seqs[i_ex], info


class SequentialEvalBinding:
    """SequentialRecModule.get_sample_with_len (prediction/models/sequential.py:70-97) of the flat model, as frame maps into its
    output frames `dense_rec.images` [B, T, C, H, W] (frame 0 is I_0, sequential.py:57):
      'basic': images[:, :end_ind + 1] — target frame t is output frame t;
      'dtw':   output frames 1..end_ind warped onto target frames 1..end_ind (gcpx_cdist, gcpx_dtw_align), then output frame 1 put in
               front.  Index 1, not 0, is what the reference prepends (`outputs.dense_rec.images[i_ex, [1]]`, sequential.py:86): it
               stands in for the ground-truth frame 0 that the DTW left out, and the crop of the first frame drops it before scoring.
    There is no tree, so no 'pruned_dtw' (the reference's method returns None for it)."""

    def __init__(self, model, pruning_scheme):
        if pruning_scheme not in ("dtw", "basic"):
            raise ValueError("Eval pruning scheme {} not supported by the sequential model!".format(pruning_scheme))
        self.m, self.lib, self.scheme = model, model.lib, pruning_scheme

    def frame_map(self, outputs, inputs):
        """(pool [B*T, C, H, W], fmap int32 [B, T]: pool row of the frame the prediction shows at target frame t)"""
        img = outputs.dense_rec.images
        tgt = inputs["traj_seq"]
        B, T = tgt.shape[:2]
        dev = tgt.device
        rows = torch.arange(B, device=dev, dtype=torch.int32)[:, None] * T
        pool = img.reshape(B * T, *img.shape[2:])
        if self.scheme == "basic":
            return pool, (rows + torch.arange(T, device=dev, dtype=torch.int32)[None]).contiguous()
        lib = self.lib
        D = tgt[0, 0].numel()
        st = torch.cuda.current_stream(dev).cuda_stream
        ns = lib.gcpx_cdist_splits(D)
        part = torch.empty(ns, B, T, T, device=dev)
        xn, yn, dsum = torch.empty(B * T, device=dev), torch.empty(B * T, device=dev), torch.empty(B, T, T, device=dev)
        est = img.contiguous()
        rt.check(lib.gcpx_cdist(est.data_ptr(), tgt.contiguous().data_ptr(), B, T, T, D, part.data_ptr(), xn.data_ptr(), yn.data_ptr(),
                                dsum.data_ptr(), st), "cdist")
        cost = dsum[:, 1:, 1:] / float(D)                       # estimates[1:end+1] vs targets[1:end+1], 'mean' reduction
        n = torch.clamp(inputs["end_ind"], min=1).to(torch.int32).contiguous()     # end_ind frames on either side
        acc = torch.empty(B, T - 1, T - 1, dtype=torch.float64, device=dev)
        inds = torch.empty(B, T - 1, dtype=torch.int32, device=dev)
        path = torch.empty(B, 2, 2 * (T - 1), dtype=torch.int32, device=dev)
        plen = torch.empty(B, dtype=torch.int32, device=dev)
        dist = torch.empty(B, dtype=torch.float64, device=dev)
        rt.check(lib.gcpx_dtw_align(cost.data_ptr(), n.data_ptr(), n.data_ptr(), B, T - 1, T - 1, acc.data_ptr(), inds.data_ptr(),
                                    path.data_ptr(), plen.data_ptr(), dist.data_ptr(), st), "dtw_align")
        fmap = torch.empty(B, T, dtype=torch.int32, device=dev)
        fmap[:, :1] = rows + 1                                  # the prepended images[:, 1]
        fmap[:, 1:] = torch.where(inds >= 0, rows + 1 + inds, torch.full_like(inds, -1))
        return pool, fmap

    def get_all_samples(self, outputs, inputs):
        """get_all_samples_with_len (sequential.py:95-97) at the ground-truth lengths: list of [end_ind + 1, C, H, W]"""
        pool, fmap = self.frame_map(outputs, inputs)
        lens = (inputs["end_ind"] + 1).tolist()
        return [pool[fmap[b, :lens[b]].long()] for b in range(len(lens))], None


def get_eval_binding(model, pruning_scheme):
    """TreeDenseRec._get_eval_binding (tree_dense_rec.py:32-40); the flat model's SequentialRecModule (sequential.py:70-97)"""
    from .sequential import GCPSequentialModel
    if isinstance(model, GCPSequentialModel):
        return SequentialEvalBinding(model, pruning_scheme)
    if pruning_scheme == "dtw":
        return DTWEvalBinding(model)
    if pruning_scheme in ("pruned_dtw", "basic"):
        assert model._hp.matching_type == "balanced"
        return BalancedPrunedDTWBinding(model) if pruning_scheme == "pruned_dtw" else BalancedEvalBinding(model)
    raise ValueError("Eval pruning scheme {} not currently supported!".format(pruning_scheme))


def image_metrics(model, est_pool, frame_map, tgt, first, last):
    """(mse, psnr, ssim) per sequence, float32 [B, 3] on the device.  tgt [B,T,C,H,W]; est_pool [R,C,H,W]; frame_map int32 [B,T]
    (pool frame matched to target frame (b, t), negative = none); frames t in [first[b], last[b]) are averaged."""
    B, T, C, H, W = tgt.shape
    dev = tgt.device
    scratch = torch.empty(2 * B * T * C, dtype=torch.float64, device=dev)
    out = torch.empty(B, 3, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    rt.check(model.lib.gcpx_image_metrics(est_pool.contiguous().data_ptr(), tgt.contiguous().data_ptr(), rt.ptr(frame_map),
                                          first.data_ptr(), last.data_ptr(), B, T, C, H, W, scratch.data_ptr(), out.data_ptr(), st),
             "image_metrics")
    return out


METRICS = ("mse", "psnr", "ssim")
SEQ_KEYS = ("gt_seq", "gen_images", "full_gen_seq")      # dump_seqs (compute_metrics.py:184-206)


class _Aligned:
    """one prediction aligned with the targets: target frame t of sequence b is pool row fmap[b, t], scored for first <= t < last;
    full_* = every frame of the prediction (the tree's nodes depth-first, compute_metrics.py:125-127), None for the flat model"""

    def __init__(self, pool, fmap, first, last, full_pool=None, full_rows=0):
        self.pool, self.fmap, self.first, self.last = pool, fmap, first, last
        self.full_pool, self.full_rows = full_pool, full_rows


class Evaluator:
    """compute_metrics.py:49-141: metrics of the prediction against the ground truth, optionally the best of `top_of`
    prior samples per sequence (`top_of_100_eval`).  Everything per-sample stays on the device: every sample is aligned and scored,
    and gcpx_topn_accumulate records its metrics, the best sample so far and that sample's frames; one device-to-host copy per batch.
    `eval` returns / accumulates [B, top_of] arrays of mse / psnr / ssim and the index of the best sample under `top_comp_metric`;
    the best sample's frames are kept in `seqs` (the arrays of dump_seqs)."""

    LOWER_IS_BETTER_METRICS = ["mse"]
    HIGHER_IS_BETTER_METRICS = ["psnr", "ssim"]

    def __init__(self, model, pruning_scheme="dtw", top_of_100=True, top_of=100, top_comp_metric="mse"):
        if top_comp_metric not in self.LOWER_IS_BETTER_METRICS + self.HIGHER_IS_BETTER_METRICS:
            raise ValueError("Currently only support comparison on the following metrics: {}. Got {}."
                             .format(self.LOWER_IS_BETTER_METRICS + self.HIGHER_IS_BETTER_METRICS, top_comp_metric))
        self.m = model
        self._binding = get_eval_binding(model, pruning_scheme)
        self._scheme = pruning_scheme
        self._top_of_100 = bool(top_of_100)
        self._top_of = top_of if top_of_100 else 1
        self._top_comp_metric = top_comp_metric
        self._full_maps = {}
        self.full_evaluation = None
        self.seqs = None

    def reset(self):
        self.full_evaluation = None
        self.seqs = None

    def _align(self, inputs, outputs):
        tgt = inputs["traj_seq"]
        B, T = tgt.shape[:2]
        dev = tgt.device
        end = inputs["end_ind"].to(torch.int32)
        first = torch.ones(B, dtype=torch.int32, device=dev)
        if isinstance(self._binding, SequentialEvalBinding):
            pool, fmap = self._binding.frame_map(outputs, inputs)
            return _Aligned(pool, fmap, first, end)            # input_seq[1:-1] against gen_seq[1:-1]: frames 1 .. end_ind - 1
        full = outputs.images_df                               # [B, n_nodes, C, H, W]
        if self._scheme == "basic":
            # BalancedEvalBinding returns the kept nodes in temporal order: frame t of the prediction is pruned row t
            o = outputs.raw
            est = o["pruned_padded"]
            n_len = o["pruned_len" if "pruned_len" in o else "seq_len"].to(torch.int32)
            fmap = (torch.arange(B, device=dev, dtype=torch.int32)[:, None] * est.shape[1] +
                    torch.arange(T, device=dev, dtype=torch.int32)[None]).contiguous()
            last = torch.minimum(end, n_len - 1)               # input_seq[1:-1] against gen_seq[1:-1]
            pool = est.reshape(-1, *est.shape[2:])
        else:
            if self._scheme == "pruned_dtw":
                o = outputs.raw
                _, _, info = self._binding.dtw.align(outputs, inputs, estimates=o["pruned_padded"],
                                                     est_len=o["pruned_len" if "pruned_len" in o else "seq_len"])
            else:
                _, _, info = self._binding.align(outputs, inputs)
            pool, N = info.pool, info.pool_rows
            fmap = (torch.arange(B, device=dev, dtype=torch.int32)[:, None] * N + info.inds).to(torch.int32)
            fmap = torch.where(info.inds >= 0, fmap, torch.full_like(fmap, -1)).contiguous()
            last = end                                         # frames 1 .. end_ind - 1
        return _Aligned(pool, fmap, first, last, full.contiguous().reshape(-1, *full.shape[2:]), full.shape[1])

    def eval_single(self, inputs, outputs):
        """metrics [B, 3] of one prediction (compute_metrics.py:89-130): align / prune, crop the two conditioning frames, score"""
        a = self._align(inputs, outputs)
        return image_metrics(self.m, a.pool, a.fmap, inputs["traj_seq"], a.first, a.last)

    def _is_better(self, a, b):
        return a < b if self._top_comp_metric in self.LOWER_IS_BETTER_METRICS else a > b

    def _full_map(self, B, F, dev):
        key = (B, F, str(dev))
        if key not in self._full_maps:
            self._full_maps[key] = torch.arange(B * F, device=dev, dtype=torch.int32)
        return self._full_maps[key]

    def eval(self, inputs, outputs=None, model=None, noises=None):
        """Evaluator.eval (compute_metrics.py:132-141): with top-of-N the model is re-run N times under the caller's val_mode
        (prior samples, train.py:205-210) and every sample is scored; `noises` (optional, [N, B, n_nodes, nz_vae]) fixes the draws.
        Returns dict(mse, psnr, ssim: [B, N] float32 on the host, best: [B] index of the best sample)."""
        import numpy as np
        model = model or self.m
        tgt = inputs["traj_seq"]
        B, T = tgt.shape[:2]
        D = tgt[0, 0].numel()
        N = self._top_of
        frame = tuple(tgt.shape[2:])
        comp = METRICS.index(self._top_comp_metric)
        lower = int(self._top_comp_metric in self.LOWER_IS_BETTER_METRICS)
        st = torch.cuda.current_stream(tgt.device).cuda_stream
        acc = None
        for n in range(N):
            if self._top_of_100 or outputs is None:
                outputs = model(inputs, "train", noise=None if noises is None else noises[n])
            a = self._align(inputs, outputs)
            vals = image_metrics(self.m, a.pool, a.fmap, tgt, a.first, a.last)
            if acc is None:
                F = a.full_rows
                acc = _BatchBuffer(B, N, T, F, D, tgt.device)
                full_map = self._full_map(B, F, tgt.device) if F else None
            rt.check(self.m.lib.gcpx_topn_accumulate(
                vals.data_ptr(), B, n, N, comp, lower, acc.all.data_ptr(), acc.best.data_ptr(),
                a.pool.data_ptr(), a.pool.shape[0], a.fmap.data_ptr(), a.first.data_ptr(), a.last.data_ptr(), T, acc.gen.data_ptr(),
                rt.ptr(a.full_pool), a.full_pool.shape[0] if F else 0, rt.ptr(full_map), F, rt.ptr(acc.full), D, st), "topn_accumulate")
        acc.gt.view((B, T - 1) + frame).copy_(tgt[:, 1:])     # dump_seqs' gt_seq: the frames after the conditioning frame
        acc.end.copy_(inputs["end_ind"].to(torch.int32))
        host = acc.buf.cpu()                                   # the only host transfer of the batch
        h = acc.views(host)
        all_ = h["all"].numpy()
        res = {"mse": all_[..., 0], "psnr": all_[..., 1], "ssim": all_[..., 2], "best": h["best"].numpy().astype(np.int64)}
        if self.full_evaluation is None:
            self.full_evaluation = {k: v.copy() for k, v in res.items()}
        else:
            for k in res:
                self.full_evaluation[k] = np.concatenate((self.full_evaluation[k], res[k]), 0)
        gen = h["gen"].numpy().reshape((B, T) + frame)[:, 1:]  # dump_seqs: gen_images[b, :len] = gen_seq (cropped), zeros after
        seqs = {"gt_seq": h["gt"].numpy().reshape((B, T - 1) + frame), "gen_images": gen, "end_ind": h["end"].numpy().copy()}
        if acc.F:
            seqs["full_gen_seq"] = h["full"].numpy().reshape((B, acc.F) + frame)
        if self.seqs is None:
            self.seqs = {k: [] for k in seqs}
        for k, v in seqs.items():
            self.seqs[k].append(v)
        return res

    def collected(self):
        """everything evaluated since the last reset, per sequence: mse / psnr / ssim [S, N], best [S], and the best samples' frames
        as dump_seqs stacks them (gt_seq, gen_images [S, T-1, C, H, W]; full_gen_seq: the tree's nodes, or gen_images cut to the longest
        cropped prediction for the flat model)"""
        import numpy as np
        if self.full_evaluation is None:
            return None
        out = {k: self.full_evaluation[k] for k in METRICS + ("best",)}
        seqs = {k: np.concatenate(v, 0) for k, v in self.seqs.items()}
        out["gt_seq"], out["gen_images"] = seqs["gt_seq"], seqs["gen_images"]
        if "full_gen_seq" in seqs:
            out["full_gen_seq"] = seqs["full_gen_seq"]
        else:                                                  # full_gen_seq = gen_seq (compute_metrics.py:125-127)
            out["full_gen_seq"] = seqs["gen_images"][:, :max(0, int(seqs["end_ind"].max()) - 1)]
        return out

    def _get_best_idxs(self, vals):
        import numpy as np
        return np.argmin(vals, 1) if self._top_comp_metric in self.LOWER_IS_BETTER_METRICS else np.argmax(vals, 1)

    def dump_metrics(self):
        """compute_metrics.py:214-226: per metric (mean, std of the best samples, mean per-sequence std over samples)"""
        import numpy as np
        out = {}
        best = self.full_evaluation["best"]
        for k in ("mse", "psnr", "ssim"):
            v = self.full_evaluation[k]
            bv = v[np.arange(v.shape[0]), best]
            out[k] = (float(bv.mean()), float(bv.std()), float(v.std(axis=1).mean()))
        return out


class _BatchBuffer:
    """the device arrays of one evaluated batch in ONE float32 allocation, so that one copy brings them to the host:
    all [B, N, 3], best int32 [B], end_ind int32 [B], gen [B, T, D] (best sample's aligned frames), full [B, F, D], gt [B, T-1, D]"""

    def __init__(self, B, N, T, F, D, device):
        self.F = F
        sizes = (("all", B * N * 3), ("best", B), ("end", B), ("gen", B * T * D), ("full", B * F * D), ("gt", B * (T - 1) * D))
        self.layout, o = [], 0
        for name, n in sizes:
            self.layout.append((name, o, n))
            o += (n + 63) // 64 * 64                           # 256-byte aligned views (the copy kernel moves float4)
        self.shapes = dict(all=(B, N, 3), best=(B,), end=(B,), gen=(B, T * D), full=(B, F * D), gt=(B, T - 1, D))
        self.buf = torch.empty(o, device=device)
        v = self.views(self.buf)
        self.all, self.best, self.end, self.gen, self.full, self.gt = (v[k] for k in ("all", "best", "end", "gen", "full", "gt"))
        if not F:
            self.full = None

    def views(self, buf):
        out = {}
        for name, o, n in self.layout:
            t = buf[o:o + n]
            if name in ("best", "end"):
                t = t.view(torch.int32)
            out[name] = t.view(self.shapes[name])
        return out


def _interleave(parts, batch_size):
    """rows of several ranks' arrays [n_batches * B, ...] in the order one process with batch W * B reads them (dataset.batch_schedule:
    global batch g = rank 0's B sequences of it, then rank 1's, ...)"""
    import numpy as np
    n = parts[0].shape[0]
    if any(p.shape[0] != n for p in parts) or n % batch_size:
        raise ValueError("every rank must have evaluated the same number of whole batches")
    blocks = [p[g * batch_size:(g + 1) * batch_size] for g in range(n // batch_size) for p in parts]
    return np.concatenate(blocks, 0) if blocks else parts[0]


def gather_evaluation(evaluation, batch_size, group=None):
    """data parallel (train.py): every rank evaluated its own shard; rank 0 receives all ranks' per-sequence arrays, in rank order
    within each global batch, i.e. the rows a single process evaluating the same sequences holds.  Other ranks get None.  Without a
    process group the input is returned."""
    d = torch.distributed
    if not (d.is_available() and d.is_initialized()) or d.get_world_size(group) == 1:
        return evaluation
    parts = [None] * d.get_world_size(group)
    d.all_gather_object(parts, evaluation, group=group)
    if d.get_rank(group) != 0:
        return None
    out = {k: _interleave([p[k] for p in parts], batch_size) for k in evaluation if k != "full_gen_seq"}
    if "full_gen_seq" in evaluation:
        # the flat model's full_gen_seq is as long as the longest prediction of its rank: pad to the longest over all ranks
        L = max(p["full_gen_seq"].shape[1] for p in parts)
        import numpy as np
        pad = [np.concatenate((p["full_gen_seq"], np.zeros((p["full_gen_seq"].shape[0], L - p["full_gen_seq"].shape[1]) +
                                                           p["full_gen_seq"].shape[2:], p["full_gen_seq"].dtype)), 1) for p in parts]
        out["full_gen_seq"] = _interleave(pad, batch_size)
    return out


def summary_lines(evaluation, top_of_100=True):
    """FileEvalLogger._log_metric / Evaluator.dump_metrics (compute_metrics.py:214-226,341-345): per metric in sorted order (mse, psnr,
    ssim) its line of results_<it>.txt, and the values of the comma-separated summary the reference prints.  Reductions in float64
    (the reference's buffers are float64 arrays, compute_metrics.py:69-78)."""
    import numpy as np
    best = np.asarray(evaluation["best"])
    lines, summary = [], []
    for name in sorted(k for k in evaluation if k in METRICS):
        vals = np.asarray(evaluation[name], dtype=np.float64)
        best_vals = vals[np.arange(vals.shape[0]), best]
        line = 'mean {} {}, standard error of the mean (SEM) {}'.format(name, best_vals.mean(), best_vals.std())
        line += ', mean std of 100 samples {}\n'.format(vals.std(axis=1).mean()) if top_of_100 else '\n'
        lines.append(line)
        summary.extend([best_vals.mean(), best_vals.std(), vals.std(axis=1).mean()])
    return lines, summary


def write_results(log_dir, it, evaluation, top_of_100=True):
    """Evaluator.dump_results with the FileEvalLogger (compute_metrics.py:143-150,184-226,327-350) into <log_dir>/metrics:
    results_<it>.txt (one line per metric, printed as well), then the reference's comma-separated summary on stdout; this build also
    writes results_<it>.npz (mse / psnr / ssim [S, N], best [S]).  The best samples' frames go where _log_array puts them:
    <metric dir>/<key>/it_<it>/<key>_0.npy for gt_seq, gen_images, full_gen_seq.  Returns the path of the .txt file."""
    import numpy as np
    d = os.path.join(log_dir, "metrics")
    os.makedirs(d, exist_ok=True)
    lines, summary = summary_lines(evaluation, top_of_100)
    path = os.path.join(d, "results_{}.txt".format(it))
    with open(path, "w") as f:
        for line in lines:
            f.write(line)
            print(line)
    print(*summary, sep=',')
    np.savez(os.path.join(d, "results_{}.npz".format(it)), **{k: np.asarray(evaluation[k]) for k in METRICS + ("best",)})
    for key in SEQ_KEYS:
        if key in evaluation:
            sub = os.path.join(d, key, "it_{}".format(it))
            os.makedirs(sub, exist_ok=True)
            np.save(os.path.join(sub, "{}_0.npy".format(key)), evaluation[key])
    return path
