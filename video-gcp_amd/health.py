"""Training guard: the reference's NanGradHook (base_trainer.py:20-66, wired at gcp_builder.py:99-103) and its NaN total loss check
(base_gcp.py:302-303), with the test and the "do not apply it" decision both on the device.

The reference reads every `p.grad` on the host between backward() and optimizer.step().  Here the gradient is one flat device vector
and the loop synchronises on logging steps only, so `gcpx_grad_health` (csrc/train_stats.hip) scans it through the chunk tables of the
gradient norms (scalar_log.grad_tables), counts NaN / +Inf / -Inf per parameter by bit pattern, and writes its verdict into slot 3 of
the optimizer state -- the gate every step kernel reads at entry (csrc/scalar_f32.hip).  A bad step is therefore a no-op on the device
whether or not the host ever looks (`nan_guard="skip"`), and the host that does look (`"raise"`) finds the weights untouched.

The module imports without a GPU: `health_numpy` restates the kernel in numpy and is its checker, as scalar_log.segment_norms_numpy is
the norms kernel's.
"""
import numpy as np

from .scalar_log import GRAD_NORM_CHUNK, grad_tables

SUMMARY_FIELDS = ("nan", "posinf", "neginf", "bad_segments", "first_bad", "extra_nonfinite", "verdict", "bad_calls")
EXP_MASK, ABS_MASK, POS_INF, NEG_INF = 0x7F800000, 0x7FFFFFFF, 0x7F800000, 0xFF800000


class NonFiniteGradients(ValueError):
    """nan_guard="raise": the step's gradient (or a loss term) holds NaN or +-Inf; the device has skipped the update.
    bad: [(parameter name, n_nan, n_posinf, n_neginf)], ok: the names of the others, loss_nonfinite: number of non-finite entries of
    the device loss vector, outputs: the forward outputs of the step."""

    def __init__(self, bad, ok, loss_nonfinite, outputs=None):
        super().__init__("there are NaN Gradients")                      # base_trainer.py:38
        self.bad, self.ok, self.loss_nonfinite, self.outputs = bad, ok, loss_nonfinite, outputs


class NonFiniteWeights(ValueError):
    """a checkpoint was about to be written from parameters or running statistics that hold NaN or +-Inf; `bad` as above"""

    def __init__(self, bad):
        super().__init__("non-finite weights: {}".format([b[0] for b in bad][:8]))
        self.bad = bad


def classify_bits(x):
    """(is_nan, is_posinf, is_neginf) of an f32 array from its bits: exponent all ones, mantissa non-zero / zero, the sign"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return (u & ABS_MASK) > EXP_MASK, u == POS_INF, u == NEG_INF


def health_numpy(x, chunks, seg_chunk0, extra=None, count0=0):
    """numpy restatement of gcpx_grad_health: (seg_bad [n_seg, 3] int32, summary [8] int32); count0: summary[7] before the call"""
    x = np.ascontiguousarray(x, np.float32)
    n_seg = len(seg_chunk0) - 1
    seg_bad = np.zeros((n_seg, 3), np.int32)
    for s in range(n_seg):
        for c in chunks[max(int(seg_chunk0[s]), 0):min(int(seg_chunk0[s + 1]), len(chunks))]:
            first, length = int(c["first"]), int(c["length"])
            if first < 0 or length <= 0 or length > GRAD_NORM_CHUNK or first + length > len(x):
                continue
            seg_bad[s] += [int(np.count_nonzero(k)) for k in classify_bits(x[first:first + length])]
    bad = np.nonzero(seg_bad.any(axis=1))[0]
    n_extra_bad = 0
    if extra is not None and len(extra):
        e = np.ascontiguousarray(extra, np.float32).view(np.uint32)
        n_extra_bad = int(np.count_nonzero((e & EXP_MASK) == EXP_MASK))
    verdict = int(len(bad) > 0 or n_extra_bad > 0)
    summary = np.array(list(seg_bad.sum(axis=0)) + [len(bad), bad[0] if len(bad) else -1, n_extra_bad, verdict, count0 + verdict],
                       np.int32)
    return seg_bad, summary


def bad_list(names, seg_bad):
    """([(name, n_nan, n_posinf, n_neginf)] of the segments with a count, the names of the others) from host counts"""
    seg_bad = np.asarray(seg_bad).reshape(len(names), 3)
    bad = [(names[s], int(seg_bad[s, 0]), int(seg_bad[s, 1]), int(seg_bad[s, 2])) for s in range(len(names)) if seg_bad[s].any()]
    hit = {b[0] for b in bad}
    return bad, [n for n in names if n not in hit]


class GradHealth:
    """device half of the guard, like scalar_log.GradStats: the tables of one model uploaded once, the buffers of the launch allocated
    once, and a 32-byte pinned host slot the summary is copied to.  buffers=True walks every entry of `_poff` (parameters and
    BatchNorm running statistics: the table for theta), False the parameters alone (the table for the gradient)."""

    def __init__(self, model, buffers=False):
        import torch
        self.names, chunks, seg_chunk0 = grad_tables(model._poff, buffers=buffers)
        dev = model.device
        self.n_chunks, self.n_seg = len(chunks), len(self.names)
        self.chunks = torch.from_numpy(chunks.view(np.uint8).copy()).to(dev)
        self.seg_chunk0 = torch.from_numpy(seg_chunk0).to(dev)
        self.partial = torch.empty(3 * self.n_chunks, dtype=torch.int32, device=dev)
        self.seg_bad = torch.zeros((self.n_seg, 3), dtype=torch.int32, device=dev)
        self.summary = torch.zeros(8, dtype=torch.int32, device=dev)           # ([7], the running count, is zeroed here and only here)
        self.host = torch.zeros(8, dtype=torch.int32).pin_memory()

    def launch(self, lib, x, extra, gate_ptr, stream):
        from . import runtime as rt
        rt.check(lib.gcpx_grad_health(x.data_ptr(), x.numel(), self.chunks.data_ptr(), self.n_chunks, self.seg_chunk0.data_ptr(),
                                      self.n_seg, rt.ptr(extra), 0 if extra is None else extra.numel(), self.partial.data_ptr(),
                                      self.partial.numel(), self.seg_bad.data_ptr(), self.summary.data_ptr(), gate_ptr, stream),
                 "grad_health")
        return self.seg_bad, self.summary

    def read_summary(self, stream):
        """the summary of the last launch on the host: one 32-byte copy into the pinned slot behind whatever `stream` (a
        torch.cuda.Stream) holds, then the wait for it"""
        import torch
        with torch.cuda.stream(stream):
            self.host.copy_(self.summary, non_blocking=True)
        stream.synchronize()
        return self.host.numpy().copy()

    def bad(self):
        """(bad, ok) name lists of the last launch (synchronises: for the path that has already found a verdict of 1)"""
        return bad_list(self.names, self.seg_bad.cpu().numpy())
