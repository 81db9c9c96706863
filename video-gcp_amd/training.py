"""Training step of the gcp_tree model on MI355X: forward + explicit backward + RAdam, all in HIP.

Mirrors the reference's inner loop (/root/reference/gcp/prediction/train.py:155-163):
    optimizer.zero_grad(); output = model(inputs); losses = model.loss(...); total = model.get_total_loss(...)
    total.value.backward(); optimizer.step()
with optimizer = RAdam(lr, betas=(adam_beta, 0.999)) (gcp_builder.py:88-89,178-179; gradient_clip defaults to None).

The reference leans on torch autograd; here the backward pass is a second recorded launch plan, generated from the
records the forward plan leaves behind (`plan.rec`), and replayed over the model's streams:
  * data gradients of Linear / Conv1d / ConvTranspose / strided-conv layers: gcpx_gemm with transposed weight packs;
    of the decoder's 3x3 convs: gcpx_conv3x3 with flipped + transposed packs;
  * weight gradients: gcpx_wgrad (f32 MFMA "TN" GEMM; convs as implicit im2col);
  * everything in between (LSTM cell, GroupNorm, BatchNorm, bilinear upsample, skips broadcast, interleave, sampling,
    losses): csrc/backward.hip.
Gradients land in ONE flat fp32 vector laid out like `model.theta` (so the data-parallel all-reduce is a single RCCL
call over one buffer) and the optimizer + the re-pack of the MFMA-ordered weights are one launch each.
"""
import ctypes as C
import os
import re
from contextlib import contextmanager

import torch

from . import packing as pk
from . import runtime as rt
from .plan_ops import _Plan, _addr, N_LANES
from .params import decoder_layers
from .backward_weights import BackwardWeightsMixin, _c16      # noqa: F401 (re-exported)
from .backward_ops import BackwardOpsMixin, _PtrHolder      # noqa: F401
from .backward_plan import BackwardPlanMixin
from .backward_stages import BackwardStagesMixin


def _numel(shape):
    n = 1
    for d in shape:
        n *= int(d)
    return n


class GCPTrainStep(BackwardWeightsMixin, BackwardOpsMixin, BackwardPlanMixin, BackwardStagesMixin):
    """`step(inputs)` = one optimisation step of `model` (GCPTreeModel) on one minibatch; `backward(inputs)` stops
    after the gradients (tests)."""

    OPTIMIZERS = {"radam": 0, "adam": 1, "rmsprop": 2, "sgd": 3}
    _early_on, _caller, last_bplan_caller_lane = False, None, False          # (see __init__: early_optimizer)
    _pending_slices = ()
    accumulate, micro_index, stepped, _accumulating, _grad_div = 1, 0, False, False, 1      # (see __init__: accumulate)
    NAN_GUARDS = (None, "raise", "skip")
    ema, ema_decay, ema_warmup, ema_updates, _ema_swapped = None, None, True, 0, False      # (see __init__: ema_decay)

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, process_group=None, optimizer="radam", momentum=0.0,
                 gradient_clip=None, nan_guard=None, accumulate=1, ema_decay=None, ema_warmup=True):
        """optimizer / momentum / gradient_clip: the trainer's `optimizer` ('radam' default, 'adam', 'rmsprop', 'sgd'), `momentum`
        (RMSprop / SGD) and `gradient_clip` settings (gcp_builder.py:174-186,255-263).
        nan_guard: None (nothing is tested: the step as it always was), "raise" or "skip" -- the reference's NanGradHook
        (base_trainer.py:20-66) as a device kernel between the backward and the optimizer (health.py): one gcpx_grad_health over the
        whole (all-reduced) gradient and the loss vector writes the gate of the optimizer state, and the step kernels and the tick
        return at entry when it is closed.  "raise": step() then reads the 32-byte summary and raises NonFiniteGradients; "skip": no
        sync, training goes on, health() holds the counts.  Either way a non-finite gradient never reaches theta or the moments.
        accumulate: k > 1 makes `step()` one MICRO-step of a cycle of k (gradient accumulation, no reference counterpart: the k
        micro-batches stand for the k replicas of nn.DataParallel, gcp_builder.py:71-78, each with its own BatchNorm statistics).  Micro-
        steps 1 .. k-1 run forward + backward and fold self.grad into a second flat vector (gcpx_grad_accumulate: assign on the first,
        add afterwards) -- no optimizer, re-pack, tick, clip norm, health launch or collective; micro-step k adds that vector into
        self.grad and runs the optimizer path as it stands with grad_scale = 1 / (k world).  The early optimizer slices and the overlap
        of the bucket all-reduces with the backward are off for k > 1 (as under gradient_clip: they need the cycle's whole sum).
        `micro_index`: position in the cycle; `stepped`: whether the last step() applied the optimizer; `mean_losses()`: the loss vector's
        mean over the cycle.  1: the step as it always was -- no buffer, no launch.
        ema_decay: a float in (0, 1) keeps an exponential moving average of theta -- parameters AND BatchNorm running statistics, one flat
        vector `self.ema`, started as a copy of theta -- moved by one gcpx_ema_update per OPTIMIZER step, on the caller's stream behind
        the step's last write to theta, gated like the step (a step the nan_guard drops leaves the average where it was).  The decay of
        update t (0-based, t = `ema_updates`, a host count of ISSUED updates: the host never reads the gate, so a dropped step advances
        it all the same) is `ema_decay`, or with ema_warmup (default) min(ema_decay, (1 + t) / (10 + t)) -- the num_updates rule of
        TensorFlow's ExponentialMovingAverage, which keeps the random initialisation from dominating the first 1 / (1 - decay) steps.
        `with trainer.ema_weights():` runs its body on the averaged weights.  None: the trainer as it was -- no vector, no launch."""
        if int(accumulate) != accumulate or int(accumulate) < 1:
            raise ValueError("accumulate must be a positive number of micro-batches, not {!r}".format(accumulate))
        self.accumulate, self.micro_index, self.stepped = int(accumulate), 0, False
        self._accumulating, self._grad_div, self._acc, self._loss_acc = False, 1, None, None
        if optimizer not in self.OPTIMIZERS:
            raise ValueError("Optimizer '{}' not supported!".format(optimizer))          # gcp_builder.py:185
        if ema_decay is not None and not 0.0 < float(ema_decay) < 1.0:
            raise ValueError("ema_decay must be None or lie in (0, 1), not {!r}".format(ema_decay))
        if nan_guard not in self.NAN_GUARDS:
            raise ValueError("nan_guard must be None, 'raise' or 'skip', not {!r}".format(nan_guard))
        self.nan_guard, self._health, self._health_extra = nan_guard, None, None
        self.optimizer, self.momentum, self.gradient_clip = optimizer, float(momentum), gradient_clip
        self._clip_state_dirty, self._clip_part = True, None      # the clip coefficient slot of the optimizer state / its scratch
        hp = model._hp
        if hp.decoder_distribution == "gaussian" and hp.adaptive:
            # (the averaging criterion's image gradient would have to go through tanh instead of through the mixture mean)
            raise ValueError(f"training the adaptive (matching_type='{hp.matching_type}') model with decoder_distribution='gaussian' is not built: "
                             "its backward takes the image gradient through the mixture mean of the discrete_logistic_mixture head")
        self.m = model
        self.lr, self.betas, self.eps = lr, betas, eps
        self.pg = process_group
        model.train()
        model.save_for_backward = True
        self.grad = torch.zeros_like(model.theta)
        self.exp_avg = torch.zeros_like(model.theta)
        self.exp_avg_sq = torch.zeros_like(model.theta)
        self.opt_state = torch.zeros(4, device=model.device)
        if self.accumulate > 1:
            self._acc = torch.zeros_like(model.theta)          # the sum of the cycle's earlier micro-gradients
            self._loss_acc = torch.zeros(16, device=model.device)          # ... and of its loss vectors (out.raw["losses"])
        if ema_decay is not None:
            self.ema_decay, self.ema_warmup, self.ema_updates, self._ema_swapped = float(ema_decay), bool(ema_warmup), 0, False
            self.ema = model.theta.clone()
        from .dist import GradBuckets, gradient_bucket_ranges
        ranges = gradient_bucket_ranges(model._poff, hp.hierarchy_levels, hp.untied_layers)
        self._ranges = ranges
        self._bucket_index = {name: i for i, (name, _, _) in enumerate(ranges)}
        self.buckets = GradBuckets(self.grad, ranges, process_group) if process_group is not None else None
        # step(): the optimizer update of a tree level's slice (+ the re-pack of its weights) is issued on the CALLER's stream — idle
        # while the backward plan runs on the model's lanes — as soon as the backward reports the slice final (and, data-parallel, its
        # all-reduce is done): the 7 levels' 10.3 M parameters each (c2) are updated under the remaining levels and the encoder
        # backward, instead of 2.9 GB of optimizer + re-pack traffic behind the last gradient.  Not with gradient_clip (the global norm
        # needs every slice).  backward() alone never touches parameters.
        # Issued at a level's mark, a full grid of the optimizer kernel stretched the tree chain's GEMMs beside it from 41 to 101 us
        # (profiles/r04n_train_timeline.txt) and took back 0.4 of the 0.58 ms; with the levels' merge chains on the caller's stream
        # (merge_on_caller_lane) the slices are held until the last chain is out and run under the encoder backward (_on_mark): -0.24 ms
        # per step (tools/ab_train_attr.py early_optimizer 1 0).  `early_blocks` > 0 holds their launches to that many workgroups
        # (one workgroup per CU, 256, is the default since round 6: -0.1 ms against full grids; 128: +0.3 ms, 64: +1.6).
        self.early_optimizer = os.environ.get("GCPX_NO_EARLY_OPTIMIZER") is None
        self.early_blocks = int(os.environ.get("GCPX_EARLY_BLOCKS", "256"))     # (round 6 sweep: 0 = full grids 12.00 ms, 64: 13.6, 128: 12.3, 256: 11.90, 512: 11.96)
        self._early_on, self._applied, self._caller = False, set(), None
        self.split_dgrad_wide = os.environ.get("GCPX_NO_SPLIT_DGRAD_WIDE") is None     # data gradients of the 32- / 64-channel decoder blocks on the split-f16 kernel
        self.bk = model.build_arena(self._pack_backward)
        self._pack_backward_split()
        self._live_gemm_split()
        self._bplans = {}
        # backward plans are built from forward plans: drop them whenever the model drops those (load_state_dict, build_arena)
        model._plan_listeners = model._plan_listeners + [self._drop_bplans]
        self.wgroup_min_blocks = int(os.environ.get("GCPX_WGROUP_MIN", "256"))
        self.fused_image_wgrad = os.environ.get("GCPX_IMAGE_WGRAD_UNFUSED") is None
        self.split_wgrad = os.environ.get("GCPX_WGRAD_NOSPLIT") is None     # decoder conv weight gradients on the split-f16 kernel
        self.wgrad_per_cu = int(os.environ.get("GCPX_WGRAD_PER_CU", "1"))         # conv weight gradients: workgroups per CU (0: the kernel's own occupancy)
        self.lean_mean_grad = os.environ.get("GCPX_NO_LEAN_MEAN_GRAD") is None   # adaptive: head backward over the 80 slots of the mixture mean
        self.fuse_stage = os.environ.get("GCPX_NO_STAGE_FUSION") is None     # 16-channel upsampling blocks: weight gradient without gcpx_conv_stage
        self.fuse_head_act = os.environ.get("GCPX_NO_HEAD_ACT_FUSION") is None     # activation backward of the last decoder block in the head's data gradient
        self.fuse_skip = os.environ.get("GCPX_NO_SKIP_FUSION") is None             # skip-connection sum of a 16 + 16 channel block in the activation pass in front of it
        self.split_wgrad_rows = os.environ.get("GCPX_WGRAD_ROWS_NOSPLIT") is None   # the tree's Linear / LSTM weight gradients (>= 256 rows) likewise
        # The parent-state merge chain of a level (batched d h_prev GEMM -> merge data gradient -> accumulation into the parents' states:
        # three dependent launches that only the NEXT level's LSTM backward waits for) runs on the CALLER's stream as a fourth lane — idle
        # during the backward, with a hardware queue of its own (a fifth stream would share one of the four) — beside the level's
        # embedding / latent / Predictor chain on lane 0
        self.merge_on_caller_lane = os.environ.get("GCPX_NO_MERGE_LANE") is None
        self.zero_on_side_lane = os.environ.get("GCPX_ZERO_ON_LANE0") is None
        self.heads_on_side_lane = os.environ.get("GCPX_NO_HEADS_ASIDE") is None

        self.batch_dh = os.environ.get("GCPX_NO_BATCH_DH") is None                 # a level's d h_prev GEMMs as one batched launch
        self.group_mlp_bwd = os.environ.get("GCPX_NO_MLP_BWD_GROUP") is None       # a level's posterior + prior backward as one launch
        self.fused_mlp_bwd = os.environ.get("GCPX_NO_FUSED_MLP_BWD") is None
        # one attention head through gcpx_attention_bwd_heads too (same bits as gcpx_attention_bwd: tests/test_gpu_attention_layers.py)
        self.attn_bwd_heads_export = os.environ.get("GCPX_ATTN_BWD_HEADS") is not None
        self._pad_fixups = []                 # (see _mlp_in_dst)
        # the decoder's weight gradients (5 ms of throughput-bound kernels) are forked after the decoder's data-gradient chain: they then
        # fill the chip during the latency-bound tree phase instead of competing with the data gradients (23.2 -> 22.8 ms / step)
        self.defer_decoder_side = os.environ.get("GCPX_NO_DEFER_DEC_SIDE") is None
        # ... and held back further, until the tree backward has passed its large levels: issued right behind the decoder's data
        # gradients they ran beside the level L-1 / L-2 GEMMs of the tree (1024 / 512 rows, throughput-bound) and stretched two of them
        # from ~0.1 to 1.5 ms each on the critical lane (profiles/r02f_train_lanes.txt); below those levels the tree backward is a
        # chain of small launches that leaves the chip to the weight gradients.  GCPX_DEC_SIDE_LEVEL = level after which they go out
        # (>= L: right after the decoder, the old behaviour).  Default L - 1: with the split-f16 weight gradients (3.4 instead of 7 ms of
        # side-lane kernels) holding them past the largest level only is best — same-box, c2: 16.8-17.2 ms / step against 17.3-17.4 (L - 2)
        # and 17.2-17.5 (L); c5: 22.0 against 22.4 / 22.3.
        # Round 3 (the tree's own weight gradients on the split-f16 kernel, 1.6 -> 1.2 ms of side-lane kernels per step): three runs each
        # on one box, c2: 15.36 ms (L - 1), 15.14 (L - 3), 15.12 (L - 4) — L - 3.
        self.dec_side_level = int(os.environ.get("GCPX_DEC_SIDE_LEVEL", str(max(0, hp.hierarchy_levels - 3))))
        self.group_wgrads = os.environ.get("GCPX_NO_WGROUP") is None   # one grouped launch per level and kernel variant
        self.side_lanes = bool(hp.untied_layers)   # tied levels accumulate into the same weights: keep them on one lane
        self.wgrad_waves = 8192               # wavefronts a split weight-gradient launch aims for (latency hiding)
        # The backward plan is replayed EAGERLY over real streams: as parallel branches of one hipGraph the runtime maps nodes of the
        # critical chain onto the same hardware queue as multi-millisecond weight-gradient kernels and serialises them (measured:
        # 32.0 ms / step as a graph, 28.0 ms eager, c2).
        # GCPX_BWD_SEGMENTS=n > 0: EVERY run of >= n consecutive launches on one lane is replayed as a small linear hipGraph
        # (plan_ops.compact); 0: only where the plan asks for it (rec["segment_ranges"]); -1: nowhere
        self.segment_graphs = int(os.environ.get("GCPX_BWD_SEGMENTS", "0"))
        self.n_side = int(os.environ.get("GCPX_NSIDE", N_LANES - 1))   # side lanes of the backward plan
        self._lanes = None
        self._lane_streams = None
        self._zeros = torch.zeros(256, device=model.device)

    # ------------------------------------------------------------------------------------------------
    # running
    # ------------------------------------------------------------------------------------------------
    def backward(self, inputs, noise=None):
        """forward (phase 'train', losses on device) + backward; gradients in self.grad.  Returns the forward outputs."""
        m = self.m
        self._refuse_on_ema_weights("backward()")
        if self.buckets is not None and not self._accumulating:
            self.buckets.begin()          # a backward without an optimizer step in between must exchange its buckets again
        self._grad_div = 1                # self.grad is one batch's gradient again (gradient_stats)
        out = m.forward(inputs, "train", noise)
        if "losses" not in out.raw:
            raise ValueError("the training step needs traj_seq and pad_mask")
        if self.nan_guard:
            self._health_extra = out.raw["losses"]        # the device loss vector: tested beside the gradient (base_gcp.py:302-303)
        fplan = m._plan_of(out.raw)
        bplan = self._bplans.get(fplan.key)
        if bplan is None:
            bplan = self._bplans[fplan.key] = self._build_backward(fplan)
        caller = torch.cuda.current_stream(m.device)
        self._caller = caller
        self._applied = set()
        self._pending_slices = []
        self.last_bplan_caller_lane = bool(bplan.rec.get("caller_lane"))
        m._stream.wait_stream(caller)
        # (the caller's stream is the plan's last lane: the levels' merge chains, and step()'s early optimizer slices behind them)
        lanes = self._backward_streams() + [caller.cuda_stream]
        ops = None
        seg_ranges = None if self.segment_graphs > 0 else bplan.rec.get("segment_ranges")
        if (self.segment_graphs > 0 or (seg_ranges and self.segment_graphs == 0)) and not bplan.rec.get("caller_lane"):
            # runs of launches on one lane as small linear graphs (fewer host calls; lanes, events and marks unchanged): everywhere
            # (GCPX_BWD_SEGMENTS=n) or where the plan asks for it (`segment_ranges`: chains with slack, GCPX_BWD_SEGMENTS=-1: nowhere)
            if bplan.segments is None:
                bplan.run(lanes, on_mark=self._on_mark)
                torch.cuda.synchronize(m.device)
                bplan.compact(self._backward_streams(), max(self.segment_graphs, 3), seg_ranges)
                self.last_bplan = bplan
                caller.wait_stream(m._stream)
                return out
            ops = bplan.segments
        bplan.run(lanes, ops=ops, on_mark=self._on_mark)
        caller.wait_stream(m._stream)
        self.last_bplan = bplan
        return out

    def _drop_bplans(self):
        """the model's plan listener: behind model._clear_plans' device synchronise"""
        for bplan in self._bplans.values():
            bplan.close()
        self._bplans.clear()

    def _on_mark(self, tag, payload):
        if tag == "slices":
            self._issue_pending_slices()
            return
        if tag != "bucket" or (self.buckets is None and not self._early_on) or self._accumulating:
            return                        # (a micro-step of an accumulation cycle: the collectives run once, on the cycle's sum)
        if self._lane_streams is None:
            self._lane_streams = [torch.cuda.ExternalStream(int(s.value if hasattr(s, "value") else s), device=self.m.device)
                                  for s in self._backward_streams()]
        if self.buckets is not None:
            self.buckets.reduce_async(payload, after_streams=self._lane_streams)
        if self._early_on:
            if self.last_bplan_caller_lane:
                # The caller's stream also carries the levels' merge chains (merge_on_caller_lane): a slice issued here would wait for
                # the level's weight gradients on the side lanes and hold up the next level's merge chain behind it (measured: 15.0
                # instead of 13.2 ms / step).  Remember where the lanes stand (events) and issue the slices behind the last merge chain
                # (the plan's "slices" mark): they then run under the encoder backward.
                evs = []
                for s_ in self._lane_streams:
                    e = torch.cuda.Event()
                    e.record(s_)
                    evs.append(e)
                self._pending_slices.append((payload, evs))
                return
            # elsewhere: at once, on the caller's stream
            self._apply_slice(payload, tick=False, on=self._caller, after=self._lane_streams, max_blocks=self.early_blocks)
            self._applied.add(payload)

    def _issue_pending_slices(self):
        for i, evs in self._pending_slices:
            self._apply_slice(i, tick=False, on=self._caller, after=evs, max_blocks=self.early_blocks)
            self._applied.add(i)
        self._pending_slices = []

    def _apply_slice(self, i, tick, on, after=(), max_blocks=0):
        """optimizer update of slice i of the flat vectors + re-pack of the weights that gather from it, on stream `on` (which first
        waits for `after` — streams or events: the lanes that produce the slice's gradient — and for the slice's all-reduce)"""
        m = self.m
        name, lo, hi = self._ranges[i]
        caller = on
        for s in after:
            if isinstance(s, torch.cuda.Event):
                caller.wait_event(s)
            else:
                caller.wait_stream(s)
        scale = 1.0
        if self.buckets is not None and torch.distributed.is_initialized():
            w = self.buckets.works.get(i)
            if w is not None:
                with torch.cuda.stream(caller):
                    w.wait()                                   # the stream waits for the collective (no host block)
            scale = 1.0 / torch.distributed.get_world_size(self.buckets.group)
        kind = self.OPTIMIZERS[self.optimizer]
        p1, p2 = (self.betas[0], self.betas[1]) if kind <= 1 else ((self.momentum, 0.99) if kind == 2 else (self.momentum, 0.0))
        st = caller.cuda_stream
        o = 4 * lo
        rt.check(m.lib.gcpx_optim_range(m.theta.data_ptr() + o, self.grad.data_ptr() + o, self.exp_avg.data_ptr() + o,
                                        self.exp_avg_sq.data_ptr() + o, self.opt_state.data_ptr(), hi - lo, kind, self.lr, p1, p2, self.eps,
                                        scale, 1 if tick else 0, max_blocks, st), "optim_range")
        m.repack(st, bucket=name, max_blocks=max_blocks)

    def _backward_streams(self):
        """lane 0 = the model's stream, side lanes = the model's own side streams: the process then uses four streams in all
        (torch's, the model's three), one per hardware queue of the default runtime configuration — extra streams get
        multiplexed onto the same queues and serialise the lanes again (measured: +4 ms / step)."""
        if self._lanes is None:
            m = self.m
            self._lanes = list(m._streams[:1 + self.n_side])
            for _ in range(1 + self.n_side - len(self._lanes)):
                sp = C.c_void_p()
                with torch.cuda.device(m.device):
                    rt.check(m.lib.gcpx_stream_create_priority(C.byref(sp), 0), "stream_create")      # middle priority; lowest (> 0) starves the side lanes: 40.9 ms / step
                self._lanes.append(sp)
        return self._lanes

    def optimizer_step(self, outputs=None):
        """The configured optimizer (RAdam / Adam / RMSprop / SGD, optional clip_grad_norm_) on the flat vectors + one re-pack gather
        (gcp_builder.py:88-89,178-179).  Under a nan_guard the gradient's health check goes first and gates all of it; with
        nan_guard="raise" the call ends by reading the verdict (`outputs`: what the exception carries as .outputs)."""
        self._optimizer_step()
        if self.nan_guard == "raise":
            self._raise_if_bad(outputs)

    def _optimizer_step(self):
        m = self.m
        self._refuse_on_ema_weights("the optimizer step")
        st = torch.cuda.current_stream(m.device).cuda_stream
        scale = 1.0
        if self.buckets is not None:
            # the tree-level buckets were started during the backward; the last one (conv stacks, heads, level 0) goes now
            scale = self.buckets.finish()
        if self._grad_div > 1:
            scale = 1.0 / (self._grad_div * round(1.0 / scale))        # the mean over the cycle's micro-batches and the ranks
        if self.nan_guard:
            # the whole gradient is final here (data-parallel: the ranks' sum, the same bits on every rank, so every rank reaches the
            # same verdict without a further collective); the verdict lands in opt_state[3] before anything below reads it
            self._grad_health().launch(m.lib, self.grad, self._health_extra, self.opt_state.data_ptr() + 12, st)
        applied, self._applied = self._applied, set()
        if applied:
            # step(): those slices were updated during the backward; the others (at least "rest") follow here, the last one ticks
            assert self._caller is not None and self._caller.cuda_stream == st, "step() runs on one stream"
            if self._clip_state_dirty:
                self.opt_state[1:2].zero_()      # (ordered behind the early slices: they already read it — see step())
                self._clip_state_dirty = False
            todo = [i for i in range(len(self._ranges)) if i not in applied]
            for j, i in enumerate(todo):
                self._apply_slice(i, tick=(j == len(todo) - 1), on=self._caller)
            if self.ema is not None:
                self._ema_update(st)          # behind the last slice (the early ones went out on this stream too)
            return
        n = m.theta.numel()
        if self.gradient_clip:
            # clip_grad_norm_ over all parameters of the (averaged) gradient: its coefficient lands in opt_state[1], which the step reads
            # (-1 for a coefficient of exactly 0 -- an overflowed norm -- since 0 means "unset": the step then applies no gradient)
            if self._clip_part is None:
                self._clip_part = torch.empty(1024, device=m.device)
            rt.check(m.lib.gcpx_grad_clip_coef(self.grad.data_ptr(), n, scale, float(self.gradient_clip), self._clip_part.data_ptr(), 1024,
                                               self.opt_state.data_ptr(), st), "grad_clip")
        elif self._clip_state_dirty:
            # opt_state[1] is the clip coefficient the step kernels apply whenever it is not 0 (> 0: the coefficient, < 0: a coefficient
            # of zero, written when the norm overflowed): without clipping it must be 0 = unset — also after
            # resuming a checkpoint that was trained WITH clipping (the whole opt_state is restored)
            self.opt_state[1:2].zero_()
            self._clip_state_dirty = False
        kind = self.OPTIMIZERS[self.optimizer]
        if kind == 0:
            rt.check(m.lib.gcpx_radam_step(m.theta.data_ptr(), self.grad.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(),
                                           self.opt_state.data_ptr(), n, self.lr, self.betas[0], self.betas[1], self.eps, scale, st), "radam")
        else:
            # torch.optim defaults of the reference's get_optimizer_class: Adam betas (adam_beta, 0.999); RMSprop alpha 0.99; eps 1e-8
            p1, p2 = (self.betas[0], self.betas[1]) if kind == 1 else ((self.momentum, 0.99) if kind == 2 else (self.momentum, 0.0))
            rt.check(m.lib.gcpx_optim_step(m.theta.data_ptr(), self.grad.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(),
                                           self.opt_state.data_ptr(), n, kind, self.lr, p1, p2, self.eps, scale, st), "optim_step")
        m.repack(st)
        if self.ema is not None:
            self._ema_update(st)

    # ---- the weight average (ema_decay) ----
    def ema_decay_at(self, t):
        """the decay of update t (0-based)"""
        d = self.ema_decay
        return min(d, (1.0 + t) / (10.0 + t)) if self.ema_warmup else d

    def _ema_update(self, st):
        """one gated gcpx_ema_update over the whole vector on stream `st` -- the caller's, on which the step's every write to theta was
        issued and behind which the next forward orders itself: the average has read theta before anything of the next step writes it"""
        m = self.m
        rt.check(m.lib.gcpx_ema_update(self.ema.data_ptr(), m.theta.data_ptr(), m.theta.numel(), self.ema_decay_at(self.ema_updates),
                                       self.opt_state.data_ptr() + 12, 0, st), "ema_update")
        self.ema_updates += 1

    def _refuse_on_ema_weights(self, what):
        if self._ema_swapped:
            raise RuntimeError(f"{what} inside ema_weights(): theta holds the averaged weights; leave the context before training on")

    def _swap_ema(self):
        m = self.m
        st = torch.cuda.current_stream(m.device).cuda_stream
        rt.check(m.lib.gcpx_swap_f32(m.theta.data_ptr(), self.ema.data_ptr(), m.theta.numel(), 0, st), "swap_f32")
        m.repack(st)

    @contextmanager
    def ema_weights(self):
        """Runs the body on the averaged weights: gcpx_swap_f32(theta, ema) + a re-pack of everything on entry, the same on exit (also
        when the body raises).  Contents move, addresses do not: every captured plan and graph stays valid.  BatchNorm running statistics
        live in theta and are averaged and exchanged with it.  step() / backward() inside raise RuntimeError."""
        if self.ema is None:
            raise ValueError("this trainer keeps no weight average (ema_decay=None)")
        if self._ema_swapped:
            raise RuntimeError("ema_weights() is already active")
        self._swap_ema()
        self._ema_swapped = True
        try:
            yield self
        finally:
            self._ema_swapped = False
            self._swap_ema()

    def ema_state(self):
        """checkpoint entry "ema": the average cut with the offsets model.state_dict() uses (so sub-module prefix filters work on it as
        on the weights), and where the warm-up stands"""
        if self.ema is None:
            raise ValueError("this trainer keeps no weight average (ema_decay=None)")
        self._refuse_on_ema_weights("ema_state()")
        flat = self.ema.detach().cpu()
        sd = {k: flat[o:o + _numel(shp)].view(shp).clone() for k, (o, shp) in self.m._poff.items()}
        return {"decay": self.ema_decay, "warmup": self.ema_warmup, "updates": int(self.ema_updates), "state_dict": sd}

    def load_ema_state(self, st):
        """the inverse of ema_state().  None (a checkpoint written without an average): the average starts again from the model's
        weights as they are now, with updates = 0, and says so.  decay / warmup stay the trainer's own (as momentum does)."""
        import warnings
        if self.ema is None:
            raise ValueError("this trainer keeps no weight average (ema_decay=None)")
        self._refuse_on_ema_weights("load_ema_state()")
        if st is None:
            warnings.warn("the checkpoint holds no weight average: it starts again from the loaded weights, ema_updates = 0")
            self.ema.copy_(self.m.theta)
            self.ema_updates = 0
            return
        for k, (o, shp) in self.m._poff.items():
            if k not in st["state_dict"]:
                raise KeyError(f"the checkpoint's weight average has no entry {k}")
            self.ema[o:o + _numel(shp)].view(shp).copy_(st["state_dict"][k])
        self.ema_updates = int(st["updates"])
        for k, own in (("decay", self.ema_decay), ("warmup", self.ema_warmup)):
            if k in st and st[k] != own:
                warnings.warn(f"checkpoint was averaged with ema {k}={st[k]!r}, this trainer runs {k}={own!r}")

    def step(self, inputs, noise=None):
        if self.accumulate > 1:
            return self._micro_step(inputs, noise)
        # (no early slices under a nan_guard either: the verdict needs the whole gradient, as the clipping norm does)
        self._early_on = self.early_optimizer and not self.gradient_clip and not self.nan_guard and len(self._ranges) > 1
        if self._early_on and self._clip_state_dirty:
            self.opt_state[1:2].zero_()          # the early slices read the clip coefficient: it must be 0 (unset) before they run
            self._clip_state_dirty = False
        try:
            out = self.backward(inputs, noise)
        finally:
            self._early_on = False
        self.optimizer_step(out)
        self.stepped = True
        return out

    # ---- gradient accumulation (accumulate > 1) ----
    def _micro_step(self, inputs, noise):
        """step() with accumulate = k > 1: micro-step `micro_index` of the cycle.  Everything the optimizer path reads is in place
        after the last one: self.grad holds the cycle's sum, the health check sees it and the summed loss vector."""
        m, k, j = self.m, self.accumulate, self.micro_index
        self._early_on, self._accumulating, self.stepped = False, True, False
        try:
            out = self.backward(inputs, noise)
        finally:
            self._accumulating = False
        st = torch.cuda.current_stream(m.device).cuda_stream          # (the backward has been joined onto it)
        n, lv = self.grad.numel(), out.raw["losses"]
        acc = m.lib.gcpx_grad_accumulate
        rt.check(acc(self._loss_acc.data_ptr(), lv.data_ptr(), lv.numel(), 1 if j == 0 else 0, 1, st), "grad_accumulate")
        if j < k - 1:
            rt.check(acc(self._acc.data_ptr(), self.grad.data_ptr(), n, 1 if j == 0 else 0, 0, st), "grad_accumulate")
            self.micro_index = j + 1
            return out
        rt.check(acc(self.grad.data_ptr(), self._acc.data_ptr(), n, 0, 0, st), "grad_accumulate")
        self.micro_index, self._grad_div = 0, k
        if self.buckets is not None:
            self.buckets.begin()          # nothing was exchanged during the micro-steps: finish() reduces every bucket of the sum
        if self.nan_guard:
            self._health_extra = self._loss_acc
        self.stepped = True               # (also when the guard drops or raises: the cycle is over)
        self.optimizer_step(out)
        return out

    def reset_accumulation(self):
        """drops a partial cycle: the next step() is the first micro-step again (pass ends, load_optimizer_state)"""
        self.micro_index, self.stepped = 0, False

    def mean_losses(self):
        """the loss vector (out.raw["losses"]) averaged over the micro-batches of the cycle that just completed: a device tensor, no
        sync.  Without accumulation there is nothing to average: call it with accumulate > 1."""
        if self.accumulate == 1:
            raise ValueError("mean_losses() is the cycle mean of a trainer with accumulate > 1; read out.raw['losses'] instead")
        return self._loss_acc / float(self.accumulate)

    # ---- the training guard (health.py) ----
    def _grad_health(self):
        if self._health is None:
            from .health import GradHealth
            self._health = GradHealth(self.m)
        return self._health

    def _raise_if_bad(self, outputs):
        """nan_guard="raise": health check, gated step and re-pack are enqueued; copy the summary behind them and wait -- the device
        works while the host does.  A verdict of 1 raises; the device has already skipped the update."""
        from .health import NonFiniteGradients
        h = self._grad_health()
        summary = h.read_summary(torch.cuda.current_stream(self.m.device))
        if summary[6]:
            bad, ok = h.bad()
            raise NonFiniteGradients(bad, ok, int(summary[5]), outputs)

    def health(self):
        """the guard's counts of the last step, as device tensors and without a sync (like gradient_stats()):
        Outputs(names, seg_bad [len(names), 3] = NaN, +Inf, -Inf elements per parameter, summary [8] int32: totals, number of bad
        parameters, the first of them or -1, non-finite loss entries, this step's verdict, [7] the number of skipped steps so far)"""
        from .plan_ops import Outputs
        if not self.nan_guard:
            raise ValueError("this trainer runs without a nan_guard")
        h = self._grad_health()
        return Outputs(names=h.names, seg_bad=h.seg_bad, summary=h.summary)

    def optimizer_state(self):
        """optimizer.state_dict() counterpart (train.py:111): flat first / second moments + step counter"""
        state = self.opt_state.detach().cpu()
        state[3] = 0.0                        # the gate belongs to the step that set it: a resumed trainer must step
        return {"exp_avg": self.exp_avg.detach().cpu(), "exp_avg_sq": self.exp_avg_sq.detach().cpu(),
                "state": state, "lr": self.lr, "betas": tuple(self.betas), "eps": self.eps,
                "optimizer": self.optimizer, "momentum": self.momentum, "gradient_clip": self.gradient_clip}

    def load_optimizer_state(self, st):
        self.reset_accumulation()
        self.exp_avg.copy_(st["exp_avg"])
        self.exp_avg_sq.copy_(st["exp_avg_sq"])
        state = torch.as_tensor(st["state"]).detach().to("cpu", torch.float32, copy=True)
        state[3] = 0.0                        # a stored gate must not outlive its run (as the clip coefficient below)
        self.opt_state.copy_(state)
        self.lr, self.betas, self.eps = st["lr"], tuple(st["betas"]), st["eps"]
        if st.get("optimizer", self.optimizer) != self.optimizer:
            raise ValueError(f"checkpoint holds the state of optimizer '{st['optimizer']}', this trainer runs '{self.optimizer}'")
        # momentum / gradient_clip are the TRAINER's settings (the conf's), as torch.optim's load_state_dict keeps the param-group
        # values it is given; a checkpoint trained with other values resumes, but says so
        for k in ("momentum", "gradient_clip"):
            if k in st and st[k] != getattr(self, k):
                import warnings
                warnings.warn(f"checkpoint was trained with {k}={st[k]!r}, this trainer runs {k}={getattr(self, k)!r}")
        self._clip_state_dirty = True         # a restored clip coefficient must not outlive a trainer without clipping

    def gradient_stats(self):
        """log_gradients (base_model.py:139-146) after `step()` / `backward()`: the L2 norm of every parameter's gradient, their mean
        and maximum -- one gcpx_grad_segment_norms on the caller's stream, no sync.  Returns device tensors:
        Outputs(names, seg_norm [len(names)], stats [4] = mean, max, number counted, number of non-finite norms).  The gradient buffer
        still holds the step's gradient (the optimizer kernels read it, the next backward clears it); under a process group it holds
        the ranks' sum and is scaled by 1 / world here; the step's clipping coefficient (opt_state[1], 0 = none, < 0 = zero) is applied as the
        step kernels apply it.  A parameter whose gradient is zero everywhere is not counted (`p.grad is None`)."""
        from .plan_ops import Outputs
        from .scalar_log import GradStats
        if getattr(self, "_grad_stats", None) is None:
            self._grad_stats = GradStats(self.m)
        scale = 1.0
        if self.buckets is not None and torch.distributed.is_initialized():
            scale = 1.0 / torch.distributed.get_world_size(self.buckets.group)
        if self._grad_div > 1:            # after a completed accumulation cycle: the buffer holds the sum of its micro-gradients
            scale = 1.0 / (self._grad_div * round(1.0 / scale))
        st = torch.cuda.current_stream(self.m.device).cuda_stream
        seg_norm, stats = self._grad_stats.launch(self.m.lib, self.grad, scale, self.opt_state.data_ptr() + 4, st)
        return Outputs(names=self._grad_stats.names, seg_norm=seg_norm, stats=stats)

    def named_grads(self):
        return {k: self.grad[o:o + int(torch.tensor(shp).prod())].view(shp) for k, (o, shp) in self.m._poff.items()}
