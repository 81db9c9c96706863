"""Training entry point: `python -m video_gcp_amd.train --path <exp_dir> [flags]` — the counterpart of
/root/reference/gcp/prediction/train.py (ModelTrainer.run / train / train_epoch / val / save_checkpoint / resume, :24-213)
with the flags of gcp/prediction/training/gcp_builder.py:188-247 that concern the device path.

What is replaced: `output = model(inputs); losses = model.loss(...); total.backward(); optimizer.step()` (train.py:155-163)
runs as `GCPTrainStep.step` (HIP forward + explicit backward + RAdam, training.py); data-parallel training is one process
per GPU (launch with `python -m torch.distributed.run --nproc-per-node N -m video_gcp_amd.train ...`), every rank on its own
shard, gradients averaged with ONE RCCL all-reduce over the flat gradient vector (gcp_builder.py:71-78 used nn.DataParallel).
What is NOT here: reading HDF5 files directly, TensorBoard logging, the control evaluation.  The experiment directory
holds `conf.json` ({"config": "c2", "overrides": {...}, "num_epochs": n, "lr": x, "batches_per_epoch": k}) or a reference-style conf.py.
Data: `--data_dir DIR` (or `configuration['data_dir']`, or `$GCP_DATA_DIR/<dataset_name>` as gcp_builder.py:118,152 resolve it)
trains and validates on a recorded dataset in the reference's layout stored as `.npz` (dataset.py: uint8 frames uploaded from pinned
host memory and assembled on the device); its dataset_spec.py overrides the model hyper-parameters (gcp_builder.py:68).  Without a
data directory, `--feed_random_data 1` (the reference's own debug flag, gcp_builder.py:239, on by default) feeds the seeded
synthetic batches of SURVEY §8d; `dataset` may also be any iterable of input dicts passed to ModelTrainer.
Prediction metrics (gcp_builder.py:84-95, train.py:205-226): with `--skip_top100_val 0` every validation batch is also scored by
evaluation.Evaluator (best of `--top_of` prior samples by mse, psnr and ssim after the configuration's `metric_pruning_scheme`, when
`top_of_100_eval`), and <path>/metrics/results_<global_step>.txt / .npz plus the best samples' frames are written after each validation.
`--metric 1` evaluates the `test` split, unshuffled, writes the results and returns: no training, no optimizer step, no checkpoint.
Deviation: the reference defaults `--skip_top100_val` to 0; here it defaults to 1, so that a plain validation is what it was (the
prior-sampled forward and the NLL).  `--top_of` (the reference's fixed `_top_of = 100`) is this build's.
Frame size: `--resize_frames 1` resizes recorded frames stored at another size than the model's img_sz inside the device-side batch
assembly, as Pillow's bilinear Image.resize does (dataset.py), for the train, validation and `--metric` test loaders alike.
Deviation: the reference resizes every item (data_loader.py:213-220); here it defaults to 0, so that a dataset of the wrong size
stops the run as it did before the option existed.
Resident data: `--device_dataset 1` uploads every split it reads (train and val, or test under `--metric 1`) once and keeps it on the
device as uint8; each batch then sends B * (64 + 4 T) bytes of indices and pad masks and is assembled from the store on the device
(dataset_resident.py), bit-identical to the host-fed batches, also with `--resize_frames 1`.  `--device_dataset_gb G` bounds one split's
store (default: half of the device's memory); a split that does not fit, or a top-rendered nav dataset, raises.  Every rank of a
process group holds the whole split.  Defaults to 0, and the trainer then issues no launch, copy or allocation it did not issue before.
On a nav dataset (Nav9Rooms, Nav25Rooms) the picture logs also hold `regressed_state_topdown` / `action_traj_topdown`, and `--metric 1`
writes `<path>/metrics/trajectories/it_<step>/trajectories_<b>.png`: the maze with the state trajectories drawn on it (image_log.py).

Picture logs: `--log_images 1` writes the reference's prediction panels (model.log_outputs, image_log.py) as PNG / animated PNG to
<path>/images/<name>_<phase>_<step>.png|.apng, on rank 0, unless --dont_save: in training every int(epoch_len / --imepoch) steps
(train.py:125-130,147,170-172), in validation for the last batch's prior-sampled prediction (train.py:229-230).
Deviation: the reference defaults `--log_images` to 1 (gcp_builder.py:231); here it defaults to 0, and the loop then issues no launch,
copy or sync it did not issue before.
Scalar logs: `--log_scalars 1` writes, on rank 0 unless --dont_save, a TensorBoard event file and scalar_data.json under <path>/events
(scalar_log.py; gcp_builder.py:41-54, logger.py:43-44,98-100).  On the steps that already synchronise (global_step %
--log_outputs_interval == 0): every loss term of the step as `<name>_loss_train`, `total_loss_train`, the tree's
`kl_loss_layerwise/level_<l>_train`, `gradients/mean_norm_train`, `gradients/max_norm_train` (base_model.py:139-146) and
`gradients/nonfinite_train` over the per-parameter gradient norms, `time/batch_train` and `time/data_load_train` (the clocks of
train.py:182-186).  After a validation: the averages of every term over its batches, once, at global_step, as `..._val`
(train.py:229-230), the layer-wise KL of the last batch, and scalar_data.json is rewritten.  Under a process group the loss terms are
rank 0's shard (the reference's DataParallel saw the whole batch); the gradient norms are of the all-reduced gradient, identical on
every rank.  Deviation: the reference always logs; `--log_scalars` defaults to 0, and nothing then changes anywhere.
Training guard: `--nan_guard raise|skip` tests every step's gradient and loss vector for NaN / +-Inf on the device, between the
backward and the optimizer, and keeps a bad gradient out of the weights and moments (health.py; NanGradHook, base_trainer.py:20-66,
gcp_builder.py:99-103; base_gcp.py:302-303).  `raise` stops as the reference does: rank 0 writes <path>/nan_debug_info.npz (the batch,
the loss terms, end_ind, the bad and OK parameter names and counts, global_step, epoch) and <path>/nan_debug_ckpt.pth (the untouched
weights and optimizer state, in the checkpoint format), prints the two lists and the run ends with NonFiniteGradients.  `skip` drops
the step on the device without a sync and goes on; with --log_scalars 1 `gradients/skipped_steps_train` counts them, and the total is
printed at the end.  Under either, a checkpoint is written only from finite parameters and running statistics.
Deviation: the reference always installs its hook; `--nan_guard` defaults to off, and a plain run is what it was.
Gradient accumulation: `--accumulate_steps k` (no reference counterpart, and a flag only: `batch_size` of a conf stays the micro-batch)
makes every optimizer step the mean gradient of k consecutive micro-batches, each with its own BatchNorm statistics -- what k times as
many data-parallel ranks compute, up to the summation order and the noise streams (training.py, dataset.accumulate_schedule).
global_step, model.step() (KL burn-in), the picture-log interval and the print / scalar-log block count optimizer steps; the printed
and logged loss terms are the cycle's means; `--nan_guard raise` dumps the inputs of the cycle's LAST micro-batch.  Defaults to 1.
Weight average: `--ema_decay D` (no reference counterpart, a flag only) keeps an exponential moving average of the weights and BatchNorm
running statistics on the device, moved once per optimizer step (training.py); `--ema_warmup 1` (default) uses min(D, (1 + t) / (10 + t))
for update t.  With `--eval_ema 1` (default) every validation pass, `--metric 1` and the validation-phase picture logs run on the averaged
weights (trainer.ema_weights()); checkpoints store the average under "ema" and `--resume` restores it (a checkpoint without one: the
average starts from the loaded weights, with a warning).  `--metric 1 --resume CKPT` without `--ema_decay` evaluates the checkpoint's
average when it holds one (`--eval_ema 0`: its weights).  Defaults to 0 = off: no allocation, no launch, no extra checkpoint key.
"""
import argparse
import json
import os
import time

import torch


def get_cmd_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--path", help="path to the experiment directory (conf.json; weights/ is created inside)")
    p.add_argument("--config", default=None, help="named configuration (c1..c5) when there is no conf.json")
    p.add_argument("--dont_save", default=False, type=int)
    p.add_argument("--resume", default="", type=str, help="'latest', an epoch number or a checkpoint path")
    p.add_argument("--train", default=True, type=int, help="if 0, runs one validation epoch")
    p.add_argument("--skip_first_val", default=False, type=int)
    p.add_argument("--gpu", default=-1, type=int)
    p.add_argument("--strict_weight_loading", default=True, type=int)
    p.add_argument("--deterministic", default=False, type=int)
    p.add_argument("--log_outputs_interval", default=10, type=int)
    p.add_argument("--feed_random_data", default=True, type=int)
    p.add_argument("--verbose_timing", default=False, type=int)
    p.add_argument("--num_epochs", default=None, type=int)
    p.add_argument("--batches_per_epoch", default=None, type=int)
    p.add_argument("--data_dir", default=None, type=str, help="dataset directory (dataset_spec.py + hdf5/<phase>/*.npz, dataset.py)")
    p.add_argument("--skip_top100_val", default=True, type=int, help="if 0, scores the best of --top_of prior samples at every validation "
                   "(the reference's default is 0)")
    p.add_argument("--metric", default=False, type=int, help="if 1, evaluates the test split, writes the metrics and returns")
    p.add_argument("--top_of", default=100, type=int, help="prior samples per sequence of the top-of-N evaluation")
    p.add_argument("--resize_frames", default=0, type=int, help="if 1, frames stored at another size are resized to img_sz on the device "
                   "(bilinear, as the reference's loader always does)")
    p.add_argument("--device_dataset", default=0, type=int, help="if 1, every split is uploaded once and kept on the device as uint8; "
                   "batches are assembled from it there (dataset_resident.py). A split that does not fit raises")
    p.add_argument("--device_dataset_gb", default=None, type=float, help="the most device memory one resident split may take, in GiB "
                   "(default: half of the device's memory)")
    p.add_argument("--imepoch", default=4, type=int, help="number of times pictures are logged per epoch")
    p.add_argument("--log_images", default=0, type=int, help="if 1, writes prediction panels to <path>/images (the reference's "
                   "default is 1)")
    p.add_argument("--log_scalars", default=0, type=int, help="if 1, writes loss terms, gradient norms and the layer-wise KL to "
                   "<path>/events (event file + scalar_data.json; the reference always does)")
    p.add_argument("--nan_guard", default="off", choices=("off", "raise", "skip"), help="tests every gradient for NaN / Inf on the device "
                   "before the optimizer applies it: 'raise' dumps the batch and a checkpoint and stops (the reference always does), "
                   "'skip' drops the step and goes on")
    p.add_argument("--accumulate_steps", default=1, type=int, help="micro-batches of `batch_size` whose mean gradient makes one optimizer "
                   "step: one GPU then trains with the batch of k ranks")
    p.add_argument("--ema_decay", default=0.0, type=float, help="decay in (0, 1) of an exponential moving average of the weights, moved on "
                   "the device once per optimizer step; 0 = none")
    p.add_argument("--ema_warmup", default=1, type=int, choices=(0, 1), help="if 1, update t uses min(ema_decay, (1 + t) / (10 + t))")
    p.add_argument("--eval_ema", default=1, type=int, choices=(0, 1), help="if 1, validation, --metric and the validation picture logs "
                   "run on the averaged weights (with --ema_decay, or under --metric on a resumed checkpoint that holds an average)")
    args = p.parse_args(argv)
    if args.accumulate_steps < 1:
        p.error("--accumulate_steps must be at least 1")
    if args.ema_decay != 0.0 and not 0.0 < args.ema_decay < 1.0:
        p.error("--ema_decay must be 0 (off) or lie in (0, 1)")
    return args


def ema_kwargs(args):
    """the trainer's weight-average arguments: none at all for --ema_decay 0, so that the trainer is built as it always was"""
    decay = float(getattr(args, "ema_decay", 0.0) or 0.0)
    return dict(ema_decay=decay, ema_warmup=bool(getattr(args, "ema_warmup", 1))) if decay else {}


def startup_line(micro_batch, accumulate, world):
    """what the trainer prints once: the batch an optimizer step averages over"""
    return "[train] micro-batch {} x accumulate_steps {} x world {} = effective batch {}".format(
        micro_batch, accumulate, world, micro_batch * accumulate * world)


def _raw_conf(path):
    """(configuration, model_config) of the experiment directory as written (conf.py or conf.json), {} / {} without one"""
    import glob
    from .conf_loader import exec_conf_py
    if path and os.path.isdir(path):
        py = sorted(glob.glob(os.path.join(os.path.abspath(path), "*.py")))
        if len(py) == 1:
            return exec_conf_py(py[0])
        js = os.path.join(path, "conf.json")
        if os.path.exists(js):
            return json.load(open(js)), {}
    return {}, {}


def load_conf_with_data(path, config, data_dir=None, use_data=True):
    """load_conf plus the dataset: (hp, trainer settings, ignored keys, data_dir or None, dataset spec, reader options).  The data
    directory is `data_dir`, else configuration['data_dir'], else $GCP_DATA_DIR/<configuration['dataset_name']> (gcp_builder.py:118,152,
    utils.py:74-76); its spec's non-list entries override the model hyper-parameters (gcp_builder.py:68)."""
    from .conf_loader import load_conf
    from .hparams import GCPHParams
    configuration, model_config = _raw_conf(path)
    if use_data and data_dir is None:
        data_dir = configuration.get("data_dir")
        name = configuration.get("dataset_name")
        if data_dir is None and isinstance(name, str) and os.environ.get("GCP_DATA_DIR"):
            data_dir = os.path.join(os.environ["GCP_DATA_DIR"], name)
    if not use_data or not data_dir:
        hp, conf, ignored = load_conf(path, default="c2", name=config)
        return hp, conf, ignored, None, None, {}
    from .dataset import load_spec, spec_overrides
    spec = load_spec(data_dir)
    hp, conf, ignored = load_conf(path, default="c2", name=config, **spec_overrides(spec, set(GCPHParams.__dataclass_fields__)))
    # randomize_length / randomize_start: model hyper-parameters of the reference (the dataset reads them from the model's hparams)
    opts = {k: bool(spec.get(k, model_config.get(k, configuration.get(k, False)))) for k in ("randomize_length", "randomize_start")}
    return hp, conf, ignored, data_dir, spec, opts


def val_phase(args):
    """the split validation reads (gcp_builder.py:84): `test` under --metric, `val` otherwise; both unshuffled (:119)"""
    return "test" if getattr(args, "metric", False) else "val"


def make_loader(data_dir, spec, phase, hp, model, data_opts, n_repeat=1, seed=0, rank=0, world=1, resize=False, resident=False,
                budget_bytes=None, accumulate=1):
    """the reference's loaders (gcp_builder.py:100-103,105-120): epoch_cycles_train passes per epoch, shuffled in the train phase only;
    `resize`: frames stored at another size are resized to hp.img_sz in the batch assembly (--resize_frames);
    `resident`: the split is uploaded once and the batches are assembled from it on the device (--device_dataset, dataset_resident.py;
    at most `budget_bytes` of it, a top-rendered dataset raises);
    `accumulate`: k micro-batches per optimizer step (--accumulate_steps): the pass walks dataset.accumulate_schedule"""
    from .dataset import HostFedLoader, VideoDataset
    ds = VideoDataset(data_dir, spec, phase, hp.img_sz, resize=resize, **data_opts)
    if resident:
        from .dataset_resident import ResidentLoader
        return ResidentLoader(ds, model, hp.batch_size, n_repeat=n_repeat, seed=seed, rank=rank, world=world, budget_bytes=budget_bytes,
                              accumulate=accumulate)
    return HostFedLoader(ds, model, hp.batch_size, n_repeat=n_repeat, seed=seed, rank=rank, world=world, accumulate=accumulate)


class SyntheticLoader:
    """Seeded synthetic batches: a different shard per rank, a different batch per step.
    accumulate = k: k * (n_batches // k) batches, so that a pass ends on a cycle boundary."""

    def __init__(self, hp, n_batches, seed, device, variant="B", accumulate=1):
        n_batches = int(accumulate) * (n_batches // int(accumulate))
        self.hp, self.n, self.seed, self.device, self.variant = hp, n_batches, seed, device, variant

    def __len__(self):
        return self.n

    def __iter__(self):
        from .synthetic import make_inputs, make_inputs_device
        on_gpu = torch.device(self.device).type == "cuda"
        for i in range(self.n):
            if on_gpu:                                   # drawn on the device: the host path is 9x slower than a training step
                yield make_inputs_device(self.hp, self.seed + i, self.variant, self.device)
            else:
                inputs, _, _ = make_inputs(self.hp, seed=self.seed + i, variant=self.variant)
                yield {k: v.to(self.device) for k, v in inputs.items()}


class ModelTrainer:
    def __init__(self, args=None, train_loader=None, val_loader=None):
        from . import dist as D
        from .hparams import config
        from .model import GCPTreeModel
        from .params import init_params
        from .training import GCPTrainStep
        self.cmd_args = args = args if args is not None else get_cmd_args()
        # <path>/conf.py in the reference's format (`configuration` + `model_config`, gcp_builder.py:129-147) or <path>/conf.json
        name = args.config or "c2"
        # an explicit --config wins over conf.json's "config" entry (and names the default experiment directory below)
        self.hp, conf, self.ignored_conf_keys, self.data_dir, spec, data_opts = load_conf_with_data(
            args.path, args.config, getattr(args, "data_dir", None))
        for k in self.ignored_conf_keys:
            if k.startswith("defaulted:"):
                print(f"[train] {k[10:]} is not in the configuration file (the reference reads it from the dataset spec): "
                      f"using {getattr(self.hp, k[10:])}", flush=True)
            else:           # inert for what is computed (conf_loader.KEY_TABLE); a key that would change it has raised in the loader
                print(f"[train] configuration key not used: {k}", flush=True)
        hp = self.hp
        self.exp_path = args.path or os.path.join("experiments", name)
        self.rank, self.local_rank, self.world = D.init_from_env()
        if args.gpu >= 0:
            self.local_rank = args.gpu
        torch.cuda.set_device(self.local_rank)
        self.device = torch.device("cuda", self.local_rank)
        self.num_epochs = args.num_epochs if args.num_epochs is not None else conf.get("num_epochs", 1)
        nb = args.batches_per_epoch if args.batches_per_epoch is not None else conf.get("batches_per_epoch", 10)
        seed = 0 if args.deterministic else conf.get("seed", 0)
        # same initial weights on every rank (same seed) = the broadcast of DataParallel replicas ...
        # configuration['model'] (gcp_builder.py:75) chooses the class: TreeModel or the flat VRNN baseline SequentialModel
        # (experiments/prediction/base_configs/gcp_sequential.py)
        self.model_kind = conf.get("model", "tree")
        if self.model_kind == "sequential":
            from .params import init_params_sequential
            from .sequential import GCPSequentialModel
            from .training_sequential import SequentialTrainStep
            model_cls, init_fn, step_cls = GCPSequentialModel, init_params_sequential, SequentialTrainStep
        else:
            model_cls, init_fn, step_cls = GCPTreeModel, init_params, GCPTrainStep
        self.model = model_cls(hp, params=init_fn(hp, seed=seed), device=self.device)
        # ... but a DIFFERENT stream of latent noise / auxiliary-model index draws per rank, as nn.DataParallel's replicas drew
        # different numbers for their different shards (gcp_builder.py:71-78); reproducible through `seed` / --deterministic
        torch.cuda.manual_seed(seed * max(self.world, 1) + self.rank + 1)
        self.model.reseed()                   # (a second trainer of the process seeded with the same value starts the same stream again)
        pg = torch.distributed.group.WORLD if self.world > 1 else None
        lr = conf.get("lr") if conf.get("lr") is not None else 1e-3
        guard = getattr(args, "nan_guard", "off")
        self.nan_guard = None if guard in (None, "off") else guard
        guard_kw = {"nan_guard": self.nan_guard} if self.nan_guard else {}
        self.accumulate = k_acc = int(getattr(args, "accumulate_steps", 1) or 1)
        if k_acc > 1:
            guard_kw["accumulate"] = k_acc
        guard_kw.update(ema_kwargs(args))
        self.eval_ema = bool(getattr(args, "eval_ema", 1))
        self._ema_loaded = False              # --metric on a checkpoint with an average: theta itself holds the averaged weights
        if self.rank == 0:
            print(startup_line(hp.batch_size, k_acc, max(self.world, 1)), flush=True)
        self.trainer = step_cls(self.model, lr=lr, betas=(conf.get("adam_beta", 0.9), 0.999), process_group=pg,
                                optimizer=conf.get("optimizer", "radam"), momentum=conf.get("momentum", 0),
                                gradient_clip=conf.get("gradient_clip"), **guard_kw)       # gcp_builder.py:174-186,255-263
        self._weight_health = None
        if self.data_dir and (train_loader is None or val_loader is None):
            # the reference's loaders (gcp_builder.py:100-103,105-120): epoch_cycles_train passes per epoch, val / test unshuffled
            reps = int(conf.get("epoch_cycles_train", 1))
            gb = getattr(args, "device_dataset_gb", None)
            # (validation is not accumulated: its loader walks the plain schedule)
            mk = lambda phase, k=1: make_loader(self.data_dir, spec, phase, hp, self.model, data_opts, n_repeat=reps, seed=seed,
                                                rank=self.rank, world=max(self.world, 1), resize=bool(getattr(args, "resize_frames", 0)),
                                                resident=bool(getattr(args, "device_dataset", 0)),
                                                budget_bytes=None if gb is None else int(gb * 2 ** 30), accumulate=k)
            train_loader = train_loader or mk("train", k_acc)
            val_loader = val_loader or mk(val_phase(args))
        if not args.feed_random_data and train_loader is None:
            raise ValueError("no dataset reader ships with this build: pass --feed_random_data 1 or give ModelTrainer a loader")
        self.train_loader = train_loader or SyntheticLoader(hp, nb, 1000 + 100000 * self.rank, self.device, accumulate=k_acc)
        self.val_loader = val_loader or SyntheticLoader(hp, max(1, nb // 5), 500000 + 100000 * self.rank, self.device)
        self.global_step = 0
        self.log = []
        # gcp_builder.py:91-95 (both models have a dense_rec here): the top-of-N evaluator, on --metric or --skip_top100_val 0
        self.log_images = bool(getattr(args, "log_images", 0)) and not args.dont_save and self.rank == 0
        if self.log_images:
            self.model.log_dir = os.path.join(self.exp_path, "images")
        self.image_files = []
        # a top-rendered (nav) dataset: its picture and stamps also serve the trajectory panels of the picture logs and of --metric
        top = getattr(getattr(self.train_loader, "ds", None), "topdown", None) or getattr(getattr(self.val_loader, "ds", None), "topdown", None)
        if top is not None and self.rank == 0 and (self.log_images or getattr(args, "metric", False)):
            self.model.topdown_assets = top
        self.scalar_log = None
        if bool(getattr(args, "log_scalars", 0)) and not args.dont_save and self.rank == 0:
            from .scalar_log import ScalarLogger
            self.scalar_log = self.model.scalar_log = ScalarLogger(os.path.join(self.exp_path, "events"))
        self.evaluator = None
        if getattr(args, "metric", False) or not getattr(args, "skip_top100_val", True):
            from .evaluation import Evaluator
            self.evaluator = Evaluator(self.model, pruning_scheme=conf.get("metric_pruning_scheme", "dtw"),
                                       top_of_100=bool(conf.get("top_of_100_eval", True)), top_of=int(getattr(args, "top_of", 100)))

    # ---- train.py:28-54 ----
    def run(self):
        start_epoch = 0
        if self.cmd_args.resume:
            start_epoch = self.resume(self.cmd_args.resume)
        try:
            if getattr(self.cmd_args, "metric", False):
                self.val()                             # train.py:222-226: one evaluation pass of the test split, then stop
                return
            if self.cmd_args.train:
                self.train(start_epoch)
            else:
                self.val()
        finally:
            if self.scalar_log is not None:
                self.scalar_log.dump_scalars()
                self.scalar_log.close()
            if self.nan_guard == "skip" and self.rank == 0 and self.trainer._health is not None:
                print("[train] steps skipped for non-finite gradients: {}".format(int(self.trainer.health().summary[7])), flush=True)

    # ---- train.py:56-70, checkpoint_handler.py:31-74 ----
    def resume(self, ckpt, path=None):
        from . import checkpoint as CK
        folder = os.path.join(self.exp_path if path is None else path, "weights")
        try:
            f = CK.get_resume_ckpt_file(ckpt, folder)
        except CK.NoCheckpointsException:               # train.py:59-62: `--resume latest` on a fresh experiment starts at epoch 0
            return 0
        strict = bool(self.cmd_args.strict_weight_loading)
        if getattr(self.cmd_args, "metric", False) and self.eval_ema and self.trainer.ema is None and CK.read_ema_state(f) is not None:
            # an evaluation pass of a checkpoint that holds an average, by a trainer that keeps none: the averaged weights are loaded
            self.global_step, epoch, opt = CK.load_weights(f, self.model, strict=strict, use_ema=True)
            self._ema_loaded = True
        else:
            self.global_step, epoch, opt = CK.load_weights(f, self.model, strict=strict)
        if opt is not None:
            self.trainer.load_optimizer_state(opt)
        if self.trainer.ema is not None:
            self.trainer.load_ema_state(CK.read_ema_state(f))          # (none stored: starts from the loaded weights, and warns)
        # schedules follow the step counter (the KL-weight burn-in, base_gcp.py:121-128, counts model.step() calls)
        self.model.n_steps = int(self.global_step)
        self.model._set_kl_weight()
        self.model.train()
        return epoch + 1

    # ---- train.py:95-104 ----
    def train(self, start_epoch):
        if not self.cmd_args.skip_first_val:
            self.val()
        for epoch in range(start_epoch, self.num_epochs):
            self.train_epoch(epoch)
            if not self.cmd_args.dont_save and self.rank == 0:
                self.save_checkpoint(epoch)
            self.val()

    # ---- train.py:106-115 ----
    def save_checkpoint(self, epoch):
        from . import checkpoint as CK
        if self.nan_guard:
            self.check_weights()                       # never overwrite a good checkpoint with non-finite weights
        ema_kw = {"ema_state": self.trainer.ema_state()} if self.trainer.ema is not None else {}
        return CK.save_checkpoint(self.model, os.path.join(self.exp_path, "weights"), epoch, self.global_step,
                                  self.trainer.optimizer_state(), **ema_kw)

    def check_weights(self):
        """one gcpx_grad_health over theta -- parameters and BatchNorm running statistics -- and a sync: raises NonFiniteWeights when
        anything in it is NaN or +-Inf (once per epoch, in front of save_checkpoint)"""
        from .health import GradHealth, NonFiniteWeights
        if self._weight_health is None:
            self._weight_health = GradHealth(self.model, buffers=True)
        h, stream = self._weight_health, torch.cuda.current_stream(self.device)
        h.launch(self.model.lib, self.model.theta, None, None, stream.cuda_stream)
        if h.read_summary(stream)[6]:
            raise NonFiniteWeights(h.bad()[0])

    def dump_nan_debug(self, err, inputs, epoch):
        """NanGradHook's report (base_trainer.py:24-66): the two name lists, nan_debug_info.npz and nan_debug_ckpt.pth.  The reference
        pickles every output tensor; here the outputs are the plan's device buffers (gigabytes at c2), so only end_ind goes along."""
        import numpy as np
        from . import checkpoint as CK
        print("Detected NaN gradients, dumping data for diagnosis, ...", flush=True)
        if not self.cmd_args.dont_save:
            info = {"inputs/" + k: v.detach().cpu().numpy() for k, v in inputs.items() if torch.is_tensor(v)}
            if err.outputs is not None:
                for k, v in self.model.loss(inputs, err.outputs).items():
                    v = v.value if isinstance(v, dict) else v
                    info["losses/" + ("total" if k == "_total" else k)] = np.asarray(v.detach().cpu().numpy() if torch.is_tensor(v) else v)
                end_ind = err.outputs.get("end_ind")
                if torch.is_tensor(end_ind):
                    info["outputs/end_ind"] = end_ind.detach().cpu().numpy()
            info["bad_parameters"] = np.array([b[0] for b in err.bad], dtype=str)
            info["ok_parameters"] = np.array(list(err.ok), dtype=str)
            info["bad_counts"] = np.array([b[1:] for b in err.bad], dtype=np.int64).reshape(len(err.bad), 3)
            info["loss_nonfinite"] = np.int64(err.loss_nonfinite)
            info["global_step"], info["epoch"] = np.int64(self.global_step), np.int64(epoch)
            os.makedirs(self.exp_path, exist_ok=True)
            np.savez(os.path.join(self.exp_path, "nan_debug_info.npz"), **info)
            CK.save_checkpoint(self.model, self.exp_path, epoch, self.global_step, self.trainer.optimizer_state(),
                               name="nan_debug_ckpt.pth")
        print("nan gradients here: ", [b[0] for b in err.bad])                  # base_trainer.py:31-32
        print("there parameters are OK: ", list(err.ok), flush=True)

    # ---- train.py:132-193 ----
    def train_epoch(self, epoch):
        self.model.train()
        if hasattr(self.train_loader, "set_epoch"):
            self.train_loader.set_epoch(epoch)          # the dataset loader's shuffle and draws are keyed on the epoch
        end = time.time()
        # train.py:147 (an epoch shorter than --imepoch batches logs every step instead of dividing by zero)
        k_acc = self.accumulate
        images_interval = max(1, int(len(self.train_loader) // k_acc / max(1, getattr(self.cmd_args, "imepoch", 4)))) if self.log_images else 0
        if k_acc > 1:
            self.trainer.reset_accumulation()          # a pass ends on a cycle boundary; a loader that was cut short leaves no partial cycle
        slog = self.scalar_log
        tick, data_time, n_timed = time.time(), 0.0, 0          # (--log_scalars only) time spent waiting for the loader
        for batch_idx, inputs in enumerate(self.train_loader):
            if slog is not None:
                data_time, n_timed = data_time + time.time() - tick, n_timed + 1
            try:
                out = self.trainer.step(inputs)        # zero_grad, forward, loss, backward, (all-reduce), optimizer.step
            except ValueError as err:                  # --nan_guard raise: the reference's hook (gcp_builder.py:99-103)
                from .health import NonFiniteGradients
                if isinstance(err, NonFiniteGradients) and self.rank == 0:
                    if k_acc > 1:
                        print("[train] --accumulate_steps {}: the gradient is the sum over {} micro-batches; the inputs dumped are "
                              "the LAST micro-batch's".format(k_acc, k_acc), flush=True)
                    self.dump_nan_debug(err, inputs, epoch)
                raise
            if not self.trainer.stepped:               # a micro-step of an accumulation cycle: no optimizer step yet
                if slog is not None:
                    tick = time.time()
                continue
            self.model.step()                          # train.py:163
            if self.log_images and self.global_step % images_interval == 0:          # train.py:125-126,170-172
                self.image_files += self.model.log_outputs(out, inputs, None, self.global_step, True, "train")
            if self.global_step % self.cmd_args.log_outputs_interval == 0:
                if k_acc > 1:                          # the cycle's mean loss vector stands in for the last micro-batch's below
                    last_losses, out.raw["losses"] = out.raw["losses"], self.trainer.mean_losses()
                total = float(out.raw["losses"][5])    # the only host sync of the loop, on logging steps
                self.log.append((self.global_step, total))
                batch_time = (time.time() - end) / max(1, self.cmd_args.log_outputs_interval)
                if self.rank == 0:
                    print("itr: {} Train Epoch: {} [{}/{}]\tLoss: {:.6f}\t{:.3f}s/batch".format(
                        self.global_step, epoch, batch_idx, len(self.train_loader), total, batch_time), flush=True)
                if slog is not None:
                    self.log_train_scalars(out, inputs, total, batch_time, data_time / max(n_timed, 1))
                    data_time, n_timed = 0.0, 0
                if k_acc > 1:
                    out.raw["losses"] = last_losses
                end = time.time()
            self.global_step += 1
            if slog is not None:
                tick = time.time()

    def log_train_scalars(self, out, inputs, total, batch_time, data_time):
        """the scalars of one logging step (base_model.py:86-108,139-146, train.py:170-186): loss terms, layer-wise KL, gradient norms
        (one launch behind the step, read back in one copy) and the two host clocks"""
        stats = self.trainer.gradient_stats().stats
        if self.nan_guard == "skip":                   # the count of skipped steps rides in the same copy
            stats = torch.cat([stats, self.trainer.health().summary[7:8].to(torch.float32)])
        losses = self.model.loss(inputs, out)
        losses["_total"] = total
        self.model.log_outputs(out, inputs, losses, self.global_step, False, "train")
        mean, mx, _, nonfinite, *skipped = stats.tolist()
        for name, v in (("gradients/mean_norm", mean), ("gradients/max_norm", mx), ("gradients/nonfinite", nonfinite),
                        ("time/batch", batch_time), ("time/data_load", data_time)) + tuple(("gradients/skipped_steps", v) for v in skipped):
            self.scalar_log.log_scalar(v, name, self.global_step, "train")
        self.scalar_log.flush()

    # ---- train.py:195-238: prior-sampled prediction (val_mode) + the training forward for the NLL, no gradient ----
    def val(self):
        """with a weight average and --eval_ema 1 the whole pass -- prediction, metrics, picture logs, NLL -- runs on the averaged
        weights (trainer.ema_weights(): exchanged on entry, exchanged back on exit)"""
        if self.trainer.ema is not None and self.eval_ema:
            with self.trainer.ema_weights():
                return self._val()
        return self._val()

    def _val(self):
        tot, n = 0.0, 0
        slog, term_names, term_sum = self.scalar_log, None, None
        start = time.time()
        n_val = len(self.val_loader) if self.log_images and hasattr(self.val_loader, "__len__") else -1
        for i_val, inputs in enumerate(self.val_loader):
            with self.model.val_mode(pred_length=False):
                output = self.model(inputs, "test")
                # train.py:229-230: the pictures of the last batch's prediction -- taken here, before the training-mode forward below
                # reuses the buffers `output` views
                if self.log_images and i_val == n_val - 1 and not getattr(self.cmd_args, "metric", False):
                    self.image_files += self.model.log_outputs(output, inputs, None, self.global_step, True, "val")
                if i_val == 0 and getattr(self.cmd_args, "metric", False) and self.model.topdown_assets is not None \
                        and not self.cmd_args.dont_save:
                    from .image_log import write_metric_trajectories   # compute_metrics.py:225-226: the first sequences on the map
                    self.image_files += write_metric_trajectories(self.model, inputs, self.exp_path, self.global_step)
                if self.evaluator is not None:         # train.py:208-209: every batch, prior samples of the model's own noise stream
                    self.evaluator.eval(inputs, output, self.model)
            out = self.model(inputs)
            losses = self.model.loss(inputs, out)
            tot += float(self.model.get_total_loss(inputs, losses).value)
            n += 1
            if slog is not None:                       # train.py:203,214: the meter of every term, kept on the device
                term_names = [k for k in losses if k != "_total"]
                vec = torch.stack([losses[k].value.reshape(()) for k in term_names])
                term_sum = vec if term_sum is None else term_sum + vec
        avg = tot / max(n, 1)
        self.last_val = avg
        if slog is not None and n and not getattr(self.cmd_args, "metric", False):
            # train.py:229-230: the averages, once, at global_step; the layer-wise KL is the last batch's (its posterior forward `out`)
            avg_terms = dict(zip(term_names, (term_sum / n).unbind(0)))
            avg_terms["_total"] = avg
            self.model.log_outputs(out, inputs, avg_terms, self.global_step, False, "val")
            slog.dump_scalars()
        if self.evaluator is not None:
            self.dump_results()
            if self.cmd_args.metric:
                if self.rank == 0:
                    print("Finished Evaluation! Exiting...", flush=True)
                return avg
        if self.rank == 0:
            print("\nTest set: Average loss: {:.4f} in {:.2f}s\n".format(avg, time.time() - start), flush=True)
        return avg


    # ---- train.py:217-219, compute_metrics.py:143-150: the evaluation of this validation, gathered on rank 0 and written there ----
    def dump_results(self):
        from .evaluation import gather_evaluation, write_results
        ev = self.evaluator.collected()
        self.evaluator.reset()
        if ev is None or self.cmd_args.dont_save:
            return None
        pg = torch.distributed.group.WORLD if self.world > 1 else None
        ev = gather_evaluation(ev, self.model._hp.batch_size, pg)
        if self.rank != 0:
            return None
        return write_results(self.exp_path, self.global_step, ev, top_of_100=self.evaluator._top_of_100)


if __name__ == "__main__":
    ModelTrainer().run()
