#!/usr/bin/env python
"""bench.py — predicted frames/sec of the gcp_tree hot path on MI355X (BASELINE.json metric).

One "step" = one forward pass of the goal-conditioned hierarchical predictor over one synthetic batch of
BASELINE.json configs[1] (25-room gcp_tree, 64x64x3, seq_len 80, batch 16 per GPU): encoder over B*T frames,
L=7 tree levels (posterior path), decoder over all B*127 tree nodes, balanced binding + matched/pruned gathers
and the auxiliary heads — everything `model(inputs)` runs (train.py:205-214 / cem_simulator.py:29-31).
Inputs are resident in HBM before the timed region.  Rank 0 prints ONE JSON line.

A plain run measures the headline only (with the head kernel's roofline, read from events inside the timed steps).  `--full`
adds what takes runs of its own: the secondary workloads under "also" (training step, planning, adaptive and sequential models,
graph / eager replay legs) and the CPU baseline.  `--dump-outputs DIR` writes what the last timed step returned as DIR/<name>.npy.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

F32_MFMA_PEAK_TFLOPS = 157.3      # /opt/skills/guides/MI355X_MICROARCH.md: v_mfma_f32_16x16x4_f32, 256 CUs @ 2.4 GHz
F16_MFMA_PEAK_TFLOPS = 2500.0     # same table: dense f16 / bf16 MFMA (no sparsity)
PMC_SUMMARY = os.path.join(ROOT, "profiles", "pmc_head_kernel.json")
HEAD_KERNEL_SOURCES = ("video-gcp_amd/csrc/conv3x3.hip", "video-gcp_amd/csrc/conv3x3_head_split.hip", "video-gcp_amd/csrc/split_mfma.h",
                       "video-gcp_amd/csrc/split_common.h", "video-gcp_amd/csrc/common.h")


def kernel_source_sha(paths=HEAD_KERNEL_SOURCES):
    import hashlib
    h = hashlib.sha256()
    for p in paths:
        with open(os.path.join(ROOT, p), "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def measured_head_traffic(batch, eval_bn):
    """HBM bytes per launch of the head kernel from the rocprofv3 PMC passes of tools/pmc_collect.sh (FETCH_SIZE x 2 for the
    gfx950 wide-load undercount + WRITE_SIZE, MI355X_MICROARCH.md "HBM"), valid only for the kernel sources they were taken on:
    the summary records a hash of those sources, and a mismatch (kernel edited since) or another workload prints null — with the
    reason on stderr, so a regenerated summary that lost a field does not make `roofline.traffic` disappear silently."""
    def reject(why):
        print(f"bench: roofline.traffic = null ({PMC_SUMMARY}: {why})", file=sys.stderr, flush=True)
        return None, None
    try:
        with open(PMC_SUMMARY) as f:
            d = json.load(f)
        if d.get("kernel_src_sha") != kernel_source_sha():
            return reject(f"taken on kernel sources {d.get('kernel_src_sha')}, these are {kernel_source_sha()}")
        if d.get("batch") != batch or bool(d.get("eval_bn")) != bool(eval_bn):
            return reject(f"taken at batch {d.get('batch')}, eval_bn {d.get('eval_bn')}")
        if not d.get("with_loss"):          # the headline forward keeps the matched frames' raw parameters (a round-2 pass did not)
            return reject("no `with_loss` field: not a pass over the forward with losses")
        return int(d["traffic_bytes_per_launch"]), d.get("round")
    except (OSError, KeyError, ValueError) as e:
        return reject(repr(e))


def _stats(ts):
    ts = sorted(ts)
    return {"median_s": round(ts[len(ts) // 2], 4), "min_s": round(ts[0], 4), "iters": len(ts)}


def _time_region(fn, budget_s, warmup, min_iters, max_iters):
    for _ in range(warmup):
        fn()
    ts, t_all = [], time.perf_counter()
    while len(ts) < max_iters and (len(ts) < min_iters or time.perf_counter() - t_all < budget_s):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
        if time.perf_counter() - t_all > budget_s and len(ts) >= min_iters:
            break
    return ts


def cpu_baseline(budget_s=24.0, full=False, schedule=None):
    """The CPU oracle (a port: the reference itself cannot run, SURVEY.md F3 / BASELINE.md section 2) on the host cores.
    Default: a BOUNDED sample of the headline workload — c2 shapes at batch 2, inference forward and one training step
    (zero_grad -> forward -> loss -> backward -> RAdam, the region of train.py:155-164) with all threads, plus the c1 plumbing
    config with 1 thread and all threads.  full=True runs BASELINE.md section 2's protocol (3 warm-up + 10 timed, threads 1 and all,
    c1 and c2 at B=16, forward + planning rollout + training step; hours on one thread); tools/cpu_baseline_full.py runs a stated
    reduction of it through `schedule` and its output is committed under profiles/."""
    import platform
    import torch
    import video_gcp_amd as V
    from oracle import gcp_model_oracle as O
    from oracle.radam_oracle import RAdamOracle
    from helpers import make_inputs
    all_threads = torch.get_num_threads()
    cpu = platform.processor() or ""
    try:
        with open("/proc/cpuinfo") as f:
            cpu = [l.split(":", 1)[1].strip() for l in f if l.startswith("model name")][0]
    except (OSError, IndexError):
        pass

    def regions(cfg, batch):
        hp = V.config(cfg, batch_size=batch)
        sd = V.init_params(hp, seed=0)
        inputs, noise, z = make_inputs(hp, seed=0, variant="A")
        plan_in = dict({k: inputs[k] for k in ("I_0", "I_g", "end_ind", "start_ind")}, z=z)
        opt = RAdamOracle(lr=2e-4)
        theta = {k: v.clone() for k, v in sd.items()}

        def fwd():
            with torch.no_grad():
                O.forward(sd, hp, inputs, noise=noise, training_bn=True)

        def rollout():
            with torch.no_grad():
                O.forward(sd, hp, plan_in, sample_prior=True, training_bn=False)

        def train():
            g, _, _, _ = O.gradients(theta, hp, inputs, noise)
            opt.step(theta, g)
        return hp, {"forward": fwd, "planning_rollout": rollout, "train_step": train}

    out = {"cores": all_threads, "kind": "port", "unit": "frames/s", "cpu": cpu, "torch": torch.__version__, "runs": []}
    if schedule is not None:
        sched = schedule
    elif full:
        sched = [(cfg, b, k, r, 3, 10, 10, 1e9) for cfg, b in (("c1", 2), ("c2", 16)) for k in (1, all_threads)
                 for r in ("forward", "planning_rollout", "train_step")]
    else:
        # bounded default (about 40 s): the headline region (c2 shapes, batch 2, inference forward) at 1 / 16 / all threads with
        # BASELINE.md section 2's 3 warm-up + 10 timed iterations (the all-thread run is oversubscribed on this oracle and slower: 3 + 4),
        # then one training step (3 + 3: a step is ~1.5 s) and the c1 plumbing config at the thread count that came out best
        mid = min(16, all_threads)
        sched = [("c2", 2, 1, "forward", 3, 10, 10, 1e9), ("c2", 2, mid, "forward", 3, 10, 10, 1e9),
                 ("c2", 2, all_threads, "forward", 3, 4, 4, 1e9)]
        tail = lambda k: [("c2", 2, k, "train_step", 3, 3, 3, 1e9), ("c1", 2, k, "forward", 3, 10, 10, 1e9),
                          ("c1", 2, k, "train_step", 3, 10, 10, 1e9)]
    cache = {}

    def run(item):
        cfg, b, k, region, warm, mn, mx, bud = item
        if (cfg, b) not in cache:
            cache[(cfg, b)] = regions(cfg, b)
        hp, fns = cache[(cfg, b)]
        torch.set_num_threads(k)
        st = _stats(_time_region(fns[region], bud, warm, mn, mx))
        st.update(config=cfg, batch=b, threads=k, region=region,
                  frames_per_s=round(hp.batch_size * hp.max_seq_len / st["median_s"], 2))
        out["runs"].append(st)

    def best_forward():
        return max((r for r in out["runs"] if r["config"] == "c2" and r["region"] == "forward"), key=lambda r: r["frames_per_s"])

    try:
        for item in sched:
            run(item)
        if schedule is None and not full:
            for item in tail(best_forward()["threads"]):
                run(item)
    finally:
        torch.set_num_threads(all_threads)
    # `value` = the BEST CPU configuration timed for the headline region (more threads are not faster on this oracle: its tree
    # levels are small GEMMs), `cores` = the threads that run used
    head = best_forward()
    out["value"] = head["frames_per_s"]
    out["cores"] = head["threads"]
    out["host_threads"] = all_threads
    # the sample's configuration, said where the number is: the metric's config is c2 at batch 16, the bounded in-run sample is batch 2
    out["config"] = f"c2 B={head['batch']}" + (" (bounded sample; the metric's configuration is c2 B=16)" if head["batch"] != 16 else "")
    if not full and schedule is None:
        # BASELINE.md section 2's protocol at the metric's own configuration (c2, B = 16) — too long for a bench run, committed from the same
        # CPU model: quoted next to the sample, marked as not measured here
        try:
            with open(os.path.join(ROOT, "profiles", "r05_cpu_baseline_full.json")) as f:
                fullp = json.load(f)
            rows = [r for r in fullp["runs"] if r["config"] == "c2" and r["batch"] == 16 and r["region"] == "forward"]
            if rows and fullp.get("cpu") == cpu:
                best = max(rows, key=lambda r: r["frames_per_s"])
                out["metric_config"] = {"config": "c2 B=16", "value": best["frames_per_s"], "cores": best["threads"], "unit": "frames/s",
                                        "source": "profiles/r05_cpu_baseline_full.json: same CPU model, same oracle, 3 warm-up + 10 timed; "
                                                  "NOT measured in this run"}
        except (OSError, KeyError, ValueError):
            pass
    out["sample"] = (f"oracle/gcp_model_oracle.py (torch {torch.__version__} CPU fp32) at c2 shapes (64x64, T=80, 127 nodes/seq) with batch "
                     f"{head['batch']}: median of {head['iters']} forward passes on {head['threads']} of {all_threads} hardware threads "
                     "(the fastest of the thread counts in `runs`, which lists every timed region: config, batch, threads, forward / "
                     "training step, median and min seconds)"
                     + ("" if (full or schedule) else "; bounded sample (3 warm-up iterations per region) — BASELINE.md section 2's protocol at "
                        "c1 and c2, B = 16, on this round's GPU box: profiles/r05_cpu_baseline_full.json"))
    return out


def _timed(fn, steps, warmup, world, dev):
    """barrier + sync on both sides, max over ranks (same rule as the headline measurement)"""
    import torch
    import torch.distributed as dist
    from video_gcp_amd import dist as D
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    return D.max_over_ranks(time.perf_counter() - t0, device=dev) / steps


DUMP_SAMPLE = 1 << 20           # elements kept of a larger output: a fixed, seeded sample of its flat positions
DUMP_LIMIT = 64 << 20           # bytes written in all


def dump_outputs(out, losses, path):
    """--dump-outputs: what a caller of the timed path holds after its last step — `model(inputs)` (decoded node frames, the tree's
    latents, the auxiliary heads' outputs, the pruned prediction) and `model.loss()` — as <path>/<name>.npy.  The inputs and the seed
    of the in-step noise are fixed: the same arguments give the same numbers.  Floating outputs are float32 (float64 stays float64),
    integer ones float64.  An output of more than DUMP_SAMPLE elements is written as the elements at DUMP_SAMPLE positions drawn from
    a generator seeded with 0 (same positions for the same size), sorted."""
    import numpy as np
    import torch
    arrays = {}

    def put(name, t):
        if not isinstance(t, torch.Tensor):
            return
        t = t.detach()
        t = t.float() if t.is_floating_point() and t.dtype != torch.float64 else t.double()
        n = t.numel()
        if n > DUMP_SAMPLE:
            idx = np.unique(np.random.default_rng(0).integers(0, n, size=DUMP_SAMPLE))
            t = t.reshape(-1).index_select(0, torch.from_numpy(idx).to(t.device))
        arrays[name] = t.cpu().numpy()

    put("images_df", out.images_df)
    for k in ("z", "p_z_mu", "p_z_log_sigma", "q_z_mu", "q_z_log_sigma", "e_g_prime", "hidden_state", "match_timesteps"):
        put("tree.df." + k, out.tree.df[k])
    for k in ("seq_len_logits", "soft_matched_estimates"):
        put(k, out.get(k))
    if "existence_predictor" in out:
        put("existence_predictor.existence", out.existence_predictor.existence)
    for k in ("model_enc_seq", "regressed_state", "actions", "cost", "cost_target"):
        put(k, getattr(out, k, None))
    put("pruned_prediction", torch.cat(list(out.pruned_prediction), 0))
    for k, v in losses.items():
        put("loss." + k.lstrip("_"), v.value if isinstance(v, dict) else v)
    total = sum(a.nbytes for a in arrays.values())
    assert total <= DUMP_LIMIT, f"--dump-outputs: {total} bytes, more than {DUMP_LIMIT}"
    os.makedirs(path, exist_ok=True)
    for k, a in arrays.items():
        np.save(os.path.join(path, k + ".npy"), a)


def extras(args, model, hp, dinp, dnoise, inputs, rank, world, dev, dinp_noloss):
    """Secondary measurements of SURVEY.md §8(d): (iii) training step (forward + backward + RAdam, RCCL all-reduce of the
    flat gradient when N > 1), (ii) one CEM planning iteration over 512 candidates sharded over the ranks, and the
    adaptive-binding forward of configs[4].  Each is whole-job predicted frames/s; failures are reported, not hidden."""
    import numpy as np
    import torch
    import torch.distributed as dist
    import video_gcp_amd as V
    from video_gcp_amd import dist as D
    from video_gcp_amd.model import GCPTreeModel
    from helpers import make_inputs
    res = {}
    k = max(3, min(args.steps, 10))
    model.set_timed_op(None)

    def agree(ok):
        """Every block first builds its model / trainer and runs one un-timed call WITHOUT collectives; the ranks then agree
        (all-reduce MIN of a flag) whether to enter the timed region, which contains collectives: a rank that failed in set-up
        (out of memory, a status error) must not leave the others waiting in an all-reduce."""
        if world == 1:
            return ok
        t = torch.tensor([1 if ok else 0], device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MIN)
        return bool(t.item())

    def setup(fn):
        try:
            return fn(), None
        except Exception as e:  # noqa: BLE001
            return None, repr(e)[:300]

    # round-2 headline for continuity: the same forward WITHOUT loss inputs (mean-only head: 80 of the 100 mixture channels)
    try:
        _, err = setup(lambda: model(dinp_noloss, "train"))
        if not agree(err is None):
            raise RuntimeError(err or "set-up failed on another rank")
        dt = _timed(lambda: model(dinp_noloss, "train"), k, 2, world, dev)
        res["forward_no_loss"] = {"value": round(world * hp.batch_size * hp.max_seq_len / dt, 1), "unit": "frames/s",
                                  "ms_per_step": round(1e3 * dt, 3),
                                  "workload": "posterior forward without pad_mask: no loss kernels, head computes the 80 channels the mixture "
                                              "mean reads (the round-2 headline; an inference forward no reference entry point runs)"}
    except Exception as e:  # noqa: BLE001
        res["forward_no_loss"] = {"error": repr(e)[:300]}
    # the planner's rollout (cem_simulator.py:29-31): eval-mode (running-stat BatchNorm) prior path with given latents z
    was = model.training
    try:
        model.eval()
        zin = dict(I_0=dinp["I_0"], I_g=dinp["I_g"], end_ind=dinp["end_ind"], start_ind=dinp["start_ind"],
                   z=torch.randn(hp.batch_size, hp.n_nodes, hp.nz_vae, device=dev))

        def rollout():
            with model.val_mode(pred_length=False):
                model(zin, "train")
        _, err = setup(rollout)
        if not agree(err is None):
            raise RuntimeError(err or "set-up failed on another rank")
        dt = _timed(rollout, k, 2, world, dev)
        res["planning_rollout"] = {"value": round(world * hp.batch_size * hp.max_seq_len / dt, 1), "unit": "frames/s",
                                   "ms_per_step": round(1e3 * dt, 3),
                                   "workload": "eval-mode planner rollout at the headline batch: prior path with given z, running-stat "
                                               "BatchNorm, every node decoded (mean-only head), no trajectory encoder"}
    except Exception as e:  # noqa: BLE001
        res["planning_rollout"] = {"error": repr(e)[:300]}
    finally:
        model.train(was)              # the exact-f32 leg below must run with the headline's batch-stat BatchNorm whatever happened here
    if model.split_f16 and model.pk_split:
        # the same forward with every conv on the exact f32 MFMA kernels (GCPX_EXACT_F32=1), for comparison
        try:
            model.split_f16 = False
            model._clear_plans()
            dt = _timed(lambda: model(dinp, "train"), k, 2, world, dev)
            res["forward_exact_f32"] = {"value": round(world * hp.batch_size * hp.max_seq_len / dt, 1), "unit": "frames/s",
                                        "ms_per_step": round(1e3 * dt, 3),
                                        "workload": "the headline forward (with losses) with the split-f16 convs switched off (GCPX_EXACT_F32=1): "
                                                    "exact f32 MFMA kernels throughout"}
        except Exception as e:  # noqa: BLE001
            res["forward_exact_f32"] = {"error": repr(e)[:300]}
        finally:
            model.split_f16 = True
            model._clear_plans()
    try:
        from video_gcp_amd.training import GCPTrainStep
        full = {k_: v.to(dev) for k_, v in inputs.items()}
        tr, err = setup(lambda: GCPTrainStep(model, process_group=(dist.group.WORLD if world > 1 else None)))
        if not agree(err is None):
            raise RuntimeError(err or "set-up failed on another rank")
        dt = _timed(lambda: tr.step(full), k, 2, world, dev)
        res["train_step"] = {"value": round(world * hp.batch_size * hp.max_seq_len / dt, 1), "unit": "frames/s",
                             "ms_per_step": round(1e3 * dt, 3), "workload": "configs[2] shard: forward + ELBO losses + backward + "
                             "RAdam, batch 16/GPU" + (", bucketed RCCL all-reduce of the flat fp32 gradient overlapped with the backward" if world > 1 else ""),
                             "grad_mbytes": round(tr.grad.numel() * 4 / 1e6, 1)}
        if world > 1 and tr.buckets is not None:
            # what the scaling curve is made of: the collectives' own time on the communication stream, bucket by bucket (in-region
            # events of one more step), next to ONE all-reduce of the whole flat gradient with nothing else running
            tr.buckets.timing = True
            tr.step(full)
            torch.cuda.synchronize()
            per = tr.buckets.comm_ms()
            tr.buckets.timing = False
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            dist.barrier()
            torch.cuda.synchronize()
            e0.record()
            for _ in range(3):
                dist.all_reduce(tr.grad)
            e1.record()
            torch.cuda.synchronize()
            flat_ms = D.max_over_ranks(e0.elapsed_time(e1) / 3, device=dev)
            tr.grad.zero_()
            res["train_step"]["allreduce"] = {"buckets_ms_in_step": {k_: round(v, 3) for k_, v in per.items()},
                                              "buckets_ms_sum": round(sum(per.values()), 3), "flat_gradient_alone_ms": round(flat_ms, 3),
                                              "note": "buckets_ms_in_step: event pairs on the communication stream around every bucket's "
                                                      "all-reduce inside one training step (rank 0; includes waiting for the slowest rank); "
                                                      "flat_gradient_alone_ms: one all-reduce of the whole gradient on an idle device, max over ranks"}
        del tr
    except Exception as e:  # noqa: BLE001
        res["train_step"] = {"error": repr(e)[:300]}
    try:
        from video_gcp_amd.planning import GCPImageSimulator, LearnedCostEstimate, SimpleTreeCEMSampler, CEMPlanner
        hp4 = V.config("c4")
        m4 = GCPTreeModel(hp4, params=V.init_params(hp4, seed=0), device=dev)
        m4.eval()
        rng = np.random.RandomState(0)
        state = rng.randint(0, 256, size=(1, hp4.img_sz, hp4.img_sz, 3)).astype(np.uint8)
        goal = rng.randint(0, 256, size=(1, hp4.img_sz, hp4.img_sz, 3)).astype(np.uint8)
        n = 512
        sampler = SimpleTreeCEMSampler(float("inf"), None, hp4.nz_vae, 1.0, n_level_hierarchy=hp4.hierarchy_levels, device=dev, seed=1)
        planner = CEMPlanner(GCPImageSimulator(m4, pred_length=False), LearnedCostEstimate(m4), sampler, n_iters=1, batch_size=n, elite_frac=0.1,
                             max_seq_len=hp4.max_seq_len)
        _, err = setup(lambda: m4.encode(torch.zeros(1, 3, hp4.img_sz, hp4.img_sz, device=dev)))
        if not agree(err is None):
            raise RuntimeError(err or "set-up failed on another rank")

        def it():
            planner.iterate(state, goal)       # draw (each rank its own shard), roll out, score, all-gather, elites, refit
        # reference-equivalent work first: every candidate's 80 frames are decoded while scoring (cem_simulator.py:29-59) ...
        planner.decode_candidates = True
        dt_all = _timed(it, 3, 1, world, dev)
        # ... then the default: the learned cost reads latents only, so scoring skips the decoder (same scores, elites and plan;
        # tests/test_gpu_planning.py) and only the returned plan is decoded
        planner.decode_candidates = False
        dt = _timed(it, 3, 1, world, dev)
        res["planning_iteration"] = {"value": round(n * hp4.max_seq_len / dt_all, 1), "unit": "frames/s",
                                     "ms_per_iteration": round(1e3 * dt_all, 2), "candidates_per_s": round(n / dt_all, 1),
                                     "workload": "configs[3]: one CEM iteration, 512 candidates x horizon 80 sharded over the ranks, "
                                     "every candidate decoded (reference-equivalent work), rollout + learned cost on device, one "
                                     "all-gather of costs",
                                     "latent_scoring": {"ms_per_iteration": round(1e3 * dt, 2), "candidates_per_s": round(n / dt, 1),
                                                        "note": "planner default: candidates scored on latents, decoder skipped while "
                                                                "scoring (bit-identical scores / elites / plan); only the returned plan "
                                                                "is decoded"}}
        del planner, m4
    except Exception as e:  # noqa: BLE001
        res["planning_iteration"] = {"error": repr(e)[:300]}
    try:
        hp5 = V.config("c5")
        m5 = GCPTreeModel(hp5, params=V.init_params(hp5, seed=0), device=dev)
        i5, n5, _ = make_inputs(hp5, seed=200 + rank, variant="A")
        d5 = {k_: v.to(dev) for k_, v in i5.items()}
        n5 = n5.to(dev)
        _, err = setup(lambda: m5(d5, "train", noise=n5))
        if not agree(err is None):
            raise RuntimeError(err or "set-up failed on another rank")
        dt = _timed(lambda: m5(d5, "train", noise=n5), k, 2, world, dev)
        res["adaptive_forward"] = {"value": round(world * hp5.batch_size * hp5.max_seq_len / dt, 1), "unit": "frames/s",
                                   "ms_per_step": round(1e3 * dt, 3), "workload": "configs[4] shard: adaptive (soft-DTW) binding + "
                                   "attentive inference forward with losses, 64x64, seq_len 200, L=8 (255 nodes), batch 8/GPU"}
        from video_gcp_amd.training import GCPTrainStep
        tr5, err = setup(lambda: GCPTrainStep(m5, process_group=(dist.group.WORLD if world > 1 else None)))
        if not agree(err is None):
            raise RuntimeError(err or "set-up failed on another rank")
        dt = _timed(lambda: tr5.step(d5, n5), max(3, k // 2), 2, world, dev)
        res["adaptive_train_step"] = {"value": round(world * hp5.batch_size * hp5.max_seq_len / dt, 1), "unit": "frames/s",
                                      "ms_per_step": round(1e3 * dt, 3), "workload": "configs[4] shard: forward + losses + backward "
                                      "+ RAdam of the adaptive model, batch 8/GPU" + (", RCCL all-reduce of the flat gradient" if world > 1 else "")}
        del tr5, m5
    except Exception as e:  # noqa: BLE001
        res["adaptive_forward"] = {"error": repr(e)[:300]}
    try:
        from video_gcp_amd.sequential import GCPSequentialModel
        ms_ = GCPSequentialModel(hp, device=dev)
        dseq = {k_: dinp[k_] for k_ in ("traj_seq", "I_0", "I_g", "end_ind", "start_ind", "pad_mask")}
        _, err = setup(lambda: ms_(dseq, "train"))
        if not agree(err is None):
            raise RuntimeError(err or "set-up failed on another rank")
        dt = _timed(lambda: ms_(dseq, "train"), k, 2, world, dev)
        res["sequential_forward"] = {"value": round(world * hp.batch_size * hp.max_seq_len / dt, 1), "unit": "frames/s",
                                     "ms_per_step": round(1e3 * dt, 3),
                                     "workload": "flat VRNN baseline gcp_sequential (sequential.py:13-131) at the headline shapes: posterior "
                                                 "rollout over 79 steps + decoder + losses"}
        if hasattr(ms_, "_has_training") and ms_._has_training:
            from video_gcp_amd.training_sequential import SequentialTrainStep
            trs, err = setup(lambda: SequentialTrainStep(ms_, process_group=(dist.group.WORLD if world > 1 else None)))
            if not agree(err is None):
                raise RuntimeError(err or "set-up failed on another rank")
            fulls = {k_: v.to(dev) for k_, v in inputs.items()}
            dt = _timed(lambda: trs.step(fulls), max(3, k // 2), 2, world, dev)
            res["sequential_train_step"] = {"value": round(world * hp.batch_size * hp.max_seq_len / dt, 1), "unit": "frames/s",
                                            "ms_per_step": round(1e3 * dt, 3),
                                            "workload": "gcp_sequential: forward + losses + backward through the 79-step recurrence + RAdam"}
            del trs
        del ms_
        if hasattr(GCPSequentialModel, "_has_training"):
            # the reference's own gcp_sequential conf runs 1024-wide LSTMs (experiments/prediction/25room/gcp_sequential/conf.py)
            from video_gcp_amd.training_sequential import SequentialTrainStep
            hpw = V.config("c2", batch_size=hp.batch_size, nz_mid_lstm=1024)
            msw = GCPSequentialModel(hpw, device=dev)
            _, err = setup(lambda: msw(dseq, "train"))
            if not agree(err is None):
                raise RuntimeError(err or "set-up failed on another rank")
            dtf = _timed(lambda: msw(dseq, "train"), max(3, k // 2), 2, world, dev)
            trw, err = setup(lambda: SequentialTrainStep(msw, process_group=(dist.group.WORLD if world > 1 else None)))
            if not agree(err is None):
                raise RuntimeError(err or "set-up failed on another rank")
            fullw = {k_: v.to(dev) for k_, v in inputs.items()}
            dtt = _timed(lambda: trw.step(fullw), max(3, k // 2), 2, world, dev)
            res["sequential_1024"] = {"forward_ms": round(1e3 * dtf, 3), "train_step_ms": round(1e3 * dtt, 3),
                                      "train_frames_per_s": round(world * hp.batch_size * hp.max_seq_len / dtt, 1),
                                      "workload": "gcp_sequential with nz_mid_lstm = 1024 (the reference conf's width), otherwise the headline shapes"}
            del trw, msw
    except Exception as e:  # noqa: BLE001
        res["sequential_forward"] = {"error": repr(e)[:300]}
    try:
        from video_gcp_amd.planning import GCPImageSimulator, LearnedCostEstimate, HierarchicalCEMPlanner
        hp4 = V.config("c4")
        m4 = GCPTreeModel(hp4, params=V.init_params(hp4, seed=0), device=dev)
        m4.eval()
        rng = np.random.RandomState(0)
        state = rng.randint(0, 256, size=(1, hp4.img_sz, hp4.img_sz, 3)).astype(np.uint8)
        goal = rng.randint(0, 256, size=(1, hp4.img_sz, hp4.img_sz, 3)).astype(np.uint8)
        sim4, cost4 = GCPImageSimulator(m4, pred_length=False), LearnedCostEstimate(m4)

        def time_planner(**kw):
            hplanner = HierarchicalCEMPlanner(sim4, cost4, hp4.hierarchy_levels, [10, 10], action_dim=hp4.nz_vae, max_seq_len=hp4.max_seq_len, **kw)
            _, err = setup(lambda: hplanner(state, goal))
            if err is not None:
                raise RuntimeError(err)
            torch.cuda.synchronize()
            ts = []
            for _ in range(5):               # a call is ~7 ms of mostly host-paced work: the MEDIAN of five calls (one call in ~20 is 2x
                t0 = time.perf_counter()     # longer — a plan key's one-time replay tuning or the host — and would double a mean of three)
                hplanner(state, goal)
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
            return sorted(ts)[len(ts) // 2]
        dt_ref, dt_fast = time_planner(), time_planner(fast_draws=True)
        res["hierarchical_planner_call"] = {"ms_per_call": round(1e3 * dt_fast, 2), "ms_per_call_reference_rng_stream": round(1e3 * dt_ref, 2),
                                            "unit": "ms",
                                            "workload": "HierarchicalCEMPlanner (tree_optimizer.py:7-260; sampling rates [10, 10], the 25-room "
                                                        "control setting) for one (start, goal) pair at 64x64, horizon 80: device-resident, "
                                                        "per-rank (not sharded); median of five calls.  ms_per_call: fast_draws=True (seeded device generator, only the "
                                                        "rows the search keeps are drawn); ms_per_call_reference_rng_stream: the reference's "
                                                        "np.random call sequence draw for draw (3.5 M legacy Gaussians per call on the host)"}
        del m4
    except Exception as e:  # noqa: BLE001
        res["hierarchical_planner_call"] = {"error": repr(e)[:300]}
    torch.cuda.empty_cache()
    return res


def self_launch(n):
    """`python bench.py --gpus N` without a launcher: one child process per GPU (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* in its
    environment, same command line), started BEFORE this process makes any GPU call — it never imports torch — so nothing that
    has initialised the GPU is ever re-executed.  Rank 0's stdout (the one JSON line) is relayed; the exit status is the worst
    child's, and when one rank dies the others are terminated by PID instead of waiting in a collective for ever."""
    import socket
    import subprocess
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=(subprocess.PIPE if r == 0 else subprocess.DEVNULL), text=(r == 0)))
    import threading
    relay = threading.Thread(target=lambda: [sys.stdout.write(l) or sys.stdout.flush() for l in procs[0].stdout], daemon=True)
    relay.start()
    rc = 0
    live = list(procs)
    while live:
        time.sleep(0.05)
        for p in list(live):
            c = p.poll()
            if c is None:
                continue
            live.remove(p)
            if c != 0:
                rc = rc or c
                for q in live:                       # the surviving ranks would block in their next collective
                    q.terminate()
    relay.join(10)
    return rc


def launch_check(args):
    """what a multi-rank bench run needs besides the GPU work: rendezvous, barrier, max-over-ranks timing, a gather"""
    import torch
    import torch.distributed as dist
    from video_gcp_amd import dist as D
    rank, _, world = D.init_from_env(args.backend)
    if rank == args.fail_rank:
        return 3
    D.barrier()
    slow = D.max_over_ranks(1.0 + rank)
    ranks = [None] * world
    if world > 1:
        dist.all_gather_object(ranks, rank)
    else:
        ranks = [0]
    if rank == 0:
        print(json.dumps({"launch_check": True, "n_gpus": world, "ranks": ranks, "slowest_rank_s": slow, "backend": args.backend}), flush=True)
    if world > 1:
        dist.destroy_process_group()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16, help="sequences per GPU (configs[1]: 16)")
    ap.add_argument("--eval-bn", action="store_true", help="running-stat BatchNorm (planner mode) instead of batch stats")
    ap.add_argument("--full", action="store_true", help="also run the secondary measurements (\"also\": replay legs, training "
                    "step, CEM planning, adaptive and sequential models) and the CPU baseline; a plain run times the headline only")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write what the last timed step returned as DIR/<name>.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-extras", action="store_true", help="with --full: skip the secondary measurements (training step, CEM "
                    "planning iteration, adaptive-binding forward) reported under \"also\"")
    ap.add_argument("--backend", default="nccl", help='torch.distributed backend of the ranks ("nccl" = RCCL; "gloo" for --launch-check on CPU)')
    ap.add_argument("--launch-check", action="store_true", help="rendezvous + barrier + max-over-ranks only, no GPU work (tests)")
    ap.add_argument("--fail-rank", type=int, default=-1, help=argparse.SUPPRESS)
    ap.add_argument("--cpu-baseline-full", action="store_true", help="BASELINE.md section-2 protocol for the CPU baseline (slow)")
    args = ap.parse_args()

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(args.gpus))
    if args.launch_check:
        sys.exit(launch_check(args))

    import torch
    import torch.distributed as dist
    import video_gcp_amd as V
    from video_gcp_amd.model import GCPTreeModel
    from helpers import make_inputs

    from video_gcp_amd import dist as D
    if args.gpus > 1:
        assert int(os.environ["WORLD_SIZE"]) == args.gpus, f"WORLD_SIZE={os.environ['WORLD_SIZE']} but --gpus {args.gpus}"
        rank, local_rank, world = D.init_from_env(args.backend, timeout_s=300)      # "nccl" is RCCL on ROCm
    else:
        rank, local_rank, world = 0, 0, 1
        torch.cuda.set_device(0)
    dev = torch.device("cuda", torch.cuda.current_device())

    hp = V.config("c2", batch_size=args.batch)
    model = GCPTreeModel(hp, params=V.init_params(hp, seed=0), device=dev)      # same seed on every rank = replicas
    model.train(not args.eval_bn)
    # the path shards by sequence: every rank predicts its own batch of independent sequences (weak scaling), no
    # data-path collective in the forward
    inputs, noise, _ = make_inputs(hp, seed=D.shard_seed(100, rank), variant="A")
    # headline = the reference's posterior forward WITH its loss (train.py:157-159 / :205-214: every caller of the posterior path
    # also calls model.loss): pad_mask, states and actions are fed, so the head computes all 100 mixture channels for the matched
    # frames and the ELBO / auxiliary loss kernels run inside the timed graph.
    # the synthetic batch is written ONCE, before the timed region, into the model's own input buffers (what a device-side
    # loader does): the forward then reads it in place instead of staging a 63 MB copy per call
    dinp = {}
    for k in ("traj_seq", "I_0", "I_g", "end_ind", "start_ind", "pad_mask", "traj_seq_states", "actions"):
        buf = model.input_buffer(k, inputs[k].shape) if k != "start_ind" else inputs[k].to(dev)
        buf.copy_(inputs[k])
        dinp[k] = buf
    dnoise = noise.to(dev)
    dinp_noloss = {k: dinp[k] for k in ("traj_seq", "I_0", "I_g", "end_ind", "start_ind")}

    # the latent noise is DRAWN inside every timed step (noise=None: Gaussian.sample() of the reference draws per forward), not fed;
    # its stream starts from torch's CUDA seed, which torch draws at random per process unless seeded: seeded per rank, so that runs
    # with the same arguments compute the same outputs (--dump-outputs)
    torch.manual_seed(D.shard_seed(0, rank))
    for _ in range(max(args.warmup, 1)):
        model(dinp, "train")
    torch.cuda.synchronize()

    model.set_timed_op("dec.head")
    model(dinp, "train")          # builds the split graphs
    torch.cuda.synchronize()
    model.timed_op_ms()

    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = model(dinp, "train")
        losses = model.loss(dinp, out)                 # device scalars computed inside the graph: no kernel, no sync
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    head_ms = model.timed_op_ms()
    elapsed = D.max_over_ranks(elapsed, device=dev)
    total_loss = float(model.get_total_loss(dinp, losses).value)
    replay = model.replay_info()
    if args.dump_outputs and rank == 0:
        dump_outputs(out, losses, args.dump_outputs)      # before any later call overwrites the plan's output buffers

    def replay_leg(mode):
        """the headline step (forward + loss, no events around the head) with every plan forced onto one way of replaying, same process"""
        model.set_timed_op(None)
        model.force_replay(mode)

        def step():
            o = model(dinp, "train")
            model.loss(dinp, o)
        step()
        dt = _timed(step, args.steps, 2, world, dev)
        return {"ms_per_step": round(1e3 * dt, 3), "value": round(world * hp.batch_size * hp.max_seq_len / dt, 1), "unit": "frames/s"}
    replay_legs = None
    if args.full and not args.no_extras:
        replay_legs = {"forward_graph": replay_leg("graph"), "forward_eager": replay_leg("eager")}
        model.force_replay("auto")

    also = None
    if args.full and not args.no_extras:
        also = extras(args, model, hp, dinp, dnoise, inputs, rank, world, dev, dinp_noloss)
        also = dict(replay_legs, **also)

    if rank == 0:
        frames = world * hp.batch_size * hp.max_seq_len * args.steps
        value = frames / elapsed
        F = hp.batch_size * hp.n_nodes
        split = model.split_f16 and "dec.head" in model.pk_split
        # algorithmic f32 FLOP per launch.  The forward with losses keeps the raw parameters of the frames matched to a ground-truth
        # frame (B * T of the B * N node frames): all 100 channels for those, the 80 channel slots the mixture mean reads (logits,
        # means, colour coefficients, red log-scales) for the other node frames, whose distribution nobody reads (frame_binding.py:91-92)
        n_matched = hp.batch_size * hp.max_seq_len
        per_ch = 2.0 * hp.img_sz * hp.img_sz * hp.ngf * 9
        if split:
            head_flops = per_ch * (80 * F + 20 * n_matched)
        else:
            head_flops = per_ch * hp.head_channels * F
        avg_ms = sum(head_ms) / len(head_ms)
        achieved = head_flops / (avg_ms * 1e-3) / 1e12
        if split:
            # every f32 product = 3 f16 MFMA products: the matrix-pipe bound for f32-equivalent FLOP is the dense f16 peak / 3
            peak = F16_MFMA_PEAK_TFLOPS / 3.0
            kern = ("conv3x3_head_split_kernel (decoder output head, 3x3 conv 16->100 ch @64x64 over 2032 node frames: 100 channels + raw "
                    "parameters for the 1280 matched frames, the 80 channels of the mixture mean for the rest; "
                    "split-f16: 3 v_mfma_f32_16x16x32_f16 per f32 product, f32 accumulate, per-item power-of-two scale; fused mixture mean)")
        else:
            peak = F32_MFMA_PEAK_TFLOPS
            kern = ("conv3x3_head_kernel<6, true> (decoder output head, 3x3 conv 16->100 ch @64x64 = 6 MFMA tiles + 4-channel 4x4x1 "
                    "remainder, fused mixture mean)")
        traffic, pmc_round = measured_head_traffic(hp.batch_size, args.eval_bn)
        traffic_source = (None if traffic is None else
                          f"profiles/pmc_head_kernel.json ({pmc_round}): rocprofv3 --pmc passes of this command on these kernel sources "
                          "(source hash checked), NOT measured in this run")
        line = {
            "metric": "predicted frames/sec, 64x64x3 seq_len=80 gcp_tree (posterior forward + all loss terms, model(inputs) and model.loss() of train.py:157-159, batch-stat BatchNorm)",
            "value": round(value, 1), "unit": "frames/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(1e3 * elapsed / args.steps, 3), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "f32" + (" (encoder / decoder convs and the tree GEMMs from 512 rows: split-f16 MFMA with f32 accumulate, f32-equivalent; everything else exact f32 MFMA)" if split else ""),
            "data": "synthetic",
            "config": {"workload": "BASELINE configs[1]: 25-room gcp_tree forward, 64x64x3, seq_len 80, batch 16/GPU, "
                                   "L=7 (127 nodes/seq decoded), discrete-logistic-mixture head, ELBO + auxiliary losses, "
                                   + ("running-stat" if args.eval_bn else "batch-stat") + " BatchNorm",
                       "batch_per_gpu": hp.batch_size, "seq_len": hp.max_seq_len, "img": hp.img_sz,
                       "nodes_per_seq": hp.n_nodes, "parallelism": f"dp{world} (independent sequences, no collective)",
                       "total_loss_last_step": total_loss,
                       # how the timed steps were replayed: GCPTreeModel times graph against eager replay once per plan (`tuned_ms`,
                       # 3 x 4 replays each between a forward() call's stream hand-overs) and keeps the faster; also.forward_graph /
                       # also.forward_eager time the whole step both ways in this process
                       "replay": replay},
            "roofline": {"kernel": kern,
                         "bound": "mfma", "achieved": round(achieved, 2), "peak": round(peak, 1), "unit": "TFLOP/s",
                         "frac": round(achieved / peak, 4),
                         "peak_basis": ("dense f16 MFMA peak 2500 TFLOP/s / 3 MFMAs per f32 product" if split else "f32 MFMA peak"),
                         # HBM bytes per launch: rocprofv3 PMC passes of this command on these kernel sources (profiles/pmc_head_kernel.json,
                         # tools/pmc_collect.sh), null when the head kernel changed since or the workload differs;
                         # algorithmic bytes = 532.7 MB in (16 ch f32 @64x64 x 2032 frames) + 99.9 MB out
                         "traffic": traffic, "traffic_source": traffic_source,
                         "avg_launch_ms": round(avg_ms, 4), "flop_per_launch": head_flops},
        }
        if also is not None:
            line["also"] = also
            if world > 1:
                # `value` has no collective in it (independent sequences): the curves that carry the exchange are the training step
                # (bucketed RCCL all-reduce under the backward) and the sharded CEM iteration (cost all-gather + elite all-reduce) —
                # as top-level fields, so that a scaling run reads them per N next to `value`
                for key in ("train_step", "planning_iteration"):
                    if isinstance(also.get(key), dict) and "error" not in also[key]:
                        line["scaling_" + key] = dict(also[key], n_gpus=world, scaling="weak")
        if world == 1 and (args.full or args.cpu_baseline_full) and not args.no_cpu_baseline:
            line["cpu_baseline"] = cpu_baseline(full=args.cpu_baseline_full)
        print(json.dumps(line), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
