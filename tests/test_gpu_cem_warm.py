"""-m gpu: receding-horizon CEM in the flat batch planner (csrc/cem_batch.hip: gcpx_cem_warm_start, gcpx_cem_population_ex;
planning.CEMPlanner(noise_rho, keep_elites, warm_std).plan_batch(warm=); control.ControlRunner(warm_start=True)).

1. both entry points against their torch mirrors (computed on CPU tensors), equal bit for bit, at K = 2, n = 5, S in {1, 2, 7},
   A in {1, 2, 3, 5, 256, 257}: A = 2 .. 4 takes the one-thread-per-row split, 257 crosses a 256-thread workgroup (K n A = 2570 threads: more
   than one block everywhere from A = 256); rho in {0, 0.5, 0.99}, m in {0, 1, n_elite = 2} of n_prev = 4 previous rows, clip 0.5 and inf, out
   apart from and over eps, NaN and Inf in the noise, a NaN with a payload in a carried row; the shifts -1, 0, 2, 4, 5, 9 with prev of
   the task without a plan NaN.  Every output sits between NaN guard floats, which stay as they are.  rho = 0, m = 0 gives the bits of
   gcpx_cem_population.  An index out of range gives NaN rows.
2. every invalid argument returns the error code and launches nothing: the NaN-filled outputs stay NaN.
3. plan_batch(device=True) on device tensors with a row-independent stub simulator and cost (tests/cem_warm_stubs.py), all options on:
   the CPU run of the same planner on the recorded noise gives the same populations, scores, elites, refits and best samples bit for
   bit; carried elites are the previous elites and no task's best score gets worse.
4. ControlRunner as visual MPC (tests/test_gpu_flat_control.py's conf), E = 3, 4 steps, re-planned at every step, plans kept on the
   device, all options on: every re-plan starts from the previous best sample moved up one step, with a zero tail."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from cem_warm_stubs import DIM, check_carried_elites, images, point_planner, same  # noqa: E402
from video_gcp_amd import planning as P  # noqa: E402
from video_gcp_amd import runtime as rt  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INF, NAN = float("inf"), float("nan")
K, N, N_PREV, N_ELITE, PAD = 2, 5, 4, 2, 64
SHIFT_PAIRS = [(-1, 0), (2, 4), (5, 9)]
SIZES = [(S, A) for S in (1, 2, 7) for A in (1, 2, 3, 5, 256, 257)]


def st():
    return rt.current_stream()


@pytest.fixture(scope="module")
def lib():
    return rt.load_library()


class Guarded:
    """a float32 tensor of `shape` on the device, NaN-filled, with PAD NaN floats in front of it and behind it"""

    def __init__(self, shape, fill=None):
        self.numel = int(np.prod(shape))
        self.buf = torch.full((self.numel + 2 * PAD,), NAN, device=DEV)
        self.t = self.buf[PAD:PAD + self.numel].view(shape)
        if fill is not None:
            self.t.copy_(fill)

    def intact(self):
        return bool(torch.isnan(self.buf[:PAD]).all()) and bool(torch.isnan(self.buf[PAD + self.numel:]).all())

    def untouched(self):
        return bool(torch.isnan(self.buf).all())


# ---- 1. the entry points ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,A", SIZES)
def test_warm_start_equals_its_mirror(lib, S, A):
    g = torch.Generator().manual_seed(100 * S + A)
    init_std = 0.3
    for shifts in SHIFT_PAIRS:
        prev = torch.randn(K, S, A, generator=g)
        for k, s in enumerate(shifts):
            if s < 0:
                prev[k] = NAN
        prev[1, S - 1, A - 1] = NAN                                                 # a NaN of the plan: stays one where it is moved to
        shift = torch.tensor(shifts, dtype=torch.int32)
        pd, sd = prev.to(DEV), shift.to(DEV)
        for warm_std in (1.0, 0.5):
            wm, ws = P.cem_warm_start_torch(prev, shift, init_std, warm_std)
            mean, std = Guarded((K, S, A)), Guarded((K, S, A))
            rt.check(lib.gcpx_cem_warm_start(pd.data_ptr(), sd.data_ptr(), init_std, warm_std, mean.t.data_ptr(), std.t.data_ptr(), K, S, A, st()),
                     "cem_warm_start")
            assert same(mean.t, wm) and same(std.t, ws), (shifts, warm_std)
            assert mean.intact() and std.intact() and same(pd, prev)
            gm, gs = P.cem_warm_start(pd, shift, init_std, warm_std)                # the wrapper takes the shifts from the host or the device
            assert same(gm, wm) and same(gs, ws)
            for k, s in enumerate(shifts):
                if s < 0 or s >= S:
                    assert bool((mean.t[k] == 0).all()) and bool((std.t[k] == np.float32(init_std)).all())


def population_inputs(S, A):
    g = torch.Generator().manual_seed(1000 * S + A)
    mean, std = torch.randn(K, S, A, generator=g), torch.rand(K, S, A, generator=g) + 0.25
    eps, prev_pop = torch.randn(K, N, S, A, generator=g), 10.0 * torch.randn(K, N_PREV, S, A, generator=g)
    eps[0, 3, 0, 0], eps[1, 4, S - 1, A - 1], eps[1, 2, S // 2, A // 2] = NAN, INF, -INF
    prev_pop[0, 3, S - 1, 0] = torch.tensor(np.array([0x7fc01234], np.uint32).view(np.float32))[0]
    idx = torch.tensor([[3, 0], [1, 1]], dtype=torch.int32)
    return mean, std, eps, prev_pop, idx


def launch_population_ex(lib, mean, std, eps, clip, rho, prev_pop, idx, m, out):
    return lib.gcpx_cem_population_ex(mean.data_ptr(), std.data_ptr(), eps.data_ptr(), clip, rho, prev_pop.data_ptr() if m else None,
                                      idx.data_ptr() if m else None, m, N_PREV if m else 0, out.data_ptr(), K, N, mean.shape[1], mean.shape[2], st())


@pytest.mark.parametrize("S,A", SIZES)
def test_population_ex_equals_its_mirror(lib, S, A):
    mean, std, eps, prev_pop, idx = population_inputs(S, A)
    md, sd, ed, pd = mean.to(DEV), std.to(DEV), eps.to(DEV), prev_pop.to(DEV)
    for m in (0, 1, N_ELITE):
        im = idx[:, :m].contiguous()
        imd = im.to(DEV)
        for rho in (0.0, 0.5, 0.99):
            for clip in (0.5, INF):
                want = P.cem_population_ex_torch(mean, std, eps, clip, rho, prev_pop if m else None, im if m else None, m)
                out = Guarded((K, N, S, A))
                rt.check(launch_population_ex(lib, md, sd, ed, clip, rho, pd, imd, m, out.t), "cem_population_ex")
                assert same(out.t, want), (m, rho, clip)
                assert out.intact() and same(ed, eps) and same(pd, prev_pop)
                inplace = Guarded((K, N, S, A), fill=eps)                           # out over eps
                rt.check(launch_population_ex(lib, md, sd, inplace.t, clip, rho, pd, imd, m, inplace.t), "cem_population_ex")
                assert same(inplace.t, want) and inplace.intact(), (m, rho, clip)
                assert same(P.cem_population_ex(md, sd, eps.to(DEV), clip, rho, pd if m else None, imd if m else None, m, inplace=True), want)
                for k in range(K):                                                  # carried rows: the words of prev_pop, not clamped again
                    for j in range(m):
                        assert same(out.t[k, j], prev_pop[k, int(idx[k, j])])
                if rho == 0.0 and m == 0:                                           # the bits of the kernel the default path runs
                    plain = Guarded((K, N, S, A))
                    rt.check(lib.gcpx_cem_population(md.data_ptr(), sd.data_ptr(), ed.data_ptr(), clip, plain.t.data_ptr(), K, N, S * A, st()),
                             "cem_population")
                    assert same(plain.t, out.t) and same(want, P.cem_population_torch(mean, std, eps, clip))
    # an index out of range in task 1: NaN in that task's carried rows alone, no load through it
    good = P.cem_population_ex_torch(mean, std, eps, 0.5, 0.5, prev_pop, idx, N_ELITE)
    for pos, val in ((1, N_PREV), (0, -1), (0, 2 ** 31 - 1)):
        bad = idx.clone()
        bad[1, pos] = val
        out = Guarded((K, N, S, A))
        rt.check(launch_population_ex(lib, md, sd, ed, 0.5, 0.5, pd, bad.to(DEV), N_ELITE, out.t), "cem_population_ex")
        assert same(out.t, P.cem_population_ex_torch(mean, std, eps, 0.5, 0.5, prev_pop, bad, N_ELITE)) and out.intact()
        assert bool(torch.isnan(out.t[1, :N_ELITE]).all()) and same(out.t[0], good[0]) and same(out.t[1, N_ELITE:], good[1, N_ELITE:])


def test_entry_points_refuse_bad_arguments(lib):
    S, A = 2, 3
    mean, std, eps, prev_pop, idx = (t.to(DEV) for t in population_inputs(S, A))
    out, wm, ws = Guarded((K, N, S, A)), Guarded((K, S, A)), Guarded((K, S, A))
    prev, shift = torch.zeros(K, S, A, device=DEV), torch.zeros(K, dtype=torch.int32, device=DEV)
    p = lambda t: t.data_ptr()

    def pop(mean=p(mean), std=p(std), eps=p(eps), clip=0.5, rho=0.5, prev_pop=p(prev_pop), idx=p(idx), m=N_ELITE, n_prev=N_PREV, o=p(out.t),
            K_=K, n=N, S_=S, A_=A):
        return lib.gcpx_cem_population_ex(mean, std, eps, clip, rho, prev_pop, idx, m, n_prev, o, K_, n, S_, A_, st())

    def warm(prev=p(prev), shift=p(shift), init_std=1.0, warm_std=0.5, mean=p(wm.t), std=p(ws.t), K_=K, S_=S, A_=A):
        return lib.gcpx_cem_warm_start(prev, shift, init_std, warm_std, mean, std, K_, S_, A_, st())

    for kw in (dict(mean=None), dict(std=None), dict(eps=None), dict(o=None), dict(prev_pop=None), dict(idx=None),            # a null pointer
               dict(K_=0), dict(n=0), dict(S_=0), dict(A_=-1), dict(n_prev=0),                                                  # a size <= 0
               dict(m=N + 1, n_prev=N + 1), dict(m=N_PREV + 1), dict(m=-1),                                                     # m > n, m > n_prev
               dict(rho=-0.5), dict(rho=1.0), dict(rho=1.5), dict(rho=NAN),                                                     # rho outside [0, 1)
               dict(K_=2 ** 20, n=2 ** 20, A_=1, m=0),                                                                          # > 2^30 workgroups
               dict(prev_pop=p(out.t)), dict(prev_pop=p(out.t) + 4 * (K * N * S * A - 1)), dict(prev_pop=p(out.t) - 4 * (K * N_PREV * S * A - 1))):
        assert pop(**kw) == -1 and b"gcpx_cem_population_ex" in lib.gcpx_last_error(), kw
    assert b"overlaps" in lib.gcpx_last_error()
    for kw in (dict(prev=None), dict(shift=None), dict(mean=None), dict(std=None), dict(K_=0), dict(S_=-2), dict(A_=0),
               dict(warm_std=0.0), dict(warm_std=-0.5), dict(warm_std=1.5), dict(warm_std=NAN), dict(K_=2 ** 30 + 1)):
        assert warm(**kw) == -1 and b"gcpx_cem_warm_start" in lib.gcpx_last_error(), kw
    torch.cuda.synchronize()
    assert out.untouched() and wm.untouched() and ws.untouched()
    assert pop() == 0 and warm() == 0 and pop(m=0, prev_pop=None, idx=None, n_prev=0) == 0       # and the calls they were made from are taken
    torch.cuda.synchronize()
    assert out.intact() and not bool(torch.isnan(wm.t).any())


# ---- 3. plan_batch on the device against the CPU run on the same noise ---------------------------------------------------------------------
def test_plan_batch_on_the_device_equals_the_cpu_run(monkeypatch):
    Kp, S = 3, 6
    g = torch.Generator().manual_seed(21)
    options = dict(keep_elites=0.5, noise_rho=0.5, warm_std=0.5, n_iters=3)
    prev, shift = torch.randn(Kp, S, DIM, generator=g), torch.tensor([1, -1, 2], dtype=torch.int32)
    prev[1] = NAN
    start, goal = torch.randn(Kp, DIM, generator=g), 3.0 * torch.randn(Kp, DIM, generator=g)
    on_dev = point_planner(device=DEV, **options)
    r = on_dev.plan_batch(images(start.to(DEV)), images(goal.to(DEV)), record=True, device=True, latents=False, warm=(prev.to(DEV), shift.to(DEV)))
    rec = on_dev.batch_record
    assert rec.populations[0].is_cuda and r.best.is_cuda and on_dev.batch_best is r.best and on_dev._sim.forwards == [Kp * 8] * 3
    noise = [e.cpu() for e in rec.noise]
    monkeypatch.setattr(torch, "randn", lambda *size, **kw: noise.pop(0))
    on_cpu = point_planner(device="cpu", **options)
    on_cpu.plan_batch(images(start.numpy()), images(goal.numpy()), record=True, warm=(prev, shift))
    monkeypatch.undo()
    chk = on_cpu.batch_record
    assert not noise and rec.m == chk.m == 2
    assert same(rec.start_mean, chk.start_mean) and same(rec.start_std, chk.start_std) and same(rec.populations[0][:, 0], rec.start_mean)
    for key in ("populations", "scores", "means", "stds"):
        assert len(rec[key]) == 3 and all(same(a, b) for a, b in zip(rec[key], chk[key])), key
    assert all(torch.equal(a.cpu(), b) for a, b in zip(rec.elite_idx, chk.elite_idx))
    assert same(r.best, chk.best_samples) and same(r.costs, on_cpu.logs[-1].elite_scores[:, 0])
    check_carried_elites(on_dev, Kp, 2)
    assert bool(torch.isfinite(r.best).all())


# ---- 4. the runner ---------------------------------------------------------------------------------------------------------------------------
class Recording:
    """the planner, every plan_batch call recorded: (start_mean, start_std, best, warm) per call"""
    device_plans = True

    def __init__(self, planner):
        self.planner, self.calls = planner, []

    @property
    def batch_best(self):
        return self.planner.batch_best

    def plan_batch(self, states, goals, **kw):
        out = self.planner.plan_batch(states, goals, record=True, **kw)
        rec = self.planner.batch_record
        self.calls.append((rec.start_mean.clone(), rec.start_std.clone(), self.planner.batch_best.clone(), kw.get("warm"), rec.m))
        return out


@pytest.fixture(scope="module")
def vmpc(tmp_path_factory):
    from test_gpu_flat_control import GPU_VMPC, _built
    yield from _built(tmp_path_factory, GPU_VMPC)


def test_runner_replans_from_the_previous_plan(vmpc):
    from test_gpu_nav_env import CW, IMG
    from video_gcp_amd import control as CT
    from video_gcp_amd import nav_env as NE
    desc, model, planner, _ = vmpc
    E, steps = 3, 4
    planner.set_receding(noise_rho=0.5, keep_elites=0.5, warm_std=0.5)
    try:
        recording = Recording(planner)
        env = NE.NavEnvBatch(9, CW, steps, IMG, DEV)
        runner = CT.ControlRunner(model, recording, env, **dict(desc.policy_args, batch_plans=True, keep_plans=False, warm_start=True))
        assert runner.replan_interval == 1
        res = runner.run(NE.draw_tasks(9, 2, range(E)))
    finally:
        planner.set_receding(noise_rho=0.0, keep_elites=0.0, warm_std=1.0)
    assert res["actions"].shape == (E, steps, 2) and np.isfinite(res["actions"]).all() and (res["n_replans"] == steps).all()
    assert len(recording.calls) == steps and all(set(p) == {"t", "cost"} for plans in runner.plans for p in plans)
    s = planner._sampler
    S, init = s._n_steps, np.float32(s._initial_std)
    n_elite = max(int(planner.batch_size * planner.elite_frac), 1)
    for c, (start_mean, start_std, best, warm, m) in enumerate(recording.calls):
        assert tuple(start_mean.shape) == (E, S, 2) and start_mean.is_cuda and best.is_cuda and m == int(0.5 * n_elite)
        if c == 0:
            assert warm[0] is None and warm[1].tolist() == [-1] * E
            assert bool((start_mean == 0).all()) and bool((start_std == init).all())
            continue
        before = recording.calls[c - 1][2]
        assert warm[1].tolist() == [1] * E and warm[1].dtype == torch.int32 and same(warm[0], before)
        assert same(start_mean[:, :S - 1], before[:, 1:]) and bool((start_mean[:, S - 1] == 0).all())
        assert bool((start_std[:, :S - 1] == np.float32(0.5) * init).all()) and bool((start_std[:, S - 1] == init).all())
    assert same(runner.best, recording.calls[-1][2])
