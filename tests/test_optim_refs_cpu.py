"""No GPU: pins tests/optim_refs.py, the float64 references and rounding bounds tests/test_gpu_optim_kernels.py holds the optimizer and
gradient-clip kernels to.
  1. ref_step, run on in float64, equals torch.optim.Adam / RMSprop / SGD and oracle.radam_oracle.RAdamOracle over 12 steps to 1e-12
     relative; ref_clip + ref_step equals torch.nn.utils.clip_grad_norm_ + the torch step; float32 clip_grad_norm_ on a gradient whose
     sum of squares overflows returns inf and leaves a gradient of zeros (the fact the kernel's overflow case is held to);
  2. the float32 restatement f32_step / f32_clip stays inside every bound on every input set the GPU file uses (both files import
     the sets from optim_refs): the bounds can be met without the code under test;
  3. the same restatement with ONE planted mistake falls outside a bound on at least one of those sets, for every mistake of
     optim_refs.MISTAKES; and so does the restatement with the float32 coefficients the kernels used to compute (today_coef);
  4. the rectification table: the float64 decision sma >= 5 and its margin for every (beta2, t) of the GPU file."""
import math

import numpy as np
import pytest
import torch

import optim_refs as R


def _close(a, b, what):
    """1e-12 relative per element (1e-14 absolute where theta - update cancels)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    err = np.abs(a - b)
    lim = 1e-12 * np.maximum(np.abs(a), np.abs(b)) + 1e-14
    assert (err <= lim).all(), (what, float(err.max()), int(np.argmax(err - lim)))


# ------------------------------------------------------------------------------------------------------------------------------
# 1. the reference against the specification
# ------------------------------------------------------------------------------------------------------------------------------
HP = dict(lr=R.f32(1e-2), b1=R.f32(0.9), b2=R.f32(0.999), alpha=R.f32(0.99), eps=R.f32(1e-8))      # float32 values, as the ABI passes them
SPEC = [("adam", 1, 0.0), ("rmsprop", 2, 0.0), ("rmsprop", 2, 0.9), ("sgd", 3, 0.0), ("sgd", 3, 0.9), ("radam", 0, 0.0)]


def _torch_optimizer(name, p, momentum):
    if name == "adam":
        return torch.optim.Adam([p], lr=HP["lr"], betas=(HP["b1"], HP["b2"]), eps=HP["eps"])
    if name == "rmsprop":
        return torch.optim.RMSprop([p], lr=HP["lr"], alpha=HP["alpha"], eps=HP["eps"], momentum=R.f32(momentum))
    return torch.optim.SGD([p], lr=HP["lr"], momentum=R.f32(momentum))


@pytest.mark.parametrize("clip", [None, 0.5])
@pytest.mark.parametrize("name,kind,momentum", SPEC)
def test_reference_equals_torch_and_the_radam_oracle(name, kind, momentum, clip):
    """12 steps in float64 from N(0, 1) parameters with gradients whose scale moves by 10 x per step; with clip: the summed gradient
    of two ranks (grad_scale = 0.5) through ref_clip -> state[1] -> ref_step against clip_grad_norm_(0.5) + the torch step"""
    from oracle.radam_oracle import RAdamOracle
    g = torch.Generator().manual_seed(5)
    n = 301
    theta0 = torch.randn(n, generator=g, dtype=torch.float64)
    p = torch.nn.Parameter(theta0.clone())
    params = {"p": theta0.clone()}
    opt = RAdamOracle(lr=HP["lr"], betas=(HP["b1"], HP["b2"]), eps=HP["eps"]) if kind == 0 else _torch_optimizer(name, p, momentum)
    p1, p2 = (HP["b1"], HP["b2"]) if kind in (0, 1) else ((momentum, HP["alpha"]) if kind == 2 else (momentum, 0.0))
    th, m, v, st = theta0.numpy().copy(), np.zeros(n), np.zeros(n), np.zeros(4)
    scale = 0.5 if clip else 1.0
    for step in range(12):
        grad = torch.randn(n, generator=g, dtype=torch.float64) * 10.0 ** (step % 3 - 1)
        p.grad = grad.clone()
        if clip:
            total = torch.nn.utils.clip_grad_norm_([p], clip)
            norm, coef = R.ref_clip((grad / scale).numpy(), scale, clip)
            assert abs(norm - float(total)) <= 1e-12 * norm
            st[1] = coef
        if kind == 0:
            opt.step(params, {"p": p.grad})
            want = params["p"].numpy()
        else:
            opt.step()
            want = p.detach().numpy()
        r = R.ref_step(kind, th, (grad / scale).numpy(), m, v, st, HP["lr"], p1, p2, HP["eps"], scale)
        th, m, v, st = r["theta"], r["m"], r["v"], r["state"]
        _close(th, want, (name, momentum, clip, step))
    assert st[0] == 12.0
    if kind == 0:
        _close(m, opt.m["p"].numpy(), "exp_avg")
        _close(v, opt.v["p"].numpy(), "exp_avg_sq")
    elif kind == 1:
        _close(m, opt.state[p]["exp_avg"].numpy(), "exp_avg")
        _close(v, opt.state[p]["exp_avg_sq"].numpy(), "exp_avg_sq")
    elif kind == 2:
        _close(v, opt.state[p]["square_avg"].numpy(), "square_avg")
        if momentum:
            _close(m, opt.state[p]["momentum_buffer"].numpy(), "momentum_buffer")
    elif momentum:
        _close(m, opt.state[p]["momentum_buffer"].numpy(), "momentum_buffer")


def test_the_gate_tick_and_the_clip_slot_of_the_reference():
    """include/gcpx.h:799-803: a closed gate leaves everything; tick = 0 leaves the counter; state[1]: 0 = unset = 1, < 0 = zero"""
    c = R.scale_cases()[0]
    a = R.ref_step(*R.step_args(dict(c, state=np.array([3, 0.25, 5, 1], dtype=np.float32))))
    for k in ("theta", "m", "v", "state"):
        assert np.array_equal(a[k], np.asarray(dict(c, state=[3, 0.25, 5, 1])[k], dtype=np.float64)), k
    assert R.ref_step(*R.step_args(c), tick=0)["state"][0] == c["state"][0] and R.ref_step(*R.step_args(c))["state"][0] == c["state"][0] + 1
    unset = R.ref_step(*R.step_args(dict(c, state=[3, 0, 0, 0])))
    one = R.ref_step(*R.step_args(dict(c, state=[3, 1, 0, 0])))
    zero = R.ref_step(*R.step_args(dict(c, state=[3, -1, 0, 0])))
    nograd = R.ref_step(*R.step_args(dict(c, state=[3, 1, 0, 0], grad=np.zeros_like(c["grad"]))))
    for k in ("theta", "m", "v"):
        assert np.array_equal(unset[k], one[k]) and np.array_equal(zero[k], nograd[k]) and not np.array_equal(zero[k], one[k]), k


@pytest.mark.parametrize("value", R.OVERFLOW_VALUES)
def test_float32_clip_grad_norm_zeroes_a_gradient_whose_norm_overflows(value):
    """the specification of the overflow case: 1000 finite elements of 1e19 / 1e20, float32: the norm is inf, the gradient left is 0"""
    c = R.overflow_case(1, 0.9, 0.999, value)
    p = torch.nn.Parameter(torch.zeros(c["grad"].size))
    p.grad = torch.from_numpy(c["grad"].copy())
    assert bool(torch.isfinite(p.grad).all())
    total = torch.nn.utils.clip_grad_norm_([p], 0.5)
    assert math.isinf(float(total)) and bool((p.grad == 0).all())
    norm, coef = R.f32_clip(c["grad"], 1.0, 0.5, 1024)
    assert math.isinf(float(norm)) and float(coef) == -1.0 and R.clip_factor(coef) == 0.0


# ------------------------------------------------------------------------------------------------------------------------------
# 2. / 3. the float32 restatement inside every bound, every planted mistake outside one
# ------------------------------------------------------------------------------------------------------------------------------
def _all_step_cases():
    for kind in (0, 1):
        for beta2 in R.BETA2S:
            yield from R.coef_cases(kind, beta2)
    seen = set()
    for kind in (0, 1):
        for mb in (0, 1, 2, 3):
            for i, n in enumerate(R.loop_lengths(mb)):
                for j in range(len(R.LOOP_OFFSETS)):
                    idx = i * len(R.LOOP_OFFSETS) + j
                    if (kind, n, idx % 2) not in seen:
                        seen.add((kind, n, idx % 2))
                        yield R.loop_case(kind, n, idx)
    yield from R.scale_cases()


def _run_all(**kw):
    """every input set through f32_step(**kw): (worst ratio, names of the cases outside a bound)"""
    worst, failed = 0.0, []

    def one(name, fn):
        nonlocal worst
        try:
            worst = max(worst, fn())
        except AssertionError:
            failed.append(name)
    for c in _all_step_cases():
        one(c["name"], lambda: R.check_step(c["name"], c, R.f32_step(*R.step_args(c), tick=c["tick"], **kw)))
    for config in R.TRAJ_CONFIGS:
        for eps in (1e-8, 1e-3):
            for zero in (False, True):
                one(f"traj-{config}-{eps}-{zero}",
                    lambda: R.trajectory(lambda c: R.f32_step(*R.step_args(c), tick=1, **kw), config, eps, zero))
    return worst, failed


def test_the_float32_restatement_meets_every_step_bound():
    worst, failed = _run_all()
    print(f"[ratio] float32 restatement, all step cases: worst err/tol {worst:.3g}")
    assert not failed, failed[:10]


@pytest.mark.parametrize("mistake", R.MISTAKES)
def test_a_planted_mistake_misses_a_bound(mistake):
    _, failed = _run_all(mistake=mistake)
    print(f"{mistake}: outside a bound on {len(failed)} cases, first {failed[:3]}")
    assert failed, f"no input set tells `{mistake}` from the right step"


def test_the_float32_coefficients_of_before_miss_the_bound():
    """Defect 1: the step with today_coef (float32 pow, float32 sma, the kernel's order) is outside the bound at beta2 = 0.999, t = 6
    (the first rectified step of the project's own betas), and by orders of magnitude at 0.9999; Adam's float32 bias correction
    sqrt(1 - powf(beta2, t)) is outside for beta2 = 0.9999 at small t (not at t = 1 HERE: a correctly rounded powf(b, 1) is b and
    1 - b is exact; a powf that is one ulp off, as a device library may be, is worst there)."""
    def worst_ratio(kind, beta2, t):
        c = [c for c in R.coef_cases(kind, beta2) if c["t"] == t and "b1=0.9-" in c["name"] and c["name"].endswith("cold")][0]
        after = R.f32_step(*R.step_args(c), coef="today")
        r = R.ref_step(*R.step_args(c))
        return float(np.max(np.abs(after["theta"].astype(np.float64) - r["theta"]) / r["tol_theta"]))
    a, b, c = worst_ratio(0, 0.999, 6), worst_ratio(0, 0.9999, 6), max(worst_ratio(1, 0.9999, t) for t in range(2, 9))
    print(f"today's coefficients: err/tol {a:.3g} (radam 0.999 t=6), {b:.3g} (radam 0.9999 t=6), {c:.3g} (adam 0.9999 t=2..8)")
    assert a > 10 and b > 1e4 and c > 10, (a, b, c)
    _, failed = _run_all(coef="today")
    assert any("radam-b2=0.999-" in f and "-t=6-" in f for f in failed) and any("adam-b2=0.9999-" in f for f in failed), failed[:10]


def test_gt_for_ge_at_the_threshold_is_no_different_function():
    """`sma > 5` for `sma >= 5` differs only where sma == 5 exactly; no (beta2, t) of the table is there (the smallest margin is
    4e-4, test_rectification_table), so on every input set the mutant leaves the bits of the right step: no test can reject it, and it
    is kept out of MISTAKES for that reason, not forgotten."""
    for beta2 in R.BETA2S:
        for c in R.coef_cases(0, beta2):
            a, b = R.f32_step(*R.step_args(c)), R.f32_step(*R.step_args(c), mistake="rect_gt")
            assert all(np.array_equal(R.bits(a[k]), R.bits(b[k])) for k in ("theta", "m", "v", "state")), c["name"]


@pytest.mark.parametrize("n", R.CLIP_NS)
def test_the_float32_clip_restatement_meets_its_bound(n):
    worst = 0.0
    for kind in R.CLIP_SETS:
        g = R.clip_grad(kind, n)
        for n_partial in R.CLIP_PARTIALS:
            for gs in R.CLIP_GRAD_SCALES:
                for mx in R.CLIP_MAX_NORMS:
                    norm, coef = R.f32_clip(g, gs, mx, n_partial)
                    rn, rc = R.ref_clip(g, gs, mx)
                    tn, tc = R.clip_tol(g, gs, mx, n_partial)
                    name = f"{kind}-n={n}-partials={n_partial}-scale={gs}-max_norm={mx}"
                    worst = max(worst, R.ratio(norm, rn, tn, "norm " + name), R.ratio(coef, rc, tc, "coef " + name))
                    if mx <= 0:
                        assert float(coef) == 1.0
    print(f"[ratio] float32 clip restatement n={n}: worst err/tol {worst:.3g}")
    # a planted mistake: the norm of the unscaled gradient
    g = R.clip_grad("normal", n)
    with pytest.raises(AssertionError):
        R.ratio(R.f32_clip(g, 1.0, 0.5, 256)[0], R.ref_clip(g, 0.5, 0.5)[0], R.clip_tol(g, 0.5, 0.5, 256)[0], "unscaled norm")


@pytest.mark.parametrize("value", R.OVERFLOW_VALUES)
def test_the_restatement_applies_no_gradient_after_an_overflowed_norm(value):
    for kind, p1, p2 in R.SCALE_CONFIGS:
        c = R.overflow_case(kind, p1, p2, value)
        norm, coef = R.f32_clip(c["grad"], 1.0, 0.5, 1024)
        c = dict(c, state=np.array([7, coef, norm, 0], dtype=np.float32))
        after = R.f32_step(*R.step_args(c))
        R.check_step(c["name"], dict(c, grad=np.zeros_like(c["grad"])), after)
        with pytest.raises(AssertionError):           # the coefficient stored as 0 reads as "unset": the gradient goes in at full size
            c0 = dict(c, state=np.array([7, 0, norm, 0], dtype=np.float32))
            R.check_step(c["name"], dict(c0, grad=np.zeros_like(c["grad"])), R.f32_step(*R.step_args(c0)))


# ------------------------------------------------------------------------------------------------------------------------------
# 4. the rectification table
# ------------------------------------------------------------------------------------------------------------------------------
def test_rectification_table():
    """For beta2 in BETA2S and t = 1 .. 64: the float64 decision sma >= 5 and its margin |sma - 5|.  The smallest margin is 3.9e-4
    (0.9999, t = 5, unrectified: sma = 4.99961).  What an implementation that forms sma in double can lose (U = 2^-53):
        sma_max = 2 / (1 - beta2) - 1: 1 - beta2 is exact, quotient and difference: 3 U sma_max;
        Q = 2 t b2t / (1 - b2t): b2t <= 2 log2(t) + 2 products (squaring) or 1 ulp (pow): <= 16 U; 1 - b2t turns that ABSOLUTE error
        into a relative one of 16 U b2t / (1 - b2t) + U; product and quotient 3 more:  Q x U x (20 + 16 b2t / (1 - b2t));
        the last difference U sma.
    Over the table that is at most 1e-7: the margin is 4000 times larger, so every (beta2, t) has ONE right decision for double
    coefficients.  In float32 the same expression is 2^29 times larger (50 at 0.9999): the decision was then a matter of luck."""
    U = 2.0 ** -53
    table, smallest, largest_loss = {}, (1e9, None), 0.0
    for beta2 in R.BETA2S:
        b2 = R.f32(beta2)
        for t in range(1, 65):
            rect, _, sma = R.radam_coef(float(t), R.f32(0.9), b2)
            b2t = b2 ** t
            sma_max = 2.0 / (1.0 - b2) - 1.0
            Q = 2.0 * t * b2t / (1.0 - b2t)
            loss = U * (3 * sma_max + Q * (20 + 16 * b2t / (1.0 - b2t)) + abs(sma))
            margin = abs(sma - 5.0)
            table[(beta2, t)] = (rect, margin)
            smallest = min(smallest, (margin, (beta2, t)))
            largest_loss = max(largest_loss, loss)
            assert margin > 1000 * loss, (beta2, t, margin, loss)
            # the switch sits between t = 5 and t = 6 for every beta2 of the table, as for the project's own 0.999
            assert rect == (t >= 6), (beta2, t, sma)
    print(f"smallest margin {smallest[0]:.3e} at {smallest[1]}; the largest loss of double coefficients {largest_loss:.3e}")
    assert smallest[1] == (0.9999, 5) and 3e-4 < smallest[0] < 5e-4, smallest
    assert largest_loss < 1e-6
    # the float32 coefficients of before decide WRONGLY within one ulp of powf: 0.9999, t = 5
    t, b2 = np.float32(5), np.float32(0.9999)
    low = np.nextafter(R._powf(b2, t), np.float32(0))
    sma_max = np.float32(2) / (np.float32(1) - b2) - np.float32(1)
    assert float(sma_max - np.float32(2) * t * low / (np.float32(1) - low)) >= 5.0 and not table[(0.9999, 5)][0]
