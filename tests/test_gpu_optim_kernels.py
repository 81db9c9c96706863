"""-m gpu: the kernels that write every parameter on every training step (csrc/scalar_f32.hip: gcpx_radam_step, gcpx_optim_step,
gcpx_optim_range, gcpx_grad_clip_coef) against the FLOAT64 references of tests/optim_refs.py: theta AND both moments, over the step
counter (t = 1 .. 40, 100 .. 2^24), six beta2, the loop structure of the 16-byte and the scalar kernels under max_blocks, grad_scale
times the clip coefficient in all its states, and the clip norm in its fixed summation order, overflow included.

Conventions (those of tests/test_gpu_loss_kernels.py):
  * the kernels are called through video_gcp_amd.runtime as GCPTrainStep.optimizer_step calls them (training.py:300-319);
  * what a kernel must write and does not own starts as NaN (state[1], state[2], the partial sums); what it must leave alone is
    compared by bits (the NaN frame around a slice, the vectors a kind does not write, state[1..3] of a step, state[0] / state[3] and
    the partial buffer past n_partial of the clip);
  * every tolerance is derived in tests/optim_refs.py beside its reference from counted float32 roundings, nothing measured;
    tests/test_optim_refs_cpu.py shows that a float32 restatement meets every bound on these inputs, that eleven planted mistakes do
    not, and that the float32 coefficients the kernels computed before do not either;
  * "worst" in a docstring = the largest error / tolerance measured on an MI355X over the cases of that test.  Ratios close to 1 are
    what these bounds give by construction: where the update is small against theta, the bound IS theta's storage rounding u |theta|,
    and a correctly rounded result errs by anything up to u |theta| just above a power of two (the float32 restatement on the CPU
    reaches 0.994 on the same inputs)."""
import math

import numpy as np
import pytest
import torch

import optim_refs as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    from video_gcp_amd import runtime as rt
    lib = rt.load_library()
    assert torch.cuda.is_available()
    return rt, lib, torch.device("cuda")


def _st():
    return torch.cuda.current_stream().cuda_stream


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()


def _host(t):
    return t.cpu().numpy()


def _step(env, case):
    """one gcpx_radam_step (kind 0) / gcpx_optim_step (kinds 1 .. 3) on a case of optim_refs -> dict theta, m, v, state (numpy float32)"""
    rt, lib, _ = env
    th, gd, m, v, st = (_dev(case[k]) for k in ("theta", "grad", "m", "v", "state"))
    n = th.numel()
    if case["kind"] == 0:
        rt.check(lib.gcpx_radam_step(th.data_ptr(), gd.data_ptr(), m.data_ptr(), v.data_ptr(), st.data_ptr(), n, *case["hp"], _st()), "radam")
    else:
        rt.check(lib.gcpx_optim_step(th.data_ptr(), gd.data_ptr(), m.data_ptr(), v.data_ptr(), st.data_ptr(), n, case["kind"], *case["hp"], _st()),
                 "optim_step")
    torch.cuda.synchronize()
    assert np.array_equal(R.bits(_host(gd)), R.bits(case["grad"])), "the gradient was written"
    return dict(theta=_host(th), m=_host(m), v=_host(v), state=_host(st))


# ------------------------------------------------------------------------------------------------------------------------------
# a. the scalar coefficients over the step counter
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beta2", R.BETA2S)
@pytest.mark.parametrize("kind", [0, 1])
def test_coefficients_over_the_step_counter(env, kind, beta2):
    """RAdam and Adam with state[0] = t - 1 written by the test, t = 1 .. 40, 100, 1e3, 1e4, 1e5, 1e6, 2^24 - 1 and 2^24 (beta2^t
    underflows; the counter lands on 2^24 exactly and stays), beta1 0.5 / 0.9, from theta = 0 (theta afterwards is the update: a purely
    relative bound of 9 - 14 roundings) with cold (m = v = 0) and warm moments, 64 gradients of 1e-6 .. 1e3.  theta, m, v and
    state[0] against ref_step.  RAdam: the result must be inside the bound of the float64 decision sma >= 5 and OUTSIDE the bound of
    the other one, for every (beta2, t): the decision is the float64 one.
    worst radam 0.849, adam 0.849 (both beta2 = 0.9995, beta1 = 0.5, t = 1, warm).  With the float32 coefficients of before this file:
    radam outside from t = 6 at every beta2 (err/tol 2.7 at 0.98, 1.7e3 at 0.999) and RECTIFIED at t = 3 for 0.9999 (err/tol 8e9),
    adam outside at t = 2 for beta2 >= 0.995 (17 at 0.9999)."""
    worst, at = 0.0, None
    for c in R.coef_cases(kind, beta2):
        after = _step(env, c)
        w = R.check_step(c["name"], c, after)
        if w > worst:
            worst, at = w, c["name"]
        if kind == 0:
            rect = R.radam_coef(float(c["t"]), R.f32(c["hp"][1]), R.f32(beta2))[0]
            with pytest.raises(AssertionError):
                R.check_step(c["name"] + " (other decision)", c, after, force_rect=not rect)
        if c["t"] == 2 ** 24:
            assert float(after["state"][0]) == 2.0 ** 24
    print(f"[ratio] coefficients {R.KIND_NAMES[kind]} beta2={beta2}: worst err/tol {worst:.3g} at {at}")


# ------------------------------------------------------------------------------------------------------------------------------
# b. twelve consecutive steps, all kinds
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("theta_zero", [False, True])
@pytest.mark.parametrize("eps", [1e-8, 1e-3])
@pytest.mark.parametrize("config", sorted(R.TRAJ_CONFIGS))
def test_twelve_steps_match_the_float64_trajectory(env, config, eps, theta_zero):
    """Twelve steps from state = 0 of every kind (RMSprop and SGD with and without momentum), eps 1e-8 / 1e-3, theta from N(0, 1) and
    from 0; 1000 gradients whose scale moves by 100 x between steps, 12 of |g| = 1e-12 and 12 of exactly 0 (eps rules: the update is ~0,
    v only decays).  theta, m, v at every step against ref_step restarted from the float32 state the kernel left (optim_refs.trajectory:
    the one-step bound holds at every step, nothing compounds); vectors a kind does not write keep their bits; state[0] ends at 12.
    worst 0.991 (radam eps = 1e-3 theta0 = N(0, 1); rmsprop eps = 1e-8)."""
    worst = R.trajectory(lambda c: _step(env, c), config, eps, theta_zero)
    print(f"[ratio] trajectory {config} eps={eps} theta0={'0' if theta_zero else 'N01'}: worst err/tol {worst:.3g}")


# ------------------------------------------------------------------------------------------------------------------------------
# c. loop structure: where elements get skipped or written twice
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_blocks", [1, 2, 3, 0])
@pytest.mark.parametrize("kind", [0, 1])
def test_slices_under_max_blocks_touch_every_element_once(env, kind, max_blocks):
    """gcpx_optim_range on a slice inside a NaN-framed buffer, held to 1 / 2 / 3 workgroups and unlimited (0).  Lengths
    (optim_refs.loop_lengths): 1 .. 9, and for S = 256 max_blocks float4 per access 8 S - 4, 8 S, 8 S + 4, 8 S + 2, 12 S + 1, 20 S + 7
    (the second access of the last trip out of range for one thread / for all / in range by one float4; n % 4 = 1, 2, 3).  Slice
    starts at 0, 1, 2, 3 floats past a 16-byte boundary, and with only `grad` off by one (any unaligned vector sends RAdam to its
    scalar kernel).  Every element inside against ref_step (counter 6, clip slot 0.5, grad_scale 0.5); every element outside keeps its
    bits in all four vectors; tick = 0 leaves `state` bit-identical, tick = 1 adds exactly 1 to state[0] and leaves state[1..3].
    worst 0.994 (radam, max_blocks 2, 3 and 0), adam 0.99."""
    rt, lib, dev = env
    worst = 0.0
    for i, n in enumerate(R.loop_lengths(max_blocks)):
        for j, (off, goff) in enumerate(R.LOOP_OFFSETS):
            c = R.loop_case(kind, n, i * len(R.LOOP_OFFSETS) + j)
            total = R.LOOP_PAD + 3 + n + R.LOOP_PAD
            host, devs = {}, {}
            for k in ("theta", "grad", "m", "v"):
                o = R.LOOP_PAD + (goff if k == "grad" else off)
                host[k] = np.full(total, np.nan, dtype=np.float32)
                host[k][o:o + n] = c[k]
                devs[k] = (_dev(host[k]), o)
            st = _dev(c["state"])
            ptr = {k: t.data_ptr() + 4 * o for k, (t, o) in devs.items()}
            assert (ptr["theta"] % 16 == 0) == (off == 0)
            rt.check(lib.gcpx_optim_range(ptr["theta"], ptr["grad"], ptr["m"], ptr["v"], st.data_ptr(), n, kind, *c["hp"], c["tick"], max_blocks,
                                          _st()), "optim_range")
            torch.cuda.synchronize()
            after = {"state": _host(st)}
            for k, (t, o) in devs.items():
                got = _host(t)
                inside = np.zeros(total, dtype=bool)
                inside[o:o + n] = k != "grad"
                assert np.array_equal(R.bits(got)[~inside], R.bits(host[k])[~inside]), f"{c['name']} offsets {off}/{goff}: {k} written outside the slice"
                after[k] = got[o:o + n]
            worst = max(worst, R.check_step(f"{c['name']} offsets {off}/{goff} max_blocks {max_blocks}", c, after))
            if not c["tick"]:
                assert np.array_equal(R.bits(after["state"]), R.bits(c["state"])), "tick = 0 changed the state"
    print(f"[ratio] slices {R.KIND_NAMES[kind]} max_blocks={max_blocks}: worst err/tol {worst:.3g}")


# ------------------------------------------------------------------------------------------------------------------------------
# d. grad_scale times the clip coefficient
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,p1,p2", R.SCALE_CONFIGS)
def test_grad_scale_times_the_clip_coefficient(env, kind, p1, p2):
    """state[1] = 0 (unset: 1), 1, 0.25, 1e-30 (g g underflows) and -1 (a coefficient of zero: the gradient does not enter) x grad_scale 1,
    0.5, 1/3, at t = 1 (warm m: SGD's buffer must start as the gradient) and t = 8; 257 elements, all four kinds, theta, m, v against
    ref_step.  With the gate closed (state[3] = 1) the same call leaves theta, m, v and the whole state bit-identical.
    worst 0.988 (sgd with momentum)."""
    worst = 0.0
    cases = [c for c in R.scale_cases() if c["kind"] == kind and c["hp"][1] == p1]
    assert len(cases) == len(R.SCALE_COEFS) * len(R.SCALE_GRAD_SCALES) * 2
    for c in cases:
        worst = max(worst, R.check_step(c["name"], c, _step(env, c)))
    gated = dict(cases[-1], state=np.array([7, 0.25, 5, 1], dtype=np.float32))
    after = _step(env, gated)
    for k in ("theta", "m", "v", "state"):
        assert np.array_equal(R.bits(after[k]), R.bits(gated[k])), f"gate closed: {k} changed"
    print(f"[ratio] grad_scale x clip {R.KIND_NAMES[kind]} p1={p1}: worst err/tol {worst:.3g}")


# ------------------------------------------------------------------------------------------------------------------------------
# e. gcpx_grad_clip_coef
# ------------------------------------------------------------------------------------------------------------------------------
def _clip(env, gd, n, gs, mx, n_partial, state0):
    rt, lib, dev = env
    part = torch.full((n_partial + 8,), R.NAN, device=dev)
    st = _dev(state0)
    rt.check(lib.gcpx_grad_clip_coef(gd.data_ptr(), n, gs, mx, part.data_ptr(), n_partial, st.data_ptr(), _st()), "grad_clip_coef")
    torch.cuda.synchronize()
    return _host(st), _host(part)


@pytest.mark.parametrize("n", R.CLIP_NS)
def test_clip_norm_and_coefficient_match_float64(env, n):
    """state[2] = ||grad_scale g|| and state[1] = min(1, max_norm / (norm + 1e-6)) against ref_clip within clip_tol (the fixed order of
    the two-stage sum: depth = 1 + ceil(n / 256 n_partial) + 8 + ceil(n_partial / 256) + 8 roundings), n 1 / 255 / 257 / 10007 / 262147 x
    n_partial 1 / 2 / 256 / 1024 (the trainer's) / 4096 x max_norm 0.5 / 1e-3 / 0 / -1 (<= 0: the coefficient is exactly 1) x grad_scale
    1 / 0.5 / -0.5 x gradients N(0, 1), one 1e6 among 1e-3, all zero (norm 0, coefficient 1), |g| over 1e-15 .. 1e15.  Both slots and the
    partials start as NaN: workgroups past the data (n < 256 n_partial) must leave 0, the buffer past n_partial keeps its NaN; state[0]
    and state[3] keep their bits.
    worst 0.082 (n = 257)."""
    worst = 0.0
    state0 = np.array([5, np.nan, np.nan, 1], dtype=np.float32)
    for kind in R.CLIP_SETS:
        g = R.clip_grad(kind, n)
        gd = _dev(g)
        for n_partial in R.CLIP_PARTIALS:
            for gs in R.CLIP_GRAD_SCALES:
                for mx in R.CLIP_MAX_NORMS:
                    st, part = _clip(env, gd, n, gs, mx, n_partial, state0)
                    name = f"{kind}-n={n}-partials={n_partial}-scale={gs}-max_norm={mx}"
                    rn, rc = R.ref_clip(g, gs, mx)
                    tn, tc = R.clip_tol(g, gs, mx, n_partial)
                    worst = max(worst, R.ratio(st[2], rn, tn, "norm " + name), R.ratio(st[1], rc, tc, "coefficient " + name))
                    if mx <= 0:
                        assert float(st[1]) == 1.0, name
                    assert np.array_equal(R.bits(st[[0, 3]]), R.bits(state0[[0, 3]])), f"{name}: state[0] / state[3] changed"
                    assert np.isfinite(part[:n_partial]).all(), f"{name}: a partial sum was not written"
                    used = -(-n // 256)
                    assert (part[used:n_partial] == 0).all(), f"{name}: a workgroup without data left a partial sum that is not 0"
                    assert np.isnan(part[n_partial:]).all(), f"{name}: the partial buffer was written past n_partial"
    print(f"[ratio] clip n={n}: worst err/tol {worst:.3g}")


@pytest.mark.parametrize("value", R.OVERFLOW_VALUES)
def test_an_overflowed_clip_norm_zeroes_the_gradient(env, value):
    """1000 finite gradients of 1e19 / 1e20: the float32 sum of squares is inf.  clip_grad_norm_ returns inf and leaves a gradient of
    zeros (pinned in tests/test_optim_refs_cpu.py), so gcpx_grad_clip_coef (max_norm 0.5, 1024 partials) followed by one step of each
    kind must leave what ref_step leaves for a ZERO gradient: state[2] = inf, state[1] < 0 (a coefficient of zero, distinct from
    0 = unset, which would apply the exploded gradient at full size).
    worst 0.986.  Before this file: state[1] = 0.0 and the gradient of 1e19 applied whole."""
    worst = 0.0
    for kind, p1, p2 in R.SCALE_CONFIGS:
        c = R.overflow_case(kind, p1, p2, value)
        assert np.isfinite(c["grad"]).all()
        st, _ = _clip(env, _dev(c["grad"]), c["grad"].size, 1.0, 0.5, 1024, np.array([7, np.nan, np.nan, 0], dtype=np.float32))
        assert math.isinf(float(st[2])) and float(st[2]) > 0, f"state[2] = {float(st[2])!r}, want inf"
        assert float(st[1]) < 0, f"state[1] = {float(st[1])!r}: a coefficient of zero must not read as unset"
        c = dict(c, state=st)
        after = _step(env, c)
        worst = max(worst, R.check_step(c["name"] + " (against a zero gradient)", dict(c, grad=np.zeros_like(c["grad"])), after))
    print(f"[ratio] overflowed norm {value:g}: worst err/tol {worst:.3g}")
