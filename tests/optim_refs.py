"""FLOAT64 references, float32 restatements, rounding bounds and the shared input sets of the optimizer and gradient-clip kernel tests
(csrc/scalar_f32.hip: gcpx_radam_step, gcpx_optim_step, gcpx_optim_range, gcpx_grad_clip_coef).  tests/test_gpu_optim_kernels.py runs
the kernels on the input sets below, tests/test_optim_refs_cpu.py pins everything here without a GPU.

References.  ref_step / ref_clip are numpy float64 of the formulas include/gcpx.h states for the four entry points (kinds 0 RAdam,
1 Adam, 2 RMSprop, 3 SGD; the state[1] coefficient, the SGD first-step rule, tick, the gate).  They are no transcription of the
kernels.  Their hyperparameters are THE FLOAT32 VALUES THE ABI RECEIVES, WIDENED TO FLOAT64 (f32(0.999) = 0.99900001287...): the entry
points take `float`, so that is the operation they define.  Against Python-double hyperparameters this moves 1 - beta2 by
1.29e-8 / 1e-3 = 1.3e-5 relative at 0.999 (2.3e-5 at 0.9999: 1 - f32(0.9999) = 1.0000229e-4), and with it v and, through the bias
corrections, the step; 1 - beta1 = 0.1 moves by 2.4e-7.  That distance belongs to the ABI, not to a kernel, and no bound here pays for it.

Bounds.  u = 2^-24 (float32 unit roundoff), gam(k) = k u / (1 - k u): k roundings in a product.  Per element
        tol = SECOND x sum over the terms of the update of gam(c_rel) x |term|  +  u x |output|  +  underflow floor
  c_rel   the float32 roundings that term goes through as an implementation must perform them: one per product, sum, quotient; sqrtf
          and the division are TAKEN as <= 1 ulp = 2 u; a fused multiply-add only removes a rounding;
  u |out| the storage rounding of the output (for m and v it is the rounding of the last sum and is counted there);
  floor   TINY = 2^-126 per operation whose result can be subnormal (flushed or gradual: the error is below the smallest normal);
  SECOND  = 1 + 2^-10 covers the products of two first-order terms (each below 2^-16 of the other).
With g = grad x gsc, gsc = fl(grad_scale x coefficient): g carries 2 roundings.  The counts:
  m (kinds 0, 1)      A = beta1 m: 1 (product) + 1 (sum);  B = (1 - beta1) g: 1 (1 - beta1) + 2 (g) + 1 (product) + 1 (sum):
                      tol_m = gam(2) |A| + gam(5) |B|
  v (kinds 0, 1, 2)   A = beta2 v: 2;  B = (1 - beta2) g g: 1 + 2 + 2 + 2 products + 1 sum = 8:  tol_v = gam(2) |A| + gam(8) |B|
  sqrt(v)             |sqrt(v') - sqrt(v)| <= tol_v / (sqrt(v) + sqrt(max(v - tol_v, 0))) =: dsq (exact for the lower end, larger than
                      the upper end's), + 2 u for sqrtf itself
  RAdam rectified     upd = lr step m / (sqrt(v) + eps): step 2 (correct to float32 rounding: 1, and 1 to spare), lr step 1, x m 1;
                      denominator d: sqrtf 2 + sum 1 (both relative to d, sqrt(v) <= d); quotient 2:
                      tol_upd = gam(9) |upd| + |lr step / d| tol_m + |upd| dsq / d
  RAdam unrectified   upd = lr step m:  gam(4) |upd| + |lr step| tol_m
  Adam                upd = lr / bc1 x m / (sqrt(v) / bc2s + eps): bc1 2, quotient 2, x m 1; d: sqrtf 2, bc2s 2, quotient 2, sum 1;
                      last quotient 2:  gam(14) |upd| + |lr / bc1 / d| tol_m + |upd| (dsq / bc2s) / d
  RMSprop             q = g / (sqrt(v) + eps): g 2, d 3, quotient 2: tol_q = gam(7) |q| + |q| dsq / d;  momentum: m = p1 m + q:
                      tol_m = gam(2) |p1 m| + gam(1) |q| + tol_q, upd = lr m: gam(1) |upd| + lr tol_m;  else upd = lr q: gam(1) |upd| + lr tol_q
  SGD                 momentum: m = g (t = 1): gam(2) |g|, else p1 m + g: gam(2) |p1 m| + gam(3) |g|; upd = lr m: gam(1) |upd| + lr tol_m;
                      else upd = lr g: gam(3) |upd|
  theta               theta - upd:  tol_theta = tol_upd + u |theta|
The scalar coefficients (b1^t, b2^t, sma_max, sma, the rectification term, the bias corrections) are ASSUMED correct to float32
rounding: the bound gives each of them (`step`, `bc1`, `bc2s`) 2 u, nothing for cancellation inside.  An implementation that forms
sma = sma_max - 2 t b2^t / (1 - b2^t) in float32 does not meet that assumption (sma_max ~ 2 / (1 - beta2) carries u x 2e4 absolute at
0.9999, and sma ~ t is what is left); today_coef restates that and tests/test_optim_refs_cpu.py shows it falls outside.

Consecutive steps.  A reference that runs on from its own state sees the kernel's error of step k again in step k + 1: the error of
m obeys e' <= beta1 e + tol_m, hence <= tol_m / (1 - beta1) (10 x at 0.9), v's <= tol_v / (1 - beta2) (1000 x at 0.999), and theta's
adds up: K steps cost K x tol_theta plus what the moments' errors do to each update.  The tests therefore restart the reference at
every step from the float32 state the implementation under test left (trajectory): every step is held to the one-step bound.

Clip norm: clip_tol, beside ref_clip."""
import math

import numpy as np

EPS = 2.0 ** -24
TINY = 2.0 ** -126
SECOND = 1.0 + 2.0 ** -10
NAN = float("nan")
F = np.float32
KIND_NAMES = {0: "radam", 1: "adam", 2: "rmsprop", 3: "sgd"}


def f32(x):
    """a Python float as the C ABI passes it (float arguments are rounded to f32 on the way in), widened again"""
    return float(np.float32(x))


def gam(k):
    return k * EPS / (1.0 - k * EPS)


def clip_factor(c):
    """state[1] as the step entry points read it: > 0 the coefficient, 0 = unset = 1, < 0 = the coefficient is zero"""
    return float(c) if c > 0 else (0.0 if c < 0 else 1.0)


# ------------------------------------------------------------------------------------------------------------------------------
# 1. the scalar coefficients
# ------------------------------------------------------------------------------------------------------------------------------
def radam_coef(t, beta1, beta2):
    """float64: (rectified?, step coefficient, sma) of RAdam at step t (Liu et al. 2019, Alg. 2, threshold sma >= 5 as the authors' code)"""
    b2t, b1t = beta2 ** t, beta1 ** t
    sma_max = 2.0 / (1.0 - beta2) - 1.0
    sma = sma_max - 2.0 * t * b2t / (1.0 - b2t)
    if sma >= 5.0:
        return True, math.sqrt((1.0 - b2t) * (sma - 4.0) / (sma_max - 4.0) * (sma - 2.0) / sma * sma_max / (sma_max - 2.0)) / (1.0 - b1t), sma
    return False, 1.0 / (1.0 - b1t), sma


def adam_coef(t, beta1, beta2):
    """float64: (1 - beta1^t, sqrt(1 - beta2^t))"""
    return 1.0 - beta1 ** t, math.sqrt(1.0 - beta2 ** t)


def _powf(b, t):
    """float32 powf, taken as correctly rounded"""
    return F(float(b) ** float(t))


def today_coef(kind, t, beta1, beta2):
    """The coefficients as the kernels computed them before they moved to double: float32 pow, float32 sma, the kernel's evaluation
    order.  kind 0 -> (rect, step), kind 1 -> (bc1, bc2s); np.float32 scalars."""
    one, two, t = F(1), F(2), F(t)
    b1, b2 = F(beta1), F(beta2)
    with np.errstate(all="ignore"):
        b2t, b1t = _powf(b2, t), _powf(b1, t)
        if kind == 1:
            return one - b1t, np.sqrt(one - b2t)
        sma_max = two / (one - b2) - one
        sma = sma_max - two * t * b2t / (one - b2t)
        if sma >= F(5):
            return True, np.sqrt((one - b2t) * (sma - F(4)) / (sma_max - F(4)) * (sma - two) / sma * sma_max / (sma_max - two)) / (one - b1t)
        return False, one / (one - b1t)


# ------------------------------------------------------------------------------------------------------------------------------
# 2. one step: float64 reference with its bound
# ------------------------------------------------------------------------------------------------------------------------------
def _dsqrt(v, tol_v):
    lo = np.sqrt(np.maximum(v - tol_v, 0.0))
    den = np.sqrt(v) + lo
    return np.where(den > 0, tol_v / np.where(den > 0, den, 1.0), np.sqrt(tol_v))


def ref_step(kind, theta, grad, m, v, state, lr, p1, p2, eps, grad_scale, tick=1, force_rect=None):
    """One optimizer step in float64 as include/gcpx.h defines it.  theta, grad, m, v: arrays of float32 values; state: 4 values;
    hyperparameters: rounded to float32 and widened (module docstring).  Returns a dict: theta, m, v, state (float64), tol_theta, tol_m,
    tol_v (the bounds of the module docstring), writes_m / writes_v (False: the vector keeps its bits), rect (kind 0).
    force_rect: take that rectification decision instead of sma >= 5 (to ask which decision an implementation took)."""
    th, gr, m0, v0 = (np.asarray(x, dtype=np.float64) for x in (theta, grad, m, v))
    st = np.asarray(state, dtype=np.float64).copy()
    lr, p1, p2, eps, gs = f32(lr), f32(p1), f32(p2), f32(eps), f32(grad_scale)
    z = np.zeros_like(th)
    out = dict(theta=th.copy(), m=m0.copy(), v=v0.copy(), state=st, tol_theta=z, tol_m=z, tol_v=z, writes_m=False, writes_v=False, rect=None)
    if st[3] != 0.0:                                     # the gate: nothing moves, whatever kind and tick
        return out
    t = float(F(st[0]) + F(1))                           # the counter is a float: exact to 2^24, then it stays
    g = gr * (gs * clip_factor(st[1]))
    ag = np.abs(g)
    if kind in (0, 1):
        A, B = p1 * m0, (1.0 - p1) * g
        mi = A + B
        tol_m = SECOND * (gam(2) * np.abs(A) + gam(5) * np.abs(B)) + 3 * TINY
        out.update(m=mi, tol_m=tol_m, writes_m=True)
    if kind in (0, 1, 2):
        A, B = p2 * v0, (1.0 - p2) * g * g
        vi = A + B
        tol_v = SECOND * (gam(2) * np.abs(A) + gam(8) * np.abs(B)) + 4 * TINY
        dsq = _dsqrt(vi, tol_v)
        out.update(v=vi, tol_v=tol_v, writes_v=True)
    if kind == 0:
        rect, step, _ = radam_coef(t, p1, p2)
        if force_rect is not None and force_rect != rect:
            b2t, sma_max = p2 ** t, 2.0 / (1.0 - p2) - 1.0
            sma = sma_max - 2.0 * t * b2t / (1.0 - b2t)
            rect = force_rect
            step = (math.sqrt(abs((1.0 - b2t) * (sma - 4.0) / (sma_max - 4.0) * (sma - 2.0) / sma * sma_max / (sma_max - 2.0))) if rect
                    else 1.0) / (1.0 - p1 ** t)
        out["rect"] = rect
        c = lr * step
        if rect:
            d = np.sqrt(vi) + eps
            upd = c * mi / d
            tol_u = gam(9) * np.abs(upd) + abs(c) / d * tol_m + np.abs(upd) * dsq / d
        else:
            upd = c * mi
            tol_u = gam(4) * np.abs(upd) + abs(c) * tol_m
    elif kind == 1:
        bc1, bc2s = adam_coef(t, p1, p2)
        c = lr / bc1
        d = np.sqrt(vi) / bc2s + eps
        upd = c * mi / d
        tol_u = gam(14) * np.abs(upd) + abs(c) / d * tol_m + np.abs(upd) * (dsq / bc2s) / d
    elif kind == 2:
        d = np.sqrt(vi) + eps
        q = g / d
        tol_q = gam(7) * np.abs(q) + np.abs(q) * dsq / d + TINY
        if p1 > 0:
            A = p1 * m0
            mi = A + q
            tol_m = SECOND * (gam(2) * np.abs(A) + gam(1) * np.abs(q) + tol_q) + TINY
            out.update(m=mi, tol_m=tol_m, writes_m=True)
            upd = lr * mi
            tol_u = gam(1) * np.abs(upd) + lr * tol_m
        else:
            upd = lr * q
            tol_u = gam(1) * np.abs(upd) + lr * tol_q
    elif kind == 3:
        if p1 > 0:
            if t == 1.0:                                 # torch.optim.SGD: the momentum buffer STARTS as the gradient
                mi, tol_m = g.copy(), SECOND * gam(2) * ag + TINY
            else:
                A = p1 * m0
                mi, tol_m = A + g, SECOND * (gam(2) * np.abs(A) + gam(3) * ag) + 2 * TINY
            out.update(m=mi, tol_m=tol_m, writes_m=True)
            upd = lr * mi
            tol_u = gam(1) * np.abs(upd) + lr * tol_m
        else:
            upd = lr * g
            tol_u = gam(3) * np.abs(upd)
    else:
        raise ValueError(kind)
    out["theta"] = th - upd
    out["tol_theta"] = SECOND * tol_u + TINY + EPS * np.abs(out["theta"])
    if tick:
        st[0] = float(F(st[0]) + F(1))
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# 3. one step: float32 restatement, operation by operation, with the planted mistakes
# ------------------------------------------------------------------------------------------------------------------------------
MISTAKES = ("swap_beta1", "swap_beta2", "scale_once_in_gg", "clip_twice", "eps_in_sqrt", "adam_no_v_correction", "rmsprop_eps_inside",
            "rect_threshold_4", "rect_4_as_2", "sgd_no_first_step", "unset_is_zero")
# `>` for `>=` at the threshold is no member: no case can tell it from the right comparison (test_optim_refs_cpu.py, rectification table)
EQUIVALENT_MUTANTS = ("rect_gt",)


def _f32_radam_coef(t, p1, p2, mistake):
    """(rect, step as float32): float64 arithmetic on the widened hyperparameters, rounded once"""
    b2t, b1t = p2 ** t, p1 ** t
    sma_max = 2.0 / (1.0 - p2) - 1.0
    sma = sma_max - 2.0 * t * b2t / (1.0 - b2t)
    rect = sma > 5.0 if mistake == "rect_gt" else (sma >= 4.0 if mistake == "rect_threshold_4" else sma >= 5.0)
    if not rect:
        return False, F(1.0 / (1.0 - b1t))
    d4 = (sma_max - 2.0) if mistake == "rect_4_as_2" else (sma_max - 4.0)
    return True, F(math.sqrt(max((1.0 - b2t) * (sma - 4.0) / d4 * (sma - 2.0) / sma * sma_max / (sma_max - 2.0), 0.0)) / (1.0 - b1t))


def f32_step(kind, theta, grad, m, v, state, lr, p1, p2, eps, grad_scale, tick=1, coef="exact", mistake=None):
    """The same step in numpy float32, one rounding per operation.  coef: "exact" = scalar coefficients in float64, rounded once;
    "today" = today_coef.  mistake: one of MISTAKES / EQUIVALENT_MUTANTS.  Returns dict theta, m, v, state (float32)."""
    th, gr, m0, v0 = (np.array(x, dtype=np.float32) for x in (theta, grad, m, v))
    st = np.array(state, dtype=np.float32)
    out = dict(theta=th, m=m0, v=v0, state=st)
    if st[3] != 0:
        return out
    lr, p1, p2, eps, gs = F(lr), F(p1), F(p2), F(eps), F(grad_scale)
    one = F(1)
    t = st[0] + one
    s1 = st[1]
    fac = s1 if s1 > 0 else (F(0) if s1 < 0 else (F(0) if mistake == "unset_is_zero" else one))
    with np.errstate(all="ignore"):
        gsc = gs * fac
        if mistake == "clip_twice":
            gsc = gsc * fac
        g = gr * gsc
        g2 = gr * fac if mistake == "scale_once_in_gg" else g         # the second factor of g g
        if kind in (0, 1):
            mi = (one - p1) * m0 + p1 * g if mistake == "swap_beta1" else p1 * m0 + (one - p1) * g
            out["m"] = mi
        if kind in (0, 1, 2):
            vi = (one - p2) * v0 + p2 * g * g2 if mistake == "swap_beta2" else p2 * v0 + (one - p2) * g * g2
            out["v"] = vi
        if kind == 0:
            rect, step = today_coef(0, t, p1, p2) if coef == "today" else _f32_radam_coef(float(t), float(p1), float(p2), mistake)
            if rect:
                d = np.sqrt(vi + eps) if mistake == "eps_in_sqrt" else np.sqrt(vi) + eps
                upd = lr * step * mi / d
            else:
                upd = lr * step * mi
        elif kind == 1:
            if coef == "today":
                bc1, bc2s = today_coef(1, t, p1, p2)
            else:
                bc1, bc2s = (F(x) for x in adam_coef(float(t), float(p1), float(p2)))
            if mistake == "adam_no_v_correction":
                bc2s = one
            d = np.sqrt(vi + eps) / bc2s if mistake == "eps_in_sqrt" else np.sqrt(vi) / bc2s + eps
            upd = lr / bc1 * mi / d
        elif kind == 2:
            q = g / (np.sqrt(vi + eps) if mistake == "rmsprop_eps_inside" else np.sqrt(vi) + eps)
            if p1 > 0:
                out["m"] = p1 * m0 + q
                upd = lr * out["m"]
            else:
                upd = lr * q
        else:
            if p1 > 0:
                out["m"] = g.copy() if (t == one and mistake != "sgd_no_first_step") else p1 * m0 + g
                upd = lr * out["m"]
            else:
                upd = lr * g
        out["theta"] = th - upd
        if tick:
            st[0] = t
    for k in ("theta", "m", "v"):
        assert out[k].dtype == np.float32, k
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# 4. holding a result to the reference
# ------------------------------------------------------------------------------------------------------------------------------
def bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.int32)


def ratio(got, ref, tol, name):
    """worst |got - ref| / tol over the elements; raises when an element is not finite or outside its tolerance"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    tol = np.broadcast_to(np.asarray(tol, dtype=np.float64), ref.shape)
    assert got.shape == ref.shape, f"{name}: {got.shape} against {ref.shape}"
    if not np.isfinite(got).all():
        raise AssertionError(f"{name}: {int((~np.isfinite(got)).sum())} elements not written (or not finite)")
    err = np.abs(got - ref)
    r = np.where(err == 0, 0.0, err / np.maximum(tol, 1e-300))
    bad = err > tol
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise AssertionError(f"{name}: {int(bad.sum())}/{bad.size} elements outside the bound; first at {i}: got {got.flat[i]!r} want "
                             f"{ref.flat[i]!r} tol {tol.flat[i]:.3e}; worst err/tol {r.max():.3g}")
    return float(r.max()) if r.size else 0.0


def check_step(name, case, after, force_rect=None):
    """`after` (dict theta, m, v, state: what an implementation left) against ref_step on `case` (dict kind, theta, grad, m, v, state, hp
    = (lr, p1, p2, eps, grad_scale), tick).  theta, m, v within their bounds (a vector the kind does not write: same bits); state[0]
    exact, state[1..3] the same bits.  Returns the worst error / tolerance."""
    r = ref_step(case["kind"], case["theta"], case["grad"], case["m"], case["v"], case["state"], *case["hp"], tick=case.get("tick", 1),
                 force_rect=force_rect)
    worst = ratio(after["theta"], r["theta"], r["tol_theta"], f"{name} theta")
    for k in ("m", "v"):
        if r["writes_" + k]:
            worst = max(worst, ratio(after[k], r[k], r["tol_" + k], f"{name} {k}"))
        else:
            assert np.array_equal(bits(after[k]), bits(case[k])), f"{name}: {k} changed, and kind {case['kind']} does not write it"
    st = np.asarray(after["state"], dtype=np.float32)
    assert float(st[0]) == r["state"][0], f"{name}: state[0] = {float(st[0])!r}, want {r['state'][0]!r}"
    assert np.array_equal(bits(st[1:]), bits(np.asarray(case["state"], dtype=np.float32)[1:])), f"{name}: state[1..3] changed"
    return worst


def step_args(case):
    return (case["kind"], case["theta"], case["grad"], case["m"], case["v"], case["state"]) + tuple(case["hp"])


# ------------------------------------------------------------------------------------------------------------------------------
# 5. gcpx_grad_clip_coef
# ------------------------------------------------------------------------------------------------------------------------------
def ref_clip(grad, grad_scale, max_norm):
    """torch.nn.utils.clip_grad_norm_ over one flat vector, float64: (norm of grad_scale x grad, min(1, max_norm / (norm + 1e-6)),
    1 when max_norm <= 0).  The kernel's state[1] holds -1 where this coefficient is 0 (clip_factor)."""
    g = np.asarray(grad, dtype=np.float64)
    norm = abs(f32(grad_scale)) * math.sqrt(float(np.sum(g * g)))
    mx = f32(max_norm)
    return norm, (min(1.0, mx / (norm + 1e-6)) if mx > 0 else 1.0)


def clip_depth(n, n_partial):
    """roundings on the way of one square into the sum, in the fixed order of the two launches: the square 1, the serial trips of a
    thread ceil(n / (256 n_partial)), the 8 levels of the 256-thread tree; the second stage: ceil(n_partial / 256) serial additions and
    8 levels again"""
    return 1 + -(-n // (256 * n_partial)) + 8 + -(-n_partial // 256) + 8


def clip_tol(grad, grad_scale, max_norm, n_partial):
    """Bounds (tol_norm, tol_coef).  All terms of the sum of squares are >= 0, so its relative error is <= gam(depth); the root halves
    it; sqrtf 2 u and the product with |grad_scale| 1 u:  tol_norm = norm x (gam(depth) / 2 + gam(3)).
    coef = min(1, max_norm / den), den = norm + 1e-6: den carries tol_norm, the float32 constant (u x 1e-6) and the sum's rounding
    (u den); the quotient 2 u; min(1, .) is 1-Lipschitz:  tol_coef = q x ((tol_norm + u 1e-6) / den + gam(3)), q = max_norm / den; 0 where
    q stays above 1 under twice that error (the coefficient is then exactly 1)."""
    n = int(np.asarray(grad).size)
    norm, coef = ref_clip(grad, grad_scale, max_norm)
    tol_norm = SECOND * norm * (gam(clip_depth(n, n_partial)) / 2 + gam(3)) + TINY
    mx = f32(max_norm)
    if mx <= 0:
        return tol_norm, 0.0
    den = norm + 1e-6
    q = mx / den
    tol_coef = 0.0 if q * (1.0 - 2 * (tol_norm / den + gam(3))) > 1.0 else SECOND * q * ((tol_norm + EPS * 1e-6) / den + gam(3)) + TINY
    return tol_norm, tol_coef


def f32_clip(grad, grad_scale, max_norm, n_partial):
    """gcpx_grad_clip_coef in numpy float32 in the order include/gcpx.h fixes (a deterministic two-stage sum): workgroup b of
    n_partial, thread i adds the squares of elements b 256 + i + k 256 n_partial in turn; a pairwise tree over the 256 threads; then one
    workgroup over the partials the same way.  Returns (state[2], state[1]) as float32, state[1] = -1 for a coefficient of 0."""
    g = np.asarray(grad, dtype=np.float32)
    n = g.size
    per = 256 * n_partial
    trips = -(-n // per)
    pad = np.zeros(trips * per, dtype=np.float32)
    pad[:n] = g
    pad = pad.reshape(trips, n_partial, 256)
    with np.errstate(all="ignore"):
        s = np.zeros((n_partial, 256), dtype=np.float32)
        for k in range(trips):
            s = s + pad[k] * pad[k]

        def tree(x):
            k = 128
            while k:
                x = x[..., :k] + x[..., k:2 * k]
                k >>= 1
            return x[..., 0]
        part = tree(s)
        rows = -(-n_partial // 256)
        p2 = np.zeros(rows * 256, dtype=np.float32)
        p2[:n_partial] = part
        p2 = p2.reshape(rows, 256)
        s2 = np.zeros(256, dtype=np.float32)
        for k in range(rows):
            s2 = s2 + p2[k]
        norm = np.abs(F(grad_scale)) * np.sqrt(tree(s2))
        mx = F(max_norm)
        coef = min(F(1), mx / (norm + F(1e-6))) if mx > 0 else F(1)
    return F(norm), (F(-1) if coef == 0 else F(coef))


# ------------------------------------------------------------------------------------------------------------------------------
# 6. the input sets (one home: the GPU file and the CPU file import them from here)
# ------------------------------------------------------------------------------------------------------------------------------
BETA2S = (0.98, 0.99, 0.995, 0.999, 0.9995, 0.9999)
BETA1S = (0.5, 0.9)
COEF_TS = tuple(range(1, 41)) + (100, 1000, 10 ** 4, 10 ** 5, 10 ** 6, 2 ** 24 - 1, 2 ** 24)
LR = 1e-2


def _rng(seed):
    return np.random.RandomState(seed)


def _case(name, kind, theta, grad, m, v, state, hp, tick=1):
    a = [np.ascontiguousarray(x, dtype=np.float32) for x in (theta, grad, m, v, state)]
    return dict(name=name, kind=kind, theta=a[0], grad=a[1], m=a[2], v=a[3], state=a[4], hp=tuple(hp), tick=tick)


def coef_cases(kind, beta2):
    """a. the coefficients over the step counter: state[0] = t - 1 written by the test, theta0 = 0 (theta afterwards IS the update and
    its bound purely relative), n = 64 gradients of magnitude 1e-6 .. 1e3 with random signs; `cold` m0 = v0 = 0, `warm` moments of the
    gradients' size.  t = 2^24 - 1 lands the counter on 2^24 - 1, t = 2^24 (counter 2^24 - 1 before) on 2^24, where it stays."""
    r = _rng(7)
    n = 64
    grad = np.sign(r.rand(n) - 0.5) * 10.0 ** np.linspace(-6, 3, n)
    warm_m, warm_v = 0.5 * grad * r.randn(n), grad * grad * (0.5 + r.rand(n))
    out = []
    for beta1 in BETA1S:
        for t in COEF_TS:
            for warm in (False, True):
                m0, v0 = (warm_m, warm_v) if warm else (np.zeros(n), np.zeros(n))
                out.append(_case(f"{KIND_NAMES[kind]}-b2={beta2}-b1={beta1}-t={t}-{'warm' if warm else 'cold'}", kind, np.zeros(n), grad, m0, v0,
                                 [t - 1, 0, 0, 0], (LR, beta1, beta2, 1e-8, 1.0)))
                out[-1]["t"] = t
    return out


TRAJ_CONFIGS = {"radam": (0, 0.9, 0.999), "adam": (1, 0.9, 0.999), "rmsprop": (2, 0.0, 0.99), "rmsprop-momentum": (2, 0.9, 0.99),
                "sgd": (3, 0.0, 0.0), "sgd-momentum": (3, 0.9, 0.0)}
TRAJ_STEPS = 12


def traj_case(config, eps, theta_zero):
    """b. twelve steps from state = 0: 1000 gradients N(0, 1) x 10^(2 (k % 3) - 3) (the scale moves by 100 x between steps), then 12
    elements of |g| = 1e-12 and 12 of g = 0 exactly (eps rules: the update is ~0 and v only decays).  -> (first case, gradients [12][n])"""
    kind, p1, p2 = TRAJ_CONFIGS[config]
    r = _rng(11)
    n = 1024
    theta = np.zeros(n) if theta_zero else r.randn(n)
    grads = []
    for k in range(TRAJ_STEPS):
        g = r.randn(n) * 10.0 ** (2 * (k % 3) - 3)
        g[1000:1012] = 1e-12 * np.sign(r.rand(12) - 0.5)
        g[1012:] = 0.0
        grads.append(g.astype(np.float32))
    c = _case(f"{config}-eps={eps}-theta0={'0' if theta_zero else 'N01'}", kind, theta, grads[0], np.zeros(n), np.zeros(n), [0, 0, 0, 0],
              (LR, p1, p2, eps, 1.0))
    return c, grads


def trajectory(step_fn, config, eps, theta_zero):
    """TRAJ_STEPS steps of `step_fn(case) -> dict theta, m, v, state`, each checked against ref_step restarted from the float32 state
    the previous step left.  Returns the worst ratio."""
    c, grads = traj_case(config, eps, theta_zero)
    worst = 0.0
    for k, g in enumerate(grads):
        c = dict(c, grad=g)
        after = step_fn(c)
        worst = max(worst, check_step(f"{c['name']} step {k + 1}", c, after))
        c = dict(c, theta=after["theta"], m=after["m"], v=after["v"], state=after["state"])
    assert float(c["state"][0]) == float(TRAJ_STEPS)
    return worst


def loop_lengths(max_blocks):
    """c. slice lengths for a launch of `max_blocks` workgroups.  The 16-byte loop of the RAdam kernel moves S = 256 max_blocks float4
    per access and two accesses per trip (8 S floats):
      8 S - 4   the last thread's second access falls out of range (`two` false for one thread);  8 S: both exactly full
      8 S + 4   one float4 into a second trip;  8 S + 2: n % 4 == 2, the remainder loop
      12 S + 1  the second trip's first access full, its second out of range for every thread; n % 4 == 1
      20 S + 7  third trip: the second access in range by one float4; n % 4 == 3
    (max_blocks = 1: 2044, 2048, 2052, 2050, 3073, 5127.)  The lengths 1 .. 9 take the scalar kernel (n < 4) or a single float4.
    max_blocks = 0 (no limit) runs the lengths of 1 and 3: every thread then makes at most one trip."""
    small = [1, 2, 3, 4, 5, 7, 8, 9]
    if max_blocks == 0:
        return small + sorted(set(loop_lengths(1)[8:] + loop_lengths(3)[8:]))
    S = 256 * max_blocks
    return small + [8 * S - 4, 8 * S, 8 * S + 4, 8 * S + 2, 12 * S + 1, 20 * S + 7]


LOOP_PAD = 8              # floats of NaN frame in front of a slice (32 bytes: the slice itself starts 16-byte aligned at offset 0)
LOOP_OFFSETS = ((0, 0), (1, 1), (2, 2), (3, 3), (0, 1))       # (offset of theta / m / v, offset of grad) in floats past the frame


def loop_case(kind, n, index):
    """the slice's values: N(0, 1) parameters and gradients, warm moments, counter 6 (past RAdam's switch at beta2 = 0.999); the
    clip coefficient slot holds 0.5 and grad_scale = 0.5; tick alternates with `index`"""
    r = _rng(1000 + 7 * n + kind)
    g = r.randn(n)
    return _case(f"{KIND_NAMES[kind]}-n={n}-#{index}", kind, r.randn(n), g, 0.1 * r.randn(n), 0.01 + 0.1 * r.rand(n), [6, 0.5, 123.0, 0],
                 (LR, 0.9, 0.999, 1e-8, 0.5), tick=index % 2)


SCALE_COEFS = (0.0, 1.0, 0.25, 1e-30, -1.0)          # state[1]: unset, 1, a coefficient, one that underflows g g, "zero"
SCALE_GRAD_SCALES = (1.0, 0.5, 1.0 / 3.0)
SCALE_CONFIGS = ((0, 0.9, 0.999), (1, 0.9, 0.999), (2, 0.9, 0.99), (2, 0.0, 0.99), (3, 0.9, 0.0), (3, 0.0, 0.0))


def scale_cases():
    """d. grad_scale x clip coefficient: n = 257, gradients 10^U(-3, 2), warm moments, counter 0 (t = 1: SGD's momentum buffer must
    START as the gradient whatever m holds) and 7"""
    r = _rng(23)
    n = 257
    grad = np.sign(r.rand(n) - 0.5) * 10.0 ** (5 * r.rand(n) - 3)
    theta, m0, v0 = r.randn(n), 0.3 * grad * r.randn(n), grad * grad * (0.5 + r.rand(n))
    out = []
    for kind, p1, p2 in SCALE_CONFIGS:
        for coef in SCALE_COEFS:
            for gs in SCALE_GRAD_SCALES:
                for t0 in (0, 7):
                    out.append(_case(f"{KIND_NAMES[kind]}-p1={p1}-coef={coef}-scale={gs:.3g}-t0={t0}", kind, theta, grad, m0, v0, [t0, coef, 5.0, 0],
                                     (LR, p1, p2, 1e-8, gs)))
    return out


CLIP_NS = (1, 255, 257, 10007, 262147)
CLIP_PARTIALS = (1, 2, 256, 1024, 4096)
CLIP_MAX_NORMS = (0.5, 1e-3, 0.0, -1.0)
CLIP_GRAD_SCALES = (1.0, 0.5, -0.5)
CLIP_SETS = ("normal", "outlier", "zero", "wide")


def clip_grad(kind, n):
    """e. the gradient sets: N(0, 1); one outlier of 1e6 among values of 1e-3 size; all zero; |g| = 10^U(-15, 15)"""
    r = _rng(31 + n)
    if kind == "normal":
        g = r.randn(n)
    elif kind == "outlier":
        g = 1e-3 * r.randn(n)
        g[n // 2] = 1e6
    elif kind == "zero":
        g = np.zeros(n)
    else:
        g = np.sign(r.rand(n) - 0.5) * 10.0 ** (30 * r.rand(n) - 15)
    return g.astype(np.float32)


OVERFLOW_VALUES = (1e19, 1e20)        # 1000 elements each: the float32 sum of squares is inf (1e38 x 1000), every element finite


def overflow_case(kind, p1, p2, value):
    """1000 gradients of `value` with alternating signs, N(0, 1) parameters, warm moments, counter 7, clip slot unset"""
    r = _rng(41)
    n = 1000
    grad = value * np.where(np.arange(n) % 2, -1.0, 1.0)
    return _case(f"{KIND_NAMES[kind]}-p1={p1}-overflow-{value:g}", kind, r.randn(n), grad, 0.1 * r.randn(n), 0.01 + 0.1 * r.rand(n), [7, 0, 0, 0],
                 (LR, p1, p2, 1e-8, 1.0))
