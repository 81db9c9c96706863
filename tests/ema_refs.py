"""Float64 reference and error bound of gcpx_ema_update (csrc/scalar_f32.hip), and the warm-up sequence of the trainer's decay.

The kernel's spec (include/gcpx.h), per element, in float32 with omd = fl(1 - decay) formed once:
    d   = fl(theta - ema)            = (theta - ema) (1 + d1),            |d1| <= u = 2^-24
    got = fl(omd d + ema)  (one fma) = (omd d + ema) (1 + d2),            |d2| <= u
so, with e* = ema + omd (theta - ema) in exact arithmetic on the float32 inputs and the float32 omd,
    got - e* = omd (theta - ema) d1 (1 + d2) + e* d2
    |got - e*| <= u (omd |theta - ema| (1 + u) + |e*|) <= u (omd |theta - ema| + |e*|) (1 + u).
The bound below carries (1 + 2^-23) in place of (1 + u): the other 2^-24 covers the float64 evaluation of e* and of the bound itself
(each a handful of roundings of 2^-53).  Where theta == ema the difference is an exact 0 and fma(omd, 0, ema) == ema: equality, no
tolerance (a -0 comes back as +0: 0 + -0 = +0 in round-to-nearest, equal as a number).  No fitted constant anywhere.
(A subtraction of two floats is exact when its result is subnormal, and no case of the tests puts the fma's result there.)"""
import numpy as np

U = 2.0 ** -24


def omd32(decay):
    """1 - decay as the kernel forms it: both operands and the result float32 (exact for decay >= 0.5, Sterbenz)"""
    return np.float32(1.0) - np.float32(decay)


def ref_update(ema, theta, decay):
    """(e*, bound): float64 arrays from float32 (or float64-held float32) inputs"""
    e, t = np.asarray(ema, dtype=np.float64), np.asarray(theta, dtype=np.float64)
    omd = float(omd32(decay))
    with np.errstate(invalid="ignore", over="ignore"):
        diff = t - e
        estar = e + omd * diff
        bound = U * (omd * np.abs(diff) + np.abs(estar)) * (1.0 + 2.0 ** -23)
    return estar, bound


def check_update(got, ema, theta, decay, what):
    """got (float32, the device's) against ref_update(ema, theta, decay); returns the worst err / bound over the elements with a bound > 0"""
    got64 = np.asarray(got, dtype=np.float64)
    estar, bound = ref_update(ema, theta, decay)
    same = np.asarray(ema) == np.asarray(theta)
    assert np.array_equal(got64[same], np.asarray(ema, dtype=np.float64)[same]), f"{what}: an element with theta == ema moved"
    err = np.abs(got64 - estar)
    bad = ~(err <= bound)
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.size} elements outside the two-rounding bound; first at "
                           f"{int(np.flatnonzero(bad)[0])}: got {got64[bad][0]!r}, e* {estar[bad][0]!r}, bound {bound[bad][0]!r}")
    pos = bound > 0
    return float((err[pos] / bound[pos]).max()) if pos.any() else 0.0


def warmup_decay(decay, t, warmup=True):
    """decay of update t (0-based): TensorFlow's ExponentialMovingAverage(num_updates) rule"""
    return min(decay, (1.0 + t) / (10.0 + t)) if warmup else decay


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
