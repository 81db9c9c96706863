"""gcpx_ema_update and gcpx_swap_f32 (csrc/scalar_f32.hip) on the GPU.

The update against the two-rounding bound of tests/ema_refs.py over every size at which the kernel takes another path (the 16-byte loop,
its second access, the scalar remainder, more than one workgroup), all 16 (ema, theta) offsets from a 16-byte boundary, four decays and
five value classes; NaN canaries around both buffers; the device-side gate; slices; a launch held to one workgroup.  The swap bit for bit.

Launch geometry: 256 threads, two float4 accesses per thread and trip, so a workgroup covers 2048 floats per trip and the grid is
ceil(n / 2048) workgroups (at most 16384) -- at full grid no thread takes a second trip below 33.5 M floats.  N_TRIPS = 9221 under
max_blocks = 2 is the size that does: 2305 float4, of which 2 x 1024 are two full trips of all 512 threads, 257 a ragged third trip
(threads 0 .. 256, their first access only), and one float is left to the scalar loop."""
import numpy as np
import pytest
import torch

import ema_refs as E

pytestmark = pytest.mark.gpu

GUARD = 64                                          # canary floats in front of and behind each range (256 bytes: alignment is `off` alone)
N_TRIPS = 2 * (2 * 256 * 8) + 1029                  # 9221, see above
SIZES = (1, 3, 4, 5, 7, 255, 256, 257, 1023, 1024, 1025, N_TRIPS)
DECAYS = (0.5, 0.9, 0.999, 0.9999)
KINDS = ("normal", "same", "zeros", "tiny", "huge")
OFFSETS = [(a, b) for a in range(4) for b in range(4)]          # (0, 0): the 16-byte loop; every other pair: the scalar loop
CANARY = np.uint32(0x7FC0DEAD)                      # a quiet NaN with a payload


def _st():
    return torch.cuda.current_stream().cuda_stream


def _values(kind, n, seed):
    rng = np.random.RandomState(seed)
    if kind == "normal":
        return rng.randn(n).astype(np.float32), rng.randn(n).astype(np.float32)
    if kind == "same":
        x = rng.randn(n).astype(np.float32)
        return x, x.copy()
    if kind == "zeros":
        z = lambda: np.where(rng.rand(n) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
        return z(), z()
    mag = np.float32(1e-30 if kind == "tiny" else 1e30)
    return (mag * rng.uniform(1, 2, n)).astype(np.float32), (mag * rng.uniform(1, 2, n)).astype(np.float32)


def _framed(values, off):
    """`values` at GUARD + off floats of a buffer of NaN canaries; host uint32 array (bits)"""
    buf = np.full(GUARD + 4 + len(values) + GUARD, CANARY, dtype=np.uint32)
    buf[GUARD + off:GUARD + off + len(values)] = E.bits(values)
    return buf


def _dev(bits):
    t = torch.from_numpy(bits.view(np.int32).copy()).cuda()
    assert t.data_ptr() % 16 == 0
    return t


def _host(t):
    return t.cpu().numpy().view(np.uint32)


def _update(lib, ema_t, oe, theta_t, ot, n, decay, gate=None, max_blocks=0):
    from video_gcp_amd import runtime as rt
    rt.check(lib.gcpx_ema_update(ema_t.data_ptr() + 4 * (GUARD + oe), theta_t.data_ptr() + 4 * (GUARD + ot), n, decay,
                                 None if gate is None else gate.data_ptr(), max_blocks, _st()), "ema_update")


@pytest.mark.parametrize("n", SIZES)
def test_update_within_the_two_rounding_bound(gcpx_lib, n):
    worst = 0.0
    for kind in KINDS:
        e, t = _values(kind, n, 1000 + n)
        for oe, ot in OFFSETS:
            he, ht = _framed(e, oe), _framed(t, ot)
            theta_t = _dev(ht)
            for decay in DECAYS:
                for max_blocks in ((0, 2) if n == N_TRIPS else (0,)):
                    ema_t = _dev(he)
                    _update(gcpx_lib, ema_t, oe, theta_t, ot, n, decay, max_blocks=max_blocks)
                    got = _host(ema_t)
                    name = f"n={n} {kind} ema+{oe} theta+{ot} decay={decay} max_blocks={max_blocks}"
                    lo, hi = GUARD + oe, GUARD + oe + n
                    assert np.array_equal(got[:lo], he[:lo]) and np.array_equal(got[hi:], he[hi:]), name + ": a canary around ema changed"
                    worst = max(worst, E.check_update(got[lo:hi].view(np.float32), e, t, decay, name))
            assert np.array_equal(_host(theta_t), ht), f"n={n} {kind} theta+{ot}: theta or a canary around it changed"
    print(f"n={n}: worst err / bound = {worst:.3g}")


def test_nonfinite_values_propagate(gcpx_lib):
    e = np.array([1.0, np.nan, 2.0, np.inf, -np.inf, 3.0, np.inf, 0.5], dtype=np.float32)
    t = np.array([np.nan, 1.0, np.inf, 2.0, 3.0, -np.inf, np.inf, 0.25], dtype=np.float32)
    ema_t, theta_t = torch.from_numpy(e).cuda(), torch.from_numpy(t).cuda()
    from video_gcp_amd import runtime as rt
    rt.check(gcpx_lib.gcpx_ema_update(ema_t.data_ptr(), theta_t.data_ptr(), 8, 0.9, None, 0, _st()), "ema_update")
    got = ema_t.cpu().numpy()
    # a finite average meeting an infinite theta goes there; an infinite average meets its own infinity with the other sign in
    # omd (theta - ema) and becomes NaN, as does Inf - Inf of one sign; the finite neighbour is untouched by all that
    assert np.isnan(got[[0, 1, 3, 4, 6]]).all() and got[2] == np.inf and got[5] == -np.inf
    E.check_update(got[7:], e[7:], t[7:], 0.9, "the finite element")


def test_gate_is_read_on_the_device(gcpx_lib):
    """the gate is written by a launch on the same stream right in front of the update, with no host sync in between"""
    n = 1025
    e, t = _values("normal", n, 5)
    he, ht = _framed(e, 0), _framed(t, 0)
    theta_t, gate = _dev(ht), torch.zeros(4, device="cuda")
    for vec_off in (0, 1):
        he = _framed(e, vec_off)
        closed, opened, ungated = _dev(he), _dev(he), _dev(he)
        torch.cuda.synchronize()
        gate[3:4].fill_(1.0)                                                   # a kernel on the current stream
        _update(gcpx_lib, closed, vec_off, theta_t, 0, n, 0.9, gate=gate[3:])
        gate[3:4].fill_(-0.0)                                                  # -0 is zero: open
        _update(gcpx_lib, opened, vec_off, theta_t, 0, n, 0.9, gate=gate[3:])
        gate[3:4].fill_(float("nan"))                                          # anything non-zero closes
        _update(gcpx_lib, closed, vec_off, theta_t, 0, n, 0.9, gate=gate[3:])
        _update(gcpx_lib, ungated, vec_off, theta_t, 0, n, 0.9, gate=None)
        torch.cuda.synchronize()
        assert np.array_equal(_host(closed), he), "a closed gate let the update write"
        lo, hi = GUARD + vec_off, GUARD + vec_off + n
        E.check_update(_host(opened)[lo:hi].view(np.float32), e, t, 0.9, "open gate")
        assert not np.array_equal(_host(opened)[lo:hi], he[lo:hi])
        assert np.array_equal(_host(opened), _host(ungated))
    assert np.array_equal(_host(theta_t), ht)


def test_slices_and_one_workgroup_leave_the_bits_of_one_call(gcpx_lib):
    """one call over 9221 elements, the same range cut at 5 points (1001, 2603 and 7777 start 1, 3 and 1 floats off a 16-byte boundary:
    the scalar loop; 4096 and 5000 the 16-byte loop), and one call held to one workgroup"""
    n, decay = N_TRIPS, 0.999
    e, t = _values("normal", n, 9)
    he, ht = _framed(e, 0), _framed(t, 0)
    theta_t = _dev(ht)
    one, cut, single = _dev(he), _dev(he), _dev(he)
    _update(gcpx_lib, one, 0, theta_t, 0, n, decay)
    _update(gcpx_lib, single, 0, theta_t, 0, n, decay, max_blocks=1)
    cuts = (0, 1001, 2603, 4096, 5000, 7777, n)
    assert sum(1 for c in cuts[1:-1] if c % 4) >= 3 and len(cuts) == 7
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        _update(gcpx_lib, cut, lo, theta_t, lo, hi - lo, decay)
    E.check_update(_host(one)[GUARD:GUARD + n].view(np.float32), e, t, decay, "one call")
    assert np.array_equal(_host(cut), _host(one)), "slices differ from one call"
    assert np.array_equal(_host(single), _host(one)), "max_blocks = 1 differs from the full grid"


def _swap_values(n, seed):
    rng = np.random.RandomState(seed)
    a, b = rng.randint(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32), rng.randint(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    special = np.array([0x80000000, 0x7FC00001, 0xFFC12345, 0x7F800001, 0x00000001, 0x7F800000], dtype=np.uint32)      # -0, NaN payloads (quiet, signalling), a subnormal, Inf
    a[:min(n, 6)] = special[:min(n, 6)]
    b[-min(n, 6):] = special[:min(n, 6)]
    a[a == CANARY] ^= np.uint32(1)
    b[b == CANARY] ^= np.uint32(1)
    return a, b


@pytest.mark.parametrize("n", SIZES)
def test_swap_exchanges_bits(gcpx_lib, n):
    from video_gcp_amd import runtime as rt
    a, b = _swap_values(n, 2000 + n)
    for oa, ob in OFFSETS:
        for max_blocks in ((0, 1, 2) if n == N_TRIPS else (0,)):
            ha, hb = _framed(a.view(np.float32), oa), _framed(b.view(np.float32), ob)
            ta, tb = _dev(ha), _dev(hb)
            pa, pb = ta.data_ptr() + 4 * (GUARD + oa), tb.data_ptr() + 4 * (GUARD + ob)
            rt.check(gcpx_lib.gcpx_swap_f32(pa, pb, n, max_blocks, _st()), "swap_f32")
            wa, wb = ha.copy(), hb.copy()
            wa[GUARD + oa:GUARD + oa + n], wb[GUARD + ob:GUARD + ob + n] = b, a
            name = f"n={n} a+{oa} b+{ob} max_blocks={max_blocks}"
            assert np.array_equal(_host(ta), wa), name + ": a is not b's bits inside unchanged canaries"
            assert np.array_equal(_host(tb), wb), name + ": b is not a's bits inside unchanged canaries"
            rt.check(gcpx_lib.gcpx_swap_f32(pa, pb, n, max_blocks, _st()), "swap_f32")
            assert np.array_equal(_host(ta), ha) and np.array_equal(_host(tb), hb), name + ": swapping twice does not restore"


def test_arguments_on_the_device(gcpx_lib):
    x = torch.zeros(16, device="cuda")
    st = _st()
    assert gcpx_lib.gcpx_ema_update(x.data_ptr(), x.data_ptr() + 32, 0, 0.9, None, 0, st) == 0
    assert gcpx_lib.gcpx_swap_f32(x.data_ptr(), x.data_ptr() + 32, 0, 0, st) == 0
    assert gcpx_lib.gcpx_ema_update(x.data_ptr(), x.data_ptr() + 32, 4, 1.0, None, 0, st) == -1
    assert gcpx_lib.gcpx_ema_update(x.data_ptr(), x.data_ptr() + 32, -1, 0.9, None, 0, st) == -1
    assert gcpx_lib.gcpx_swap_f32(x.data_ptr(), None, 4, 0, st) == -1
    torch.cuda.synchronize()
    assert not x.any()
