"""-m gpu: gcpx_attention_bwd_heads, gcpx_row_layernorm and gcpx_row_layernorm_bwd (csrc/adaptive.hip) against the float64 restatements
and derived bounds of tests/attn_refs.py (pinned without a GPU by tests/test_attn_refs_cpu.py).

Conventions of tests/test_gpu_backward_kernels.py: the kernels are called through video_gcp_amd.runtime as their call sites in
backward_stages._attention_backward and forward_plan._plan_attention call them; every output starts as NaN, so an element a kernel must
write and does not is found, and one it must leave alone still holds the NaN.

Shapes (dk 32, nz 128, three sequences): T = 37 and 300 (below and above one 256-thread trip over the frames), 1, 2, 4 and 8 heads
(8: the minimal head widths 4 and 16), 1 and 5 query rows per sequence, end_ind = [T - 1, 0, 20] (whole window, a one-frame window whose
dS and dq are all zero, an interior cut), temperature 0.6.  dK / dV go into the middle one of three column blocks of wider buffers,
as the (level, layer) blocks of the backward plan lie side by side."""
import ctypes as C
import functools

import pytest
import torch

import attn_refs as R

pytestmark = pytest.mark.gpu

NAN = float("nan")
NBLK, BLK = 3, 1


@pytest.fixture(scope="module")
def env():
    from video_gcp_amd import runtime as rt
    lib = rt.load_library()
    assert torch.cuda.is_available()
    return rt, lib


def _st():
    return torch.cuda.current_stream().cuda_stream


def _nan(*shape):
    return torch.full(shape, NAN, device="cuda")


@functools.lru_cache(maxsize=None)
def _reference(T, rpb, heads):
    """float64 gradients and bounds of one case, computed once on the CPU"""
    c = {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in R.mha_case(T, rpb).items()}
    args = (c["q"], c["k"], c["v"], c["end"], c["temp"], heads, rpb, c["dout"])
    return R.mha_grads(*args), R.mha_bounds(*args)


def _worst(got, ref, bound, name):
    got = got.double().cpu()
    assert bool(torch.isfinite(got).all()), f"{name}: {int((~torch.isfinite(got)).sum())} elements not written (or not finite)"
    ratio = float(((got - ref).abs() / bound).max())
    assert ratio <= 1.0, f"{name}: worst error / bound {ratio:.3g}"
    return ratio


def _run_heads(env, T, rpb, heads):
    rt, lib = env
    c = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in R.mha_case(T, rpb).items()}
    M, dk, nz, B = c["q"].shape[0], R.DK, R.NZ, R.B_SEQ
    tmp = torch.tensor([c["temp"]], device="cuda")
    stats, dS, dq, dtr = _nan(M, heads, 2), _nan(M, heads, T), _nan(M, dk), _nan(M)
    dKb, dVb = _nan(B * T, NBLK * dk), _nan(B * T, NBLK * nz)
    rt.check(lib.gcpx_attention_bwd_heads(c["q"].data_ptr(), c["k"].data_ptr(), c["v"].data_ptr(), c["dout"].data_ptr(), c["end"].data_ptr(),
                                          tmp.data_ptr(), stats.data_ptr(), dS.data_ptr(), dq.data_ptr(), dtr.data_ptr(),
                                          dKb.data_ptr() + 4 * BLK * dk, NBLK * dk, dVb.data_ptr() + 4 * BLK * nz, NBLK * nz, M, rpb, T, dk,
                                          nz, heads, _st()), "attention_bwd_heads")
    torch.cuda.synchronize()
    return c, tmp, dict(stats=stats, dS=dS, dq=dq, dtemp_row=dtr, dKb=dKb, dVb=dVb)


@pytest.mark.parametrize("rpb", R.RPB_CASES)
@pytest.mark.parametrize("heads", R.HEAD_CASES)
@pytest.mark.parametrize("T", R.T_CASES)
def test_attention_bwd_heads_vs_float64(env, T, heads, rpb):
    rt, lib = env
    c, tmp, out = _run_heads(env, T, rpb, heads)
    M, dk, nz, B = c["q"].shape[0], R.DK, R.NZ, R.B_SEQ
    for j in range(NBLK):
        if j != BLK:
            assert bool(torch.isnan(out["dKb"][:, j * dk:(j + 1) * dk]).all()) and bool(torch.isnan(out["dVb"][:, j * nz:(j + 1) * nz]).all())
    dK = out["dKb"][:, BLK * dk:(BLK + 1) * dk].reshape(B, T, dk)
    dV = out["dVb"][:, BLK * nz:(BLK + 1) * nz].reshape(B, T, nz)
    ref, bnd = _reference(T, rpb, heads)
    w = {name: _worst(got, ref[name], bnd[name], name)
         for name, got in (("dS", out["dS"]), ("dq", out["dq"]), ("dK", dK), ("dV", dV), ("dtemp_row", out["dtemp_row"]))}
    print(f"attention_bwd_heads T={T} heads={heads} rpb={rpb}: worst error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in w.items()))
    assert bool(torch.isfinite(out["stats"]).all())
    # rows of dK / dV past end_ind are written, as zeros; the one-frame window gives no gradient to scores or query
    for b, e in enumerate(R.end_ind(T).tolist()):
        assert bool((dK[b, e + 1:] == 0).all()) and bool((dV[b, e + 1:] == 0).all())
    assert bool((out["dS"][rpb:2 * rpb] == 0).all()) and bool((out["dq"][rpb:2 * rpb] == 0).all())
    if heads == 1:
        # one head: the bits of gcpx_attention_bwd on the forward's saved weights
        o, att = _nan(M, nz), _nan(M, T)
        rt.check(lib.gcpx_attention(c["q"].data_ptr(), c["k"].data_ptr(), c["v"].data_ptr(), None, c["end"].data_ptr(), tmp.data_ptr(),
                                    o.data_ptr(), att.data_ptr(), M, rpb, T, dk, nz, 1, _st()), "attention")
        dS1, dq1, dtr1 = _nan(M, T), _nan(M, dk), _nan(M)
        dKb1, dVb1 = _nan(B * T, NBLK * dk), _nan(B * T, NBLK * nz)
        rt.check(lib.gcpx_attention_bwd(c["q"].data_ptr(), c["k"].data_ptr(), c["v"].data_ptr(), att.data_ptr(), c["dout"].data_ptr(),
                                        c["end"].data_ptr(), tmp.data_ptr(), dS1.data_ptr(), dq1.data_ptr(), dtr1.data_ptr(),
                                        dKb1.data_ptr() + 4 * BLK * dk, NBLK * dk, dVb1.data_ptr() + 4 * BLK * nz, NBLK * nz, M, rpb, T, dk,
                                        nz, _st()), "attention_bwd")
        torch.cuda.synchronize()
        bits = lambda t: t.view(torch.int32)
        for name, a, b in (("dS", out["dS"][:, 0], dS1), ("dq", out["dq"], dq1), ("dtemp_row", out["dtemp_row"], dtr1),
                           ("dK", out["dKb"], dKb1), ("dV", out["dVb"], dVb1)):
            assert torch.equal(bits(a.contiguous()), bits(b)), f"{name}: not the bits of gcpx_attention_bwd"


def test_attention_bwd_heads_runs_twice_to_the_same_bits(env):
    _, _, a = _run_heads(env, 300, 5, 4)
    _, _, b = _run_heads(env, 300, 5, 4)
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k


def test_invalid_sizes_return_the_error_code(env):
    """checked before anything is launched: the outputs stay as they were"""
    rt, lib = env
    M, rpb, T, dk, nz = 6, 2, 12, 32, 128
    buf = {n: _nan(4096) for n in ("q", "k", "v", "dout", "temp", "stats", "dS", "dq", "dtr", "dK", "dV")}
    end = torch.zeros(8, dtype=torch.int64, device="cuda")

    def call(M=M, rpb=rpb, T=T, dk=dk, nz=nz, heads=2, null=None):
        p = {n: (None if n == null else t.data_ptr()) for n, t in buf.items()}
        e = None if null == "end" else end.data_ptr()
        return lib.gcpx_attention_bwd_heads(p["q"], p["k"], p["v"], p["dout"], e, p["temp"], p["stats"], p["dS"], p["dq"], p["dtr"], p["dK"],
                                            dk, p["dV"], nz, M, rpb, T, dk, nz, heads, _st())

    for null in list(buf) + ["end"]:
        assert call(null=null) == -1, f"null {null}"
    bad = dict(too_long=dict(T=4097), no_frames=dict(T=0), no_rows=dict(M=0), ragged_rows=dict(M=5), no_heads=dict(heads=0),
               dk_not_divisible=dict(heads=3, dk=32, nz=129), nz_not_divisible=dict(heads=4, dk=32, nz=130),
               key_head_width_2=dict(heads=4, dk=8), value_head_width_6=dict(heads=4, dk=32, nz=24),
               value_quarter_3=dict(heads=2, dk=32, nz=24), key_quarter_3=dict(heads=2, dk=24, nz=128),
               weights_past_lds=dict(M=8194, rpb=4097, heads=2))
    for name, kw in bad.items():
        assert call(**kw) == -1, name
        assert b"gcpx_attention_bwd_heads" in lib.gcpx_last_error()
    for W in (0, 30, 1028):
        assert lib.gcpx_row_layernorm(buf["q"].data_ptr(), None, buf["dq"].data_ptr(), None, 3, W, C.c_float(1e-5), _st()) == -1, W
        assert lib.gcpx_row_layernorm_bwd(buf["q"].data_ptr(), buf["k"].data_ptr(), buf["v"].data_ptr(), buf["dq"].data_ptr(), 3, W, _st()) == -1
    assert lib.gcpx_row_layernorm(None, None, buf["dq"].data_ptr(), None, 3, 32, C.c_float(1e-5), _st()) == -1
    assert lib.gcpx_row_layernorm_bwd(buf["q"].data_ptr(), buf["k"].data_ptr(), None, buf["dq"].data_ptr(), 3, 32, _st()) == -1
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in buf.values())


@pytest.mark.parametrize("with_add", [False, True])
@pytest.mark.parametrize("W", [32, 128])
def test_row_layernorm_forward_and_backward_vs_float64(env, W, with_add):
    """rows of nz_attn_key = 32 and nz_enc = 128 floats; 7 rows (the last group of four wavefronts is partial), one of them constant
    (variance 0: the output is rounding noise times 1 / sqrt(1e-5), which the bound allows for and no more)"""
    rt, lib = env
    c = R.layernorm_case(W, with_add)
    c64 = {k: (v.double() if v is not None else None) for k, v in c.items()}
    x, dy = c["x"].cuda(), c["dy"].cuda()
    add = c["add"].cuda() if with_add else None
    rows = x.shape[0]
    y, rstd, dx = _nan(rows + 1, W), _nan(rows + 1), _nan(rows + 1, W)
    rt.check(lib.gcpx_row_layernorm(x.data_ptr(), rt.ptr(add), y.data_ptr(), rstd.data_ptr(), rows, W, C.c_float(R.LN_EPS), _st()), "layernorm")
    rt.check(lib.gcpx_row_layernorm_bwd(dy.data_ptr(), y.data_ptr(), rstd.data_ptr(), dx.data_ptr(), rows, W, _st()), "layernorm_bwd")
    y2 = _nan(rows, W)
    rt.check(lib.gcpx_row_layernorm(x.data_ptr(), rt.ptr(add), y2.data_ptr(), None, rows, W, C.c_float(R.LN_EPS), _st()), "layernorm (no rstd)")
    torch.cuda.synchronize()
    assert bool(torch.isnan(y[rows]).all()) and bool(torch.isnan(rstd[rows])) and bool(torch.isnan(dx[rows]).all())      # the row past the last
    y, rstd, dx = y[:rows], rstd[:rows], dx[:rows]
    assert torch.equal(y.view(torch.int32), y2.view(torch.int32))
    y64, rstd64 = R.layernorm(c64["x"], c64["add"])
    by, brs = R.layernorm_bound(c64["x"], c64["add"])
    w = [_worst(y, y64, by, "y"), _worst(rstd, rstd64, brs, "rstd")]
    ys, rs = y.double().cpu(), rstd.double().cpu()                   # the backward is judged on the y and rstd it was handed
    w.append(_worst(dx, R.layernorm_bwd(c64["dy"], ys, rs), R.layernorm_bwd_bound(c64["dy"], ys, rs), "dx"))
    print(f"row_layernorm W={W} add={with_add}: worst error / bound y {w[0]:.3f}, rstd {w[1]:.3f}, dx {w[2]:.3f}")
