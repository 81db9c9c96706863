"""No GPU: pins tests/gemm_refs.py, the float64 reference and rounding bounds tests/test_gpu_gemm_forms.py holds every gemm_tile body of
the exact row GEMM to.
  1. evaluate(p, float64) equals F.linear on the concatenated rows, F.conv1d (padding 1) behind an affine + LeakyReLU, and
     torch.nn.LSTMCell, all in float64, to 1e-12; the per-row-block sums equal explicit sums;
  2. torch's own float32 result, evaluate(p, float32), stays inside every bound on every case the GPU file runs: the bounds can be met
     without the code under test;
  3. the same float32 result with ONE k-group of 16 columns dropped, or counted twice, falls outside the bound on every case;
  4. gcpx_gemm_form, which makes no HIP launch and assumes 256 CUs without a device, answers the form, block shape and grid each case
     is named for — the forced one-wavefront forms under their environment, the split-K forms from the cost models."""
import ctypes as C
import dataclasses

import pytest
import torch
import torch.nn.functional as F

import gemm_refs as R

CASES = R.all_cases()


def _close(a, b, what):
    err = (a.double() - b.double()).abs()
    lim = 1e-12 * torch.maximum(a.double().abs(), b.double().abs()) + 1e-13
    assert bool((err <= lim).all()), (what, float(err.max()))


# ------------------------------------------------------------------------------------------------------------------------------
# 1. the reference against torch's operators in float64
# ------------------------------------------------------------------------------------------------------------------------------
def test_reference_equals_linear_on_concatenated_padded_rows():
    p = R.tails_case(("W", 2, 2), "k272")
    xs = [torch.as_strided(p.xbuf, (p.M, s.width), (s.sr, 1), s.off) for s in p.srcs]
    want = F.linear(torch.cat(xs, 1).double(), p.w[0].double(), p.bias[0].double())
    got = R.evaluate(p)
    _close(got["pre"][0], want, "linear")
    assert got["out"] is got["pre"]


def test_reference_equals_conv1d_behind_affine_lrelu_and_gather():
    p = R.sources_case(("W", 4, 2))                  # M = 69 rows in batches of 20: the last batch is cut after 9 rows
    B, T, Cc = -(-p.M // p.rpb), p.rpb, p.srcs[0].width
    s0 = p.srcs[0]
    x = torch.as_strided(p.xbuf, (B, T, Cc), (s0.sb, s0.sr, 1), s0.off).double()
    xa = F.leaky_relu(x * s0.scale.double() + s0.shiftv.double(), R.SLOPE)
    wc = p.w[0, :, :3 * Cc].double().view(p.N, 3, Cc).permute(0, 2, 1)              # [N][C][tap]: source d holds tap d + 1
    conv = F.conv1d(xa.transpose(1, 2), wc, None, padding=1).transpose(1, 2).reshape(B * T, p.N)[:p.M]
    s3 = p.srcs[3]
    tab = torch.as_strided(p.xbuf, (50, s3.width), (s3.sr, 1), s3.off).double()
    want = conv + F.linear(tab[s3.rowidx.long()], p.w[0, :, 3 * Cc:].double(), p.bias[0].double())
    got = R.evaluate(p)
    _close(got["pre"][0], want, "conv1d + gather")
    _close(got["out"][0], F.leaky_relu(want, R.SLOPE), "lrelu epilogue")
    blocks = R.stats_blocks(got["out"][0], 64)
    assert blocks.shape == (2, 2, p.N)
    _close(blocks[1, 0], got["out"][0][64:].sum(0), "block sum")
    _close(blocks[0, 1], (got["out"][0][:64] ** 2).sum(0), "block sum of squares")


def test_reference_equals_lstm_cell():
    from video_gcp_amd import packing as pk
    torch.manual_seed(11)
    M, In, H = 21, 112, 160
    cell = torch.nn.LSTMCell(In, H).double()
    x, h, c = torch.randn(M, In), torch.randn(M, H), torch.randn(M, H + 8)
    with torch.no_grad():
        h1, c1 = cell(x.double(), (h.double(), c[:, :H].double()))
        w, b = pk.lstm_gate_interleave(cell.weight_ih, cell.weight_hh, cell.bias_ih, cell.bias_hh)
        pre = F.linear(x.double(), cell.weight_ih, cell.bias_ih) + F.linear(h.double(), cell.weight_hh, cell.bias_hh)
    srcs = [R.Src(0, 0, In, In), R.Src(M * In, 0, H, H)]
    p = R.Problem("cell", torch.cat([x.flatten(), h.flatten()]), srcs, M, 4 * H, In + H, M, w[None], b[None], epi=R.EPI_LSTM,
                  c_prev=c, c_prev_stride=H + 8)
    got = R.evaluate(p)                              # (w, b are float64 here: .to(float64) keeps them)
    _close(got["h"], h1, "h")
    _close(got["c"], c1, "c")
    i, f, g, o = pre.chunk(4, 1)                     # torch's gate-major order -> [M][H][4]
    _close(got["gates"], torch.stack([torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)], -1), "gates")


def test_batches_read_their_own_rows_weights_and_bias():
    p = R.batched_case(("W", 1, 2), 21, 160, 2)
    got = R.evaluate(p)["pre"]
    for z in range(2):
        xs = [torch.as_strided(p.xbuf, (3, p.rpb, s.width), (s.sb, s.sr, 1), s.off + z * p.z_src_off).reshape(21, s.width) for s in p.srcs]
        _close(got[z], F.linear(torch.cat(xs, 1).double(), p.w[z].double(), p.bias[z].double()), f"batch {z}")
    assert float((got[0] - got[1]).abs().min()) > 0


# ------------------------------------------------------------------------------------------------------------------------------
# 2. / 3. torch's float32 result against the bounds, intact and with a planted mistake
# ------------------------------------------------------------------------------------------------------------------------------
def _worst(p, got, ref, bnd):
    keys = ("gates", "c", "h") if p.epi == R.EPI_LSTM else ("out",)
    return max(float(((got[k].double() - ref[k]).abs() / bnd[k]).max()) for k in keys)


@pytest.mark.parametrize("p", CASES, ids=lambda p: p.name)
def test_float32_torch_stays_inside_the_bound_and_a_wrong_k_group_does_not(p):
    ref = R.evaluate(p)
    bnd = R.bounds(p, ref)
    assert all(bool(torch.isfinite(v).all()) and float(v.min()) > 0 for v in bnd.values())
    ratio = _worst(p, R.evaluate(p, torch.float32), ref, bnd)
    assert ratio <= 1.0, ratio
    if p.stats:
        for rows in (16, 32, 64):
            want, tol = R.stats_ref(p, ref, bnd, rows)
            got = R.stats_blocks(R.evaluate(p, torch.float32)["out"][0], rows)
            assert got.shape == want.shape and bool(((got.double() - want).abs() <= tol).all())
    # a k-group of the last source dropped (its weights zeroed) / counted twice (doubled), in float64: nothing but the mistake
    for factor in (0.0, 2.0):
        w = p.w.clone()
        w[:, :, p.K - 16:] *= factor
        bad = R.evaluate(dataclasses.replace(p, w=w))
        keys = ("gates", "c", "h") if p.epi == R.EPI_LSTM else ("out",)
        for k in keys:
            frac = float(((bad[k] - ref[k]).abs() > bnd[k]).double().mean())
            assert frac > 0.5, (k, factor, frac)


def test_bound_is_in_the_class_the_module_states():
    for form, kset, cap in ((("W", 1, 1), "k272", 5e-4), (("KS", 2, 4), "k1312", 3e-3)):
        p = R.tails_case(form, kset)
        b = R.bounds(p, R.evaluate(p))["out"]
        assert float(b.max()) < cap and float(b.median()) > (p.K + 8) * R.U * 0.3 * p.K ** 0.5


# ------------------------------------------------------------------------------------------------------------------------------
# 4. the dispatch query names the form each case is built for
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from video_gcp_amd import runtime as rt
    return rt, rt.load_library()


def _form(rt, lib, p):
    out6 = (C.c_int32 * 6)()
    rt.check(lib.gcpx_gemm_form(C.byref(R.gemm_args(rt, p, lambda name: 64, orow=p.N)), out6), "gemm_form")
    return list(out6)


@pytest.mark.parametrize("form", R.FORMS, ids=R.form_id)
def test_query_answers_the_form_of_every_case(lib, form, monkeypatch):
    rt, lib = lib
    for k, v in R.tile_env(form).items():
        monkeypatch.setenv(k, v)
    M, N = R.form_shape(form)
    for p in [R.tails_case(form, k) for k in R.K_SETS] + [R.sources_case(form), R.lstm_case(form)]:
        assert _form(rt, lib, p) == R.expected_form(form, M, N), p.name
    if form == ("KS", 1, 1):
        assert _form(rt, lib, R.stats_on_split_k_case()) == R.expected_form(form, M, N) and lib.gcpx_gemm_row_blocks(M, N) == 3
    if form[0] == "W":
        assert lib.gcpx_gemm_row_blocks(M, N) == 2
    for f, Mb, Nb, nb in R.batched_cases():
        if f == form:
            assert _form(rt, lib, R.batched_case(f, Mb, Nb, nb)) == R.expected_form(f, Mb, Nb, nb)


def test_query_rejects_what_gemm_rejects_and_sees_the_other_kernels(lib):
    rt, lib = lib
    out6 = (C.c_int32 * 6)()
    assert lib.gcpx_gemm_form(C.byref(rt.GemmArgs()), out6) == -1 and b"nsrc" in lib.gcpx_last_error()
    p = R.tails_case(("KS", 1, 1), "k272")
    a = R.gemm_args(rt, p, lambda name: 64, orow=p.N)
    assert lib.gcpx_gemm_form(C.byref(a), None) == -1
    a.K += 16
    assert lib.gcpx_gemm_form(C.byref(a), out6) == -1 and b"K != sum" in lib.gcpx_last_error()
    # 8192 rows with the f16 pieces of the weights: the split-f16 kernel; with a workspace as well: the planes form
    a = rt.GemmArgs()
    a.src[0].ptr, a.src[0].sr, a.src[0].width = 64, 256, 256
    a.nsrc, a.M, a.N, a.K, a.rpb, a.wpk, a.out, a.orow, a.wpk_split = 1, 8192, 1024, 256, 8192, 64, 64, 1024, 64
    rt.check(lib.gcpx_gemm_form(C.byref(a), out6), "gemm_form")
    assert list(out6) == [rt.GEMM_FORM_SPLIT_F16, 0, 0, 0, 0, 1]
    a.x_planes, a.x_exp, a.x_planes_bytes = 64, 64, 1 << 40
    rt.check(lib.gcpx_gemm_form(C.byref(a), out6), "gemm_form")
    assert list(out6) == [rt.GEMM_FORM_PLANES, 0, 0, 0, 0, 1]
