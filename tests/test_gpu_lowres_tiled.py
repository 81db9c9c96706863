"""conv3x3_lowres_kernel with register-tiled interpolation stages (csrc/conv3x3_lowres.hip): what tests/test_gpu_lowres_up.py cannot
reach.  There the frame counts (6, 5, 1) are below the grid, so no workgroup ever does a second unit; here the persistent loop wraps
(the output of unit n is stored behind the staging of unit n + 1, the addend of unit n is requested before the input of unit n + 1),
one-hot pixels sit on the seams of the half-runs, and the addend changes magnitude by 1e3 from one sequence to the next.

Tile sizes as built: both stages split a row (column) of 2 Hin outputs into two half-runs of Hin outputs; the first reads source
samples 0 .. Hin / 2, the mirrored second reads Hin / 2 - 1 .. Hin - 1.  The seam is between source samples Hin / 2 - 1 and Hin / 2
(3 | 4 at Hin = 8, 1 | 2 at Hin = 4), both of which feed both half-runs."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

from test_gpu_lowres_up import SHAPES, SHAPE_IDS, _block_args, _env, _stream

pytestmark = pytest.mark.gpu

#             Hin, cin, cout, addend_frame_div (0: no addend)
WRAP_CASES = [(8, 64, 32, 0), (8, 64, 32, 3), (4, 128, 64, 0)]
WRAP_IDS = ["Hin8-64-32", "Hin8-64-32-addend3", "Hin4-128-64"]
GUARD = 2          # frames behind frame F - 1 of the output buffer that must stay untouched


@functools.lru_cache(maxsize=None)
def _run_wrapped(Hin, cin, cout, div):
    """F = 2 G + 3 frames at 8x8 (one frame per unit), 4 G + 5 at 4x4 (two per unit), G = gcpx_conv3x3_grid: two full rounds of the
    persistent loop and a partial one, and at 4x4 an odd frame count, so that the last unit repeats a frame that must not be stored.
    One launch of the exact f32 kernel (no statistics, no addend: it takes none) and one of the low-res kernel with statistics."""
    rt, pk, lib, dev = _env()
    torch.manual_seed(23)
    H2 = 2 * Hin
    x0 = torch.randn(1, cin, Hin, Hin)
    xd0 = x0.permute(0, 2, 3, 1).contiguous().to(dev)
    sc, sh = torch.rand(cin) + 0.5, torch.randn(cin) * 0.2
    w, b = torch.randn(cout, cin, 3, 3) / (9 * cin) ** 0.5, torch.randn(cout) * 0.1
    wp, bd = pk.pack_conv3x3(w, 32).to(dev), pk.pad_vec(b, cout).to(dev)
    ws, e = pk.pack_conv3x3_split32(w)
    ws = ws.to(dev)
    probe = _block_args(rt, [(xd0, cin, 1, sc.to(dev), sh.to(dev), rt.ACT_LRELU)], 1, Hin, cout, wp, bd, xd0, stats_partial=xd0)
    probe.wpk_split, probe.w_split_log2, probe.split_layout = ws.data_ptr(), e, rt.SPLIT_LOWRES
    G = lib.gcpx_conv3x3_grid(C.byref(probe))
    assert G > 0
    Fr = 2 * G + 3 if Hin == 8 else 4 * G + 5
    x = torch.randn(Fr, cin, Hin, Hin)
    xd = x.permute(0, 2, 3, 1).contiguous().to(dev)
    src = [(xd, cin, 1, sc.to(dev), sh.to(dev), rt.ACT_LRELU)]
    ref = pk.lowres_up_reference(F.leaky_relu(x * sc[None, :, None, None] + sh[None, :, None, None], 0.2), w, b)
    out32 = torch.full((Fr, H2, H2, cout), float("nan"), device=dev)
    a32 = _block_args(rt, src, Fr, Hin, cout, wp, bd, out32)
    rt.check(lib.gcpx_conv3x3(C.byref(a32), _stream()), "exact f32")
    out = torch.full((Fr + GUARD, H2, H2, cout), float("nan"), device=dev)
    st = torch.full((G, 2, cout), float("nan"), device=dev)
    a = _block_args(rt, src, Fr, Hin, cout, wp, bd, out, stats_partial=st)
    a.wpk_split, a.w_split_log2, a.split_layout = ws.data_ptr(), e, rt.SPLIT_LOWRES
    add = None
    if div:
        add = torch.randn((Fr + div - 1) // div, cout, H2, H2)
        addd = add.permute(0, 2, 3, 1).contiguous().to(dev)
        a.addend, a.addend_frame_div = addd.data_ptr(), div
        a._keep_add = addd
    assert lib.gcpx_conv3x3_lowres_supported(C.byref(a)) == 1
    assert lib.gcpx_conv3x3_grid(C.byref(a)) == G
    rt.check(lib.gcpx_conv3x3(C.byref(a), _stream()), "lowres, wrapped")
    torch.cuda.synchronize()
    got = out.cpu()
    want = ref if add is None else ref + add.double().repeat_interleave(div, 0)[:Fr]
    return dict(Fr=Fr, G=G, cout=cout, got=got[:Fr].permute(0, 3, 1, 2).double(), guard=got[Fr:], want=want,
                err32=(out32.cpu().permute(0, 3, 1, 2).double() - ref).abs(), scale=float(ref.abs().max()), st=st.cpu())


@pytest.mark.parametrize("Hin,cin,cout,div", WRAP_CASES, ids=WRAP_IDS)
def test_wrapped_units_error_vs_float64(Hin, cin, cout, div):
    """every output element against packing.lowres_up_reference (+ the addend), under the bounds of test_lowres_error_vs_float64: rms
    error <= 1.5 x, max error <= 2 x the exact f32 kernel's on the same input (its conv alone: the f32 kernel takes no addend; the
    one extra f32 addition lies inside the max bound's 4e-7 of scale)"""
    r = _run_wrapped(Hin, cin, cout, div)
    assert torch.isfinite(r["got"]).all()
    err = (r["got"] - r["want"]).abs()
    rms, rms32 = float(err.pow(2).mean().sqrt()), float(r["err32"].pow(2).mean().sqrt())
    mx, mx32 = float(err.max()), float(r["err32"].max())
    scale = r["scale"] if not div else float(r["want"].abs().max())
    print(f"F {r['Fr']} G {r['G']}: rms lowres {rms:.3e} f32 {rms32:.3e} | max lowres {mx:.3e} f32 {mx32:.3e} | scale {scale:.3e}")
    assert rms <= 1.5 * rms32 + 1e-12 * scale
    assert mx <= 2.0 * mx32 + 4e-7 * scale


@pytest.mark.parametrize("Hin,cin,cout,div", WRAP_CASES, ids=WRAP_IDS)
def test_wrapped_units_batchnorm_sums_and_guard(Hin, cin, cout, div):
    """rows of stats_partial summed = the float64 column sums of the launch's own output within the sequential-sum bound
    2 n 2^-24 sum|v| of test_lowres_batchnorm_partial_sums_vs_float64 (the repeated frame of an odd count is not counted); the
    frames behind F - 1 of the output buffer are untouched"""
    r = _run_wrapped(Hin, cin, cout, div)
    v = r["got"].permute(0, 2, 3, 1).reshape(-1, r["cout"])
    n = v.shape[0]
    assert torch.isfinite(r["st"]).all()
    got = r["st"].double().sum(0)
    for which, t in ((0, v), (1, v * v)):
        want, bound = t.sum(0), 2 * n * 2.0 ** -24 * t.abs().sum(0)
        e = (got[which] - want).abs()
        print(f"sum v^{which + 1}: worst error / bound = {float((e / bound).max()):.3e}")
        assert bool((e <= bound).all()), (which, float((e / bound).max()))
    assert r["guard"].numel() > 0 and bool(torch.isnan(r["guard"]).all())


def _seam_positions(Hin):
    m, l = Hin // 2, Hin - 1
    pos = [(m - 1, m - 1), (m - 1, m), (m, m - 1), (m, m), (0, m - 1), (0, m), (m - 1, l), (m, l),       # the seam of rows and of columns
           (0, 0), (0, l), (l, 0), (l, l),                                                             # corners
           (1, 1), (1, l - 1), (l - 1, 1), (l - 1, l - 1), (1, m), (l - 1, m - 1), (m, 1), (m - 1, l - 1)]   # one in from each border
    return list(dict.fromkeys(pos))


@pytest.mark.parametrize("Hin,c_prev,c_skip,cout", SHAPES, ids=SHAPE_IDS)
def test_tile_seams_exact(Hin, c_prev, c_skip, cout):
    """one frame per position (row, column) of a one-hot input pixel, one-hot taps (tap = output channel % 9: all nine in every
    frame), no affine, bias a multiple of 1/16, as in test_lowres_borders_exact: every step is exact in f32 and the result must EQUAL
    the float64 reference.  Positions, with m = Hin / 2 and l = Hin - 1 (half-runs read samples 0 .. m and m - 1 .. l): the last sample
    of the first half-run and the first of the second, (m - 1 | m), in rows and in columns, alone, together and on a border; the four
    corners; one in from each border.  At Hin = 8: rows / columns 3 | 4, 0, 7, 1, 6; at Hin = 4: 1 | 2, 0, 3."""
    rt, pk, lib, dev = _env()
    cin = c_prev + c_skip
    pos = _seam_positions(Hin)
    Fr = len(pos)
    x = torch.zeros(Fr, cin, Hin, Hin)
    for f, (y, xx) in enumerate(pos):
        x[f, (f * 37 + 5) % cin, y, xx] = 1.0
    w = torch.zeros(cout, cin, 3, 3)
    for co in range(cout):
        w[co, :, (co % 9) // 3, (co % 9) % 3] = 1.0
    b = torch.arange(cout, dtype=torch.float32) / 16 - 1
    ref = pk.lowres_up_reference(x, w, b)
    assert torch.equal(ref * 16, (ref * 16).round())
    xd = x.permute(0, 2, 3, 1).contiguous().to(dev)
    srcs = [(xd[..., :c_prev].contiguous(), c_prev, 1, None, None, rt.ACT_NONE)]
    if c_skip:
        srcs.append((xd[..., c_prev:].contiguous(), c_skip, 1, None, None, rt.ACT_NONE))
    wp, bd = pk.pack_conv3x3(w, 32).to(dev), pk.pad_vec(b, cout).to(dev)
    ws, e = pk.pack_conv3x3_split32(w)
    ws = ws.to(dev)
    out = torch.full((Fr, 2 * Hin, 2 * Hin, cout), float("nan"), device=dev)
    a = _block_args(rt, srcs, Fr, Hin, cout, wp, bd, out)
    a.wpk_split, a.w_split_log2, a.split_layout = ws.data_ptr(), e, rt.SPLIT_LOWRES
    assert lib.gcpx_conv3x3_lowres_supported(C.byref(a)) == 1
    rt.check(lib.gcpx_conv3x3(C.byref(a), _stream()), "lowres, one-hot on the seams")
    torch.cuda.synchronize()
    got = out.cpu().permute(0, 3, 1, 2).double()
    bad = (got != ref).flatten(1).any(1).nonzero().flatten().tolist()
    assert torch.equal(got, ref), (float((got - ref).abs().max()), [pos[f] for f in bad])


def test_addend_across_a_sequence_boundary():
    """F = 2 div + 1 = 7, div = 3: frames 0-2, 3-5 and 6 add the addend frames 0, 1, 2, of magnitude 1, 1e3 and 1e-3.  Bound per element,
    from the number formats: the conv's own error <= 2e-5 (the bound test_lowres_hoisted_pair... uses for this kernel against float64
    at unit scale) + three f32 roundings (bias + addend, + conv, and the addend's own) of at most 2^-24 (|conv + bias| + |addend|) each.
    A stale, early or missing addend tile is off by ~1e3, ~1 or ~1e-3 on almost every element."""
    rt, pk, lib, dev = _env()
    torch.manual_seed(29)
    Hin, cin, cout, div = 8, 64, 32, 3
    Fr, H2 = 2 * div + 1, 16
    x = torch.randn(Fr, cin, Hin, Hin)
    sc, sh = torch.rand(cin) + 0.5, torch.randn(cin) * 0.2
    w, b = torch.randn(cout, cin, 3, 3) / (9 * cin) ** 0.5, torch.randn(cout) * 0.1
    add = torch.randn(3, cout, H2, H2) * torch.tensor([1.0, 1e3, 1e-3])[:, None, None, None]
    conv = pk.lowres_up_reference(F.leaky_relu(x * sc[None, :, None, None] + sh[None, :, None, None], 0.2), w, b)
    addf = add.double().repeat_interleave(div, 0)[:Fr]
    want = conv + addf
    tol = 2e-5 + 3 * 2.0 ** -24 * (conv.abs() + addf.abs())
    xd, addd = x.permute(0, 2, 3, 1).contiguous().to(dev), add.permute(0, 2, 3, 1).contiguous().to(dev)
    wp, bd = pk.pack_conv3x3(w, 32).to(dev), pk.pad_vec(b, cout).to(dev)
    ws, e = pk.pack_conv3x3_split32(w)
    ws = ws.to(dev)
    out = torch.full((Fr, H2, H2, cout), float("nan"), device=dev)
    a = _block_args(rt, [(xd, cin, 1, sc.to(dev), sh.to(dev), rt.ACT_LRELU)], Fr, Hin, cout, wp, bd, out)
    a.wpk_split, a.w_split_log2, a.split_layout = ws.data_ptr(), e, rt.SPLIT_LOWRES
    a.addend, a.addend_frame_div = addd.data_ptr(), div
    assert lib.gcpx_conv3x3_lowres_supported(C.byref(a)) == 1
    rt.check(lib.gcpx_conv3x3(C.byref(a), _stream()), "lowres, addend of three magnitudes")
    torch.cuda.synchronize()
    got = out.cpu().permute(0, 3, 1, 2).double()
    assert torch.isfinite(got).all()
    err = (got - want).abs()
    for f in range(Fr):
        print(f"frame {f} (addend frame {f // div}): worst error / bound = {float((err[f] / tol[f]).max()):.3e}")
    assert bool((err <= tol).all()), float((err / tol).max())
