"""conv3x3_lowres_kernel (GCPX_SPLIT_LOWRES, csrc/conv3x3_lowres.hip): the 32 / 64-output-channel upsampling blocks with the nine tap
products taken on the source grid and the bilinear x2 + 3x3 shift-sum behind them.  One frame per unit of work, one workgroup per CU:
the frame counts here (5, 6, 1) are below the grid, so most workgroups do no work, and the shapes cover every kernel instance
(CT, Hin, chunks) = (4, 4, 4), (2, 8, 2), (2, 8, 4), (2, 4, 4)."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

from helpers import assert_close

pytestmark = pytest.mark.gpu

#          Hin, c_prev, c_skip, cout
SHAPES = [(4, 128, 0, 64), (8, 64, 0, 32), (8, 64, 64, 32), (4, 64, 64, 32)]
SHAPE_IDS = [f"Hin{h}-{cp}+{cs}-{co}" for h, cp, cs, co in SHAPES]
CASES = ["unit", "chunk_scales", "outlier", "zero_chunk"]
FRAMES = [(6, 3), (5, 5), (1, 1)]          # (frames, nodes per sequence = frame_div of the skip source)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _env():
    from video_gcp_amd import runtime as rt, packing as pk
    return rt, pk, rt.load_library(), torch.device("cuda")


def _conv_args(rt, srcs, **kw):
    a = rt.ConvArgs()
    a._keep = (srcs, kw)          # device tensors must outlive the launch (the struct only holds raw pointers)
    cin = 0
    for i, (t, Cc, fdiv, sc, sh, act) in enumerate(srcs):
        s = a.src[i]
        s.ptr, s.C, s.frame_div, s.act = t.data_ptr(), Cc, fdiv, act
        s.scale = sc.data_ptr() if sc is not None else None
        s.shift = sh.data_ptr() if sh is not None else None
        cin += Cc
    a.nsrc, a.Cin = len(srcs), cin
    for k, v in kw.items():
        setattr(a, k, v.data_ptr() if hasattr(v, "data_ptr") else v)
    return a


def _block_args(rt, srcs, Fr, Hin, cout, wp, bd, out, **kw):
    return _conv_args(rt, srcs, F=Fr, Hin=Hin, Win=Hin, Hout=2 * Hin, Wout=2 * Hin, Cout=cout, out_pitch=cout, upsample=1,
                      head_mode=rt.HEAD_RAW, wpk=wp, bias=bd, out=out, **kw)


@pytest.mark.parametrize("Fr,nodes", FRAMES, ids=[f"F{f}" for f, _ in FRAMES])
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("Hin,c_prev,c_skip,cout", SHAPES, ids=SHAPE_IDS)
def test_lowres_error_vs_float64(case, Hin, c_prev, c_skip, cout, Fr, nodes):
    """against float64, next to the exact f32 kernel, with the cases and bounds of test_conv3x3_up32_split_error_vs_float64: the
    32-channel chunks differ in magnitude by 1e4 either way, carry an outlier, or are all zero"""
    rt, pk, lib, dev = _env()
    torch.manual_seed(7)
    cin = c_prev + c_skip
    amp_a, amp_b = {"unit": (1, 1), "chunk_scales": (1e-2, 1e2), "outlier": (1, 1), "zero_chunk": (0, 1)}[case]
    for order in (0, 1):
        a_lo, a_hi = (amp_a, amp_b) if order == 0 else (amp_b, amp_a)
        camp = torch.where(torch.arange(cin) < cin // 2, torch.tensor(float(a_lo)), torch.tensor(float(a_hi)))
        x = torch.randn(Fr, c_prev, Hin, Hin) * camp[None, :c_prev, None, None]
        if case == "outlier":
            x[min(2, Fr - 1), 7, 1, 2] = 2e4
        sc, sh = torch.rand(c_prev) + 0.5, torch.randn(c_prev) * 0.2 * camp[:c_prev]
        srcs_ref = [F.leaky_relu(x * sc[None, :, None, None] + sh[None, :, None, None], 0.2)]
        xd = x.permute(0, 2, 3, 1).contiguous().to(dev)
        srcs = [(xd, c_prev, 1, sc.to(dev), sh.to(dev), rt.ACT_LRELU)]
        if c_skip:
            sk = torch.randn(Fr // nodes, c_skip, Hin, Hin) * camp[None, c_prev:, None, None]
            srcs_ref.append(sk.repeat_interleave(nodes, 0))
            srcs.append((sk.permute(0, 2, 3, 1).contiguous().to(dev), c_skip, nodes, None, None, rt.ACT_NONE))
        w, b = torch.randn(cout, cin, 3, 3) / (9 * cin) ** 0.5, torch.randn(cout) * 0.1
        up = F.interpolate(torch.cat(srcs_ref, 1).double(), scale_factor=2, mode="bilinear", align_corners=False)
        ref = F.conv2d(up, w.double(), b.double(), padding=1)
        wp, bd = pk.pack_conv3x3(w, 32).to(dev), pk.pad_vec(b, cout).to(dev)
        ws, e = pk.pack_conv3x3_split32(w)
        ws = ws.to(dev)
        err = {}
        for name in ("f32", "lowres"):
            out = torch.full((Fr, 2 * Hin, 2 * Hin, cout), float("nan"), device=dev)
            a = _block_args(rt, srcs, Fr, Hin, cout, wp, bd, out)
            if name == "lowres":
                a.wpk_split, a.w_split_log2, a.split_layout = ws.data_ptr(), e, rt.SPLIT_LOWRES
                assert lib.gcpx_conv3x3_lowres_supported(C.byref(a)) == 1
            rt.check(lib.gcpx_conv3x3(C.byref(a), _stream()), name)
            torch.cuda.synchronize()
            got = out.cpu().permute(0, 3, 1, 2).double()
            assert torch.isfinite(got).all()
            err[name] = (got - ref).abs()
        scale = float(ref.abs().max())
        rms = {k: float(v.pow(2).mean().sqrt()) for k, v in err.items()}
        mx = {k: float(v.max()) for k, v in err.items()}
        print(f"order {order}: rms lowres {rms['lowres']:.3e} f32 {rms['f32']:.3e} | max lowres {mx['lowres']:.3e} f32 {mx['f32']:.3e} | scale {scale:.3e}")
        assert rms["lowres"] <= 1.5 * rms["f32"] + 1e-12 * scale
        assert mx["lowres"] <= 2.0 * mx["f32"] + 4e-7 * scale


@functools.lru_cache(maxsize=None)
def _run_hoisted():
    """(8, 64, 64, 32), F = 6, three nodes per sequence: the one-launch PLAIN kernel over both sources; the LOWRES skip launch (two
    sequence frames, zero bias, the pack's skip offset) and the LOWRES node launch with the addend, twice, with statistics."""
    rt, pk, lib, dev = _env()
    torch.manual_seed(11)
    Hin, cp, cs, cout, Fr, nodes = 8, 64, 64, 32, 6, 3
    x, sk = torch.randn(Fr, cp, Hin, Hin), torch.randn(Fr // nodes, cs, Hin, Hin)
    sc, sh, ssc, ssh = torch.rand(cp) + 0.5, torch.randn(cp) * 0.2, torch.rand(cs) + 0.5, torch.randn(cs) * 0.2
    w, b = torch.randn(cout, cp + cs, 3, 3) / (9 * (cp + cs)) ** 0.5, torch.randn(cout) * 0.1
    xd, skd = x.permute(0, 2, 3, 1).contiguous().to(dev), sk.permute(0, 2, 3, 1).contiguous().to(dev)
    s_node, s_skip = (xd, cp, 1, sc.to(dev), sh.to(dev), rt.ACT_LRELU), (skd, cs, 1, ssc.to(dev), ssh.to(dev), rt.ACT_LRELU)
    wp, bd = pk.pack_conv3x3(w, 32).to(dev), pk.pad_vec(b, cout).to(dev)
    ws, e = pk.pack_conv3x3_split32(w)
    ws = ws.to(dev)
    H2 = 2 * Hin
    out1 = torch.full((Fr, H2, H2, cout), float("nan"), device=dev)
    a1 = _block_args(rt, [s_node, s_skip[:2] + (nodes,) + s_skip[3:]], Fr, Hin, cout, wp, bd, out1)
    a1.wpk_split, a1.w_split_log2, a1.split_layout = ws.data_ptr(), e, rt.SPLIT_PLAIN
    rt.check(lib.gcpx_conv3x3(C.byref(a1), _stream()), "PLAIN, one launch")
    add = torch.full((Fr // nodes, H2, H2, cout), float("nan"), device=dev)
    a_s = _block_args(rt, [s_skip], Fr // nodes, Hin, cout, wp, torch.zeros(cout, device=dev), add)
    # the skip channels' k-steps follow the node channels' in the pack: [chunk][tap][CT][2][64] x 16 B
    a_s.wpk_split, a_s.w_split_log2, a_s.split_layout = ws.data_ptr() + (cp // 32) * 9 * (cout // 16) * 2048, e, rt.SPLIT_LOWRES
    sup = lib.gcpx_conv3x3_lowres_supported(C.byref(a_s))
    rt.check(lib.gcpx_conv3x3(C.byref(a_s), _stream()), "LOWRES skip half")
    outs, sts = [], []
    for rep in range(2):
        out2 = torch.full((Fr, H2, H2, cout), float("nan"), device=dev)
        a2 = _block_args(rt, [s_node], Fr, Hin, cout, wp, bd, out2, stats_partial=out2)
        a2.wpk_split, a2.w_split_log2, a2.split_layout = ws.data_ptr(), e, rt.SPLIT_LOWRES
        a2.addend, a2.addend_frame_div = add.data_ptr(), nodes
        sup = sup and lib.gcpx_conv3x3_lowres_supported(C.byref(a2))
        G = lib.gcpx_conv3x3_grid(C.byref(a2))
        assert G > 0
        st = torch.full((G, 2, cout), float("nan"), device=dev)
        a2.stats_partial = st.data_ptr()
        rt.check(lib.gcpx_conv3x3(C.byref(a2), _stream()), "LOWRES node half + addend")
        outs.append(out2)
        sts.append(st)
    a1.split_layout, a1.stats_partial = rt.SPLIT_PLAIN, out1.data_ptr()
    G1 = lib.gcpx_conv3x3_grid(C.byref(a1))
    torch.cuda.synchronize()
    xin = F.leaky_relu(sk * ssc[None, :, None, None] + ssh[None, :, None, None], 0.2)
    return dict(out1=out1.cpu(), add=add.cpu(), out2=outs[0].cpu(), out2b=outs[1].cpu(), st=sts[0].cpu(), stb=sts[1].cpu(), G=G, G1=G1, sup=sup,
                Fr=Fr, cout=cout, want_skip64=pk.lowres_up_reference(xin, w[:, cp:], None))


def test_lowres_hoisted_pair_equals_the_one_launch_plain_block():
    """skip launch + node launch with addend (F = 6, addend_frame_div = 3) against conv3x3_up32_split_kernel over the concatenated
    channels, within the tolerances of tests/test_gpu_fold16_hoist.py (atol 4e-6, rtol 1e-5); the statistics rows of both forms agree"""
    r = _run_hoisted()
    assert r["sup"] and r["G"] == r["G1"]
    worst = float(((r["out2"] - r["out1"]).abs() / (4e-6 + 1e-5 * r["out1"].abs())).max())
    print(f"hoisted LOWRES pair vs one PLAIN launch: worst error / bound = {worst:.3f}")
    assert_close(r["out2"], r["out1"], atol=4e-6, rtol=1e-5, name="hoisted LOWRES pair vs the PLAIN launch")
    assert_close(r["add"].permute(0, 3, 1, 2).double(), r["want_skip64"], atol=2e-5, rtol=1e-5, name="skip half alone vs float64")


def test_lowres_batchnorm_partial_sums_vs_float64():
    """rows of stats_partial summed = the float64 column sums of the launch's OWN output, within the sequential-sum bound
    2 n 2^-24 sum|v| (tests/test_gpu_fold16_hoist.py); one frame per workgroup: the rows behind the first F did no work and are zero"""
    r = _run_hoisted()
    v = r["out2"].double().reshape(-1, r["cout"])
    n = v.shape[0]
    assert torch.isfinite(r["st"]).all()
    got = r["st"].double().sum(0)
    for which, t in ((0, v), (1, v * v)):
        want, bound = t.sum(0), 2 * n * 2.0 ** -24 * t.abs().sum(0)
        err = (got[which] - want).abs()
        print(f"sum v^{which + 1}: worst error / bound = {float((err / bound).max()):.3e}")
        assert bool((err <= bound).all()), (which, float((err / bound).max()))
    assert r["G"] > r["Fr"] and bool((r["st"][r["Fr"]:] == 0).all())
    assert bool((r["st"][:r["Fr"], 1] > 0).all())


def test_lowres_is_deterministic():
    r = _run_hoisted()
    assert torch.equal(r["out2"], r["out2b"]) and torch.equal(r["st"], r["stb"])
    assert not torch.isnan(r["out2"]).any()


@pytest.mark.parametrize("Hin,cin,cout", [(4, 128, 64), (8, 64, 32)], ids=["Hin4-128-64", "Hin8-64-32"])
def test_lowres_borders_exact(Hin, cin, cout):
    """one frame per position of a one-hot input pixel — the four corners, the four edges, the interior — and a one-hot tap per output
    channel (tap = channel % 9), no affine, bias a multiple of 1/16: every product of bilinear weights is a multiple of 1/16, so every
    step is exact in f32 and the result must EQUAL the float64 reference"""
    rt, pk, lib, dev = _env()
    m, l = Hin // 2, Hin - 1
    pos = [(0, 0), (0, l), (l, 0), (l, l), (0, m), (l, m), (m, 0), (m, l), (m, m - 1)]
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
    wp, bd = pk.pack_conv3x3(w, 32).to(dev), pk.pad_vec(b, cout).to(dev)
    ws, e = pk.pack_conv3x3_split32(w)
    ws = ws.to(dev)
    out = torch.full((Fr, 2 * Hin, 2 * Hin, cout), float("nan"), device=dev)
    a = _block_args(rt, [(xd, cin, 1, None, None, rt.ACT_NONE)], Fr, Hin, cout, wp, bd, out)
    a.wpk_split, a.w_split_log2, a.split_layout = ws.data_ptr(), e, rt.SPLIT_LOWRES
    rt.check(lib.gcpx_conv3x3(C.byref(a), _stream()), "lowres, one-hot")
    torch.cuda.synchronize()
    got = out.cpu().permute(0, 3, 1, 2).double()
    assert torch.equal(got, ref), float((got - ref).abs().max())


def test_lowres_supported_query():
    rt, pk, lib, dev = _env()
    buf = torch.zeros(16, device=dev)

    def args(Hin, c_prev, c_skip, cout, upsample=1, layout=rt.SPLIT_LOWRES, split=True):
        srcs = [(buf, c_prev, 1, None, None, rt.ACT_NONE)] + ([(buf, c_skip, 3, None, None, rt.ACT_NONE)] if c_skip else [])
        Ho = 2 * Hin if upsample else Hin
        a = _conv_args(rt, srcs, F=6, Hin=Hin, Win=Hin, Hout=Ho, Wout=Ho, Cout=cout, out_pitch=cout, upsample=upsample,
                       head_mode=rt.HEAD_RAW, wpk=buf, bias=buf, out=buf)
        if split:
            a.wpk_split, a.w_split_log2, a.split_layout = buf.data_ptr(), 0, layout
        return a

    for Hin, cp, cs, cout in SHAPES:
        assert lib.gcpx_conv3x3_lowres_supported(C.byref(args(Hin, cp, cs, cout))) == 1, (Hin, cp, cs, cout)
        assert lib.gcpx_conv3x3_lowres_supported(C.byref(args(Hin, cp, cs, cout, layout=rt.SPLIT_PLAIN))) == 1       # the same pack
    assert lib.gcpx_conv3x3_lowres_supported(C.byref(args(8, 64, 0, 32, upsample=0))) == 0
    assert lib.gcpx_conv3x3_lowres_supported(C.byref(args(16, 16, 0, 16))) == 0
    assert lib.gcpx_conv3x3_lowres_supported(C.byref(args(16, 32, 0, 16))) == 0
    for layout in (rt.SPLIT_ROWFOLD, rt.SPLIT_ROWFOLD16, rt.SPLIT_HEAD32):
        assert lib.gcpx_conv3x3_lowres_supported(C.byref(args(8, 64, 0, 32, layout=layout))) == 0
    assert lib.gcpx_conv3x3_lowres_supported(C.byref(args(8, 64, 0, 32, split=False))) == 0
    # GCPX_SPLIT_LOWRES on a block the query refuses is an error, not a fall-back
    a = args(4, 64, 0, 32)
    assert lib.gcpx_conv3x3_lowres_supported(C.byref(a)) == 0
    assert lib.gcpx_conv3x3(C.byref(a), _stream()) != 0
