"""conv3x3_up16_fold16_kernel (GCPX_SPLIT_ROWFOLD16): the 16 + 16 -> 16 channel upsampling block with its skip half convolved once per
sequence (one launch over the sequences' frames, zero bias) and added, as a register-resident addend tile, by the per-node launch that
walks a sequence's nodes back to back.  Shapes: the smallest at which the node-inner item order, the run change inside a wavefront's
range and the two-stage patch ring can go wrong."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

from helpers import assert_close

pytestmark = pytest.mark.gpu

#         Hin, frames, nodes per sequence
CASES = [(8, 6, 3),         # one column block, two row blocks: top and bottom corrections in neighbouring items; more wavefronts than items
         (32, 74, 37),      # ranges of 2 items against an odd run length: a wavefront crosses a run boundary mid-range and reloads ab
         (32, 127, 127)]    # one sequence at the workload's run length
IDS = [f"Hin{h}-F{f}-N{n}" for h, f, n in CASES]


def _stream():
    return torch.cuda.current_stream().cuda_stream


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


@functools.lru_cache(maxsize=None)
def _run(Hin, Fr, nodes):
    """Every launch of one case, once: the one-launch 32-channel row-folded block, the skip half, the node half + addend (twice, for the
    determinism check), and the CPU references.  The tests below only read the result."""
    from video_gcp_amd import runtime as rt, packing as pk
    lib, dev = rt.load_library(), torch.device("cuda")
    torch.manual_seed(Hin + nodes)
    cp = cs = cout = 16
    x = torch.randn(Fr, cp, Hin, Hin)
    sc, sh = torch.rand(cp) + 0.5, torch.randn(cp) * 0.2
    sk = torch.randn(Fr // nodes, cs, Hin, Hin)
    ssc, ssh = torch.rand(cs) + 0.5, torch.randn(cs) * 0.2
    xin = F.leaky_relu(x * sc[None, :, None, None] + sh[None, :, None, None], 0.2)
    skin = F.leaky_relu(sk * ssc[None, :, None, None] + ssh[None, :, None, None], 0.2)
    w, b = torch.randn(cout, cp + cs, 3, 3) / (9 * 32) ** 0.5, torch.randn(cout) * 0.1
    want = F.conv2d(F.interpolate(torch.cat([xin, skin.repeat_interleave(nodes, 0)], 1), scale_factor=2, mode="bilinear", align_corners=False),
                    w, b, padding=1)
    want_skip64 = F.conv2d(F.interpolate(skin.double(), scale_factor=2, mode="bilinear", align_corners=False), w[:, cp:].double(), None, padding=1)
    xd, skd = x.permute(0, 2, 3, 1).contiguous().to(dev), sk.permute(0, 2, 3, 1).contiguous().to(dev)
    wp, bd = pk.pack_conv3x3(w, 16).to(dev), pk.pad_vec(b, cout).to(dev)
    scd, shd, sscd, sshd = sc.to(dev), sh.to(dev), ssc.to(dev), ssh.to(dev)
    H2 = 2 * Hin
    r = dict(want=want, want_skip64=want_skip64, Fr=Fr, H2=H2, cout=cout)
    # the 32-channel row-folded kernel, one launch over both sources
    wf, ef = pk.pack_conv3x3_fold(w)
    wf = wf.to(dev)
    out1 = torch.full((Fr, H2, H2, cout), float("nan"), device=dev)
    a1 = _conv_args(rt, [(xd, cp, 1, scd, shd, rt.ACT_LRELU), (skd, cs, nodes, sscd, sshd, rt.ACT_LRELU)],
                    F=Fr, Hin=Hin, Win=Hin, Hout=H2, Wout=H2, Cout=cout, out_pitch=cout, upsample=1, head_mode=rt.HEAD_RAW, wpk=wp, bias=bd,
                    out=out1, stats_partial=out1)
    a1.wpk_split, a1.w_split_log2, a1.split_layout = wf.data_ptr(), ef, rt.SPLIT_ROWFOLD
    G = lib.gcpx_conv3x3_grid(C.byref(a1))
    assert G > 0
    st1 = torch.full((G, 2, cout), float("nan"), device=dev)
    a1.stats_partial = st1.data_ptr()
    rt.check(lib.gcpx_conv3x3(C.byref(a1), _stream()), "32-channel row-folded block, one launch")
    # the skip half once per sequence (no addend, zero bias) ...
    wa, ea = pk.pack_conv3x3_fold16(w, 0)
    wb, eb = pk.pack_conv3x3_fold16(w, 16)
    wa, wb = wa.to(dev), wb.to(dev)
    add = torch.full((Fr // nodes, H2, H2, cout), float("nan"), device=dev)
    a_s = _conv_args(rt, [(skd, cs, 1, sscd, sshd, rt.ACT_LRELU)], F=Fr // nodes, Hin=Hin, Win=Hin, Hout=H2, Wout=H2, Cout=cout,
                     out_pitch=cout, upsample=1, head_mode=rt.HEAD_RAW, wpk=wp, bias=torch.zeros(cout, device=dev), out=add)
    a_s.wpk_split, a_s.w_split_log2, a_s.split_layout = wb.data_ptr(), eb, rt.SPLIT_ROWFOLD16
    rt.check(lib.gcpx_conv3x3(C.byref(a_s), _stream()), "skip half")
    # ... and the node half with the addend, twice
    outs, sts = [], []
    for rep in range(2):
        out2 = torch.full((Fr, H2, H2, cout), float("nan"), device=dev)
        a2 = _conv_args(rt, [(xd, cp, 1, scd, shd, rt.ACT_LRELU)], F=Fr, Hin=Hin, Win=Hin, Hout=H2, Wout=H2, Cout=cout,
                        out_pitch=cout, upsample=1, head_mode=rt.HEAD_RAW, wpk=wp, bias=bd, out=out2, stats_partial=out2)
        a2.wpk_split, a2.w_split_log2, a2.split_layout = wa.data_ptr(), ea, rt.SPLIT_ROWFOLD16
        a2.addend, a2.addend_frame_div = add.data_ptr(), nodes
        r["G2"] = lib.gcpx_conv3x3_grid(C.byref(a2))
        st2 = torch.full((G, 2, cout), float("nan"), device=dev)
        a2.stats_partial = st2.data_ptr()
        rt.check(lib.gcpx_conv3x3(C.byref(a2), _stream()), "node half + addend")
        outs.append(out2)
        sts.append(st2)
    # refused, not dropped: the one-launch fold layout and the exact-f32 path with a 16-channel addend
    a1.addend, a1.addend_frame_div = add.data_ptr(), nodes
    r["refused_fold"] = lib.gcpx_conv3x3(C.byref(a1), _stream())
    a1.wpk_split = None
    r["refused_exact"] = lib.gcpx_conv3x3(C.byref(a1), _stream())
    torch.cuda.synchronize()
    r.update(G=G, out1=out1.cpu(), st1=st1.cpu(), add=add.cpu(), out2=outs[0].cpu(), st2=sts[0].cpu(), out2b=outs[1].cpu(), st2b=sts[1].cpu(),
             items=Fr * (Hin // 4) * (H2 // 16))
    return r


def _ratio(got, want, atol, rtol):
    return float(((got - want).abs() / (atol + rtol * want.abs())).max())


@pytest.mark.parametrize("Hin,Fr,nodes", CASES, ids=IDS)
def test_fold16_hoisted_equals_the_one_launch_block(Hin, Fr, nodes):
    """hoisted form against conv3x3_up16_fold_kernel over the concatenated channels (atol 4e-6, rtol 1e-5); the same grid, so the plan's
    stats_partial rows fit both; a wavefront of the two large cases walks at least two items"""
    r = _run(Hin, Fr, nodes)
    assert r["G2"] == r["G"]
    ipw = -(-r["items"] // (r["G"] * 8))
    print(f"items {r['items']}, workgroups {r['G']}, items per wavefront {ipw}")
    if Hin == 32:
        assert ipw >= 2, (r["items"], r["G"])
    print(f"hoisted vs one launch: worst error / bound = {_ratio(r['out2'], r['out1'], 4e-6, 1e-5):.3f}")
    assert_close(r["out2"], r["out1"], atol=4e-6, rtol=1e-5, name="hoisted vs the 32-channel row-folded launch")


@pytest.mark.parametrize("Hin,Fr,nodes", CASES, ids=IDS)
def test_fold16_hoisted_equals_conv2d(Hin, Fr, nodes):
    r = _run(Hin, Fr, nodes)
    got = r["out2"].permute(0, 3, 1, 2)
    print(f"hoisted vs F.conv2d: worst error / bound = {_ratio(got, r['want'], 2e-5, 1e-5):.3f}")
    assert_close(got, r["want"], atol=2e-5, rtol=1e-5, name="16-channel row-folded block, skip hoisted, vs F.conv2d")


@pytest.mark.parametrize("Hin,Fr,nodes", CASES, ids=IDS)
def test_fold16_batchnorm_partial_sums_vs_float64(Hin, Fr, nodes):
    """rows of stats_partial summed = the float64 column sums of the launch's OWN output, within the sequential-sum bound
    2 n 2^-24 sum|v| (n elements per channel; sum v^2 likewise with v^2), which no tiled summation order exceeds"""
    r = _run(Hin, Fr, nodes)
    v = r["out2"].double().reshape(-1, r["cout"])
    n = v.shape[0]
    got = r["st2"].double().sum(0)
    for which, t in ((0, v), (1, v * v)):
        want, bound = t.sum(0), 2 * n * 2.0 ** -24 * t.abs().sum(0)
        err = (got[which] - want).abs()
        print(f"sum v^{which + 1}: worst error / bound = {float((err / bound).max()):.3e}")
        assert bool((err <= bound).all()), (which, float((err / bound).max()))


@pytest.mark.parametrize("Hin,Fr,nodes", CASES, ids=IDS)
def test_fold16_skip_launch_alone_vs_float64(Hin, Fr, nodes):
    """addend = NULL, div = 1: ab is the (zero) bias and the item order is (frame, column block, row block).  Tolerance: that of the whole
    block against F.conv2d (atol 2e-5, rtol 1e-5) — the skip half's products are a subset of the block's, every one of them carries the
    same split-f16 and f32-accumulation error terms, and its reference here is float64, which adds none"""
    r = _run(Hin, Fr, nodes)
    got = r["add"].permute(0, 3, 1, 2).double()
    print(f"skip launch vs float64: worst error / bound = {_ratio(got, r['want_skip64'], 2e-5, 1e-5):.3f}")
    assert_close(got, r["want_skip64"], atol=2e-5, rtol=1e-5, name="skip half alone vs float64 conv2d")


@pytest.mark.parametrize("Hin,Fr,nodes", CASES, ids=IDS)
def test_fold16_is_deterministic_and_other_paths_refuse_the_addend(Hin, Fr, nodes):
    r = _run(Hin, Fr, nodes)
    assert torch.equal(r["out2"], r["out2b"]) and torch.equal(r["st2"], r["st2b"])
    assert not torch.isnan(r["out2"]).any() and not torch.isnan(r["st2"]).any()
    assert r["refused_fold"] != 0, "GCPX_SPLIT_ROWFOLD took a 16-channel addend"
    assert r["refused_exact"] != 0, "the exact-f32 path took an addend"
