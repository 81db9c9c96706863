"""-m gpu: the one-launch form of the first two encoder blocks (csrc/conv_enc_fused.hip, gcpx_conv4x4s2_image_fused) against the two
launches it replaces — gcpx_conv4x4s2_image, then gcpx_conv4x4s2 with the same split-f16 pack — never against itself.

The fused kernel forms the 32 x 32 x 16 map with the first kernel's products in its order and runs the second kernel's steps on it, so
the comparison is for equal BITS (int32 views: a NaN or the sign of a zero counts), of the layer output and of the map where it is
stored.  The BatchNorm partial sums are held to float64 sums of the (bit-equal) output within the sequential-sum bound
2 n 2^-24 sum|v| that tests/test_gpu_lowres_tiled.py applies to its sums.  The model-level cases reuse the tolerances of
tests/test_gpu_model.py (_check_common) and tests/test_gpu_training.py (_compare_grads) against the oracle, computed once."""
import ctypes as C

import pytest
import torch

from helpers import make_inputs

pytestmark = pytest.mark.gpu

S, C0, C1 = 64, 16, 32


@pytest.fixture(scope="module")
def ctx():
    from video_gcp_amd import runtime as rt, packing as pk
    lib = rt.load_library()
    assert torch.cuda.is_available()
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(11)
    w0, b0 = torch.randn(C0, 3, 4, 4, generator=g) / 48 ** 0.5, torch.randn(C0, generator=g) * 0.1
    w1, b1 = torch.randn(C1, C0, 4, 4, generator=g) / 256 ** 0.5, torch.randn(C1, generator=g) * 0.1
    ws, e = pk.pack_conv4x4_split(w1)
    return dict(rt=rt, pk=pk, lib=lib, dev=dev, w0=pk.pack_conv4x4_image(w0).to(dev), b0=b0.to(dev), w1=pk.pack_conv4x4(w1).to(dev),
                b1=b1.to(dev), ws=ws.to(dev), e=e, G=lib.gcpx_conv4x4s2_image_fused_grid(), rows=lib.gcpx_conv4x4s2_grid())


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.contiguous().view(torch.int32)


def _frames(F, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(F, 3, S, S, generator=g) * 2 - 1


def _args(c, F, a0, out, st, split=True, Hin=S // 2, cout=C1):
    rt = c["rt"]
    a = rt.ConvArgs()
    s = a.src[0]
    s.ptr, s.C, s.frame_div, s.act = (a0.data_ptr() if a0 is not None else None), C0, 1, rt.ACT_NONE
    a.nsrc, a.Cin, a.F, a.Hin, a.Win, a.Hout, a.Wout, a.Cout, a.out_pitch = 1, C0, F, Hin, Hin, Hin // 2, Hin // 2, cout, cout
    a.wpk, a.bias, a.out = c["w1"].data_ptr(), c["b1"].data_ptr(), out.data_ptr()
    a.stats_partial = st.data_ptr() if st is not None else None
    if split:
        a.wpk_split, a.w_split_log2, a.split_layout = c["ws"].data_ptr(), c["e"], rt.SPLIT_PLAIN
    return a


def _buffers(c, F, stats):
    """one sentinel frame of NaN behind frame F - 1 of the map and of the output; every row of stats_partial NaN"""
    nan, dev = float("nan"), c["dev"]
    a0 = torch.full((F + 1, S // 2, S // 2, C0), nan, device=dev)
    out = torch.full((F + 1, S // 4, S // 4, C1), nan, device=dev)
    st = torch.full((c["rows"], 2, C1), nan, device=dev) if stats else None
    return a0, out, st


def _pair(c, xd, stats=True):
    """the reference: the two launches"""
    rt, lib, F = c["rt"], c["lib"], xd.shape[0]
    a0, out, st = _buffers(c, F, stats)
    rt.check(lib.gcpx_conv4x4s2_image(xd.data_ptr(), c["w0"].data_ptr(), c["b0"].data_ptr(), a0.data_ptr(), F, S, S, C0, rt.ACT_LRELU,
                                      _stream()), "image")
    a = _args(c, F, a0, out, st)
    rt.check(lib.gcpx_conv4x4s2(C.byref(a), _stream()), "conv4x4s2")
    torch.cuda.synchronize()
    return a0, out, st


def _fused(c, xd, store=True, stats=True):
    rt, lib, F = c["rt"], c["lib"], xd.shape[0]
    a0, out, st = _buffers(c, F, stats)
    a = _args(c, F, None, out, st)
    assert lib.gcpx_conv4x4s2_image_fused_supported(C.byref(a), S, S) == 1
    rt.check(lib.gcpx_conv4x4s2_image_fused(xd.data_ptr(), c["w0"].data_ptr(), c["b0"].data_ptr(), rt.ACT_LRELU,
                                            a0.data_ptr() if store else None, C.byref(a), _stream()), "fused")
    torch.cuda.synchronize()
    return a0, out, st


_cache = {}


def _case(c, which):
    """(x, reference pair, fused with the map stored) of a frame count, computed once and not modified by the tests"""
    if which not in _cache:
        F = {"one": 1, "three": 3, "wrap": c["G"] + 3}[which]
        xd = _frames(F, 100 + F).to(c["dev"])
        _cache[which] = (xd, _pair(c, xd), _fused(c, xd))
    return _cache[which]


@pytest.mark.parametrize("which", ["one", "three", "wrap"])
def test_frame_counts_bit_equal_and_sentinels(ctx, which):
    """F = 1, 3 and grid + 3 (a few workgroups loop twice, most once, and every workgroup's last frame has no next frame): output and
    stored map bit-equal to the two launches, the frame behind F - 1 of both untouched"""
    xd, (ra0, rout, _), (fa0, fout, _) = _case(ctx, which)
    F = xd.shape[0]
    assert bool(torch.isfinite(rout[:F]).all()) and bool(torch.isfinite(ra0[:F]).all())
    assert torch.equal(_bits(fout[:F]), _bits(rout[:F]))
    assert torch.equal(_bits(fa0[:F]), _bits(ra0[:F]))
    assert bool(torch.isnan(fout[F:]).all()) and bool(torch.isnan(fa0[F:]).all())
    assert bool(torch.isnan(rout[F:]).all()) and bool(torch.isnan(ra0[F:]).all())


@pytest.mark.parametrize("which", ["three", "wrap"])
def test_without_the_map_store_and_without_stats(ctx, which):
    """a0_out = NULL is accepted and nothing is written to the map; stats_partial = NULL runs; the layer output is in both cases
    bit-equal to the run with the store pointer and the sums"""
    xd, _, (_, fout, _) = _case(ctx, which)
    F = xd.shape[0]
    n0, nout, nst = _fused(ctx, xd, store=False)
    assert bool(torch.isnan(n0).all())
    assert torch.equal(_bits(nout), _bits(fout))
    assert bool(torch.isfinite(nst).all())
    for store in (False, True):
        s0, sout, sst = _fused(ctx, xd, store=store, stats=False)
        assert sst is None and torch.equal(_bits(sout), _bits(fout))
        assert bool(torch.isnan(s0[F:]).all()) and bool(torch.isnan(s0).all()) == (not store)


def test_frame_content_zero_large_small(ctx):
    """frames that are all zero (the amax = 0 branch: the map is LeakyReLU(bias), and with a zero bias exactly zero), scaled by 1e3 and
    by 1e-3 next to ordinary ones in one launch: the scale is per frame, every frame bit-equal"""
    x = _frames(7, 5)
    x[1] = 0
    x[2] *= 1e3
    x[3] *= 1e-3
    x[5] = 0
    xd = x.to(ctx["dev"])
    ra0, rout, rst = _pair(ctx, xd)
    fa0, fout, fst = _fused(ctx, xd)
    assert torch.equal(_bits(fout), _bits(rout)) and torch.equal(_bits(fa0), _bits(ra0))
    # amax = 0 proper: a zero first-layer bias makes the map of a zero frame exactly zero
    c0 = dict(ctx, b0=torch.zeros_like(ctx["b0"]))
    ra0, rout, _ = _pair(c0, xd)
    fa0, fout, _ = _fused(c0, xd)
    assert bool((ra0[1] == 0).all()) and bool((ra0[5] == 0).all())
    assert torch.equal(_bits(fout), _bits(rout)) and torch.equal(_bits(fa0), _bits(ra0))
    assert torch.equal(fout[1], ctx["b1"].expand_as(fout[1]))


@pytest.mark.parametrize("which", ["one", "three", "wrap"])
def test_stats_partial_rows_and_sums(ctx, which):
    """every row of stats_partial is written and the rows without a frame are zero; the column sums in float64 against float64 sums of
    the launch's own output within 2 n 2^-24 sum|v| (n values per channel); row f holds frame f alone, as in the two launches whose
    one-frame workgroups write the same rows: compared bit for bit"""
    xd, (_, _, rst), (_, fout, fst) = _case(ctx, which)
    F = xd.shape[0]
    assert F <= ctx["rows"] and bool(torch.isfinite(fst).all())
    assert bool((fst[F:] == 0).all()) and bool((fst[:F, 1] > 0).all())
    v = fout[:F].reshape(-1, C1).double().cpu()
    n = v.shape[0]
    got = fst.double().sum(0).cpu()
    for k, t in ((0, v), (1, v * v)):
        want, bound = t.sum(0), 2 * n * 2.0 ** -24 * t.abs().sum(0)
        e = (got[k] - want).abs()
        print(f"F = {F}: sum v^{k + 1}: worst error / bound = {float((e / bound).max()):.3e}")
        assert bool((e <= bound).all()), (k, float((e / bound).max()))
    same = torch.equal(_bits(fst), _bits(rst))
    print(f"F = {F}: stats_partial rows bit-equal to the two launches: {same}")
    assert same


def test_supported_answers(ctx):
    """0 for a 32 x 32 image, for Cout other than 32, for absent split weights, for a layout other than PLAIN, for more frames than
    stats_partial has rows; 1 for the encoder's problem.  The launch itself refuses what the query refuses, before any HIP call"""
    rt, lib = ctx["rt"], ctx["lib"]
    _, out, st = _buffers(ctx, 3, True)
    q = lambda a, s=S: lib.gcpx_conv4x4s2_image_fused_supported(C.byref(a), s, s)
    assert q(_args(ctx, 3, None, out, st)) == 1
    assert q(_args(ctx, 3, None, out, None)) == 1
    assert q(_args(ctx, 3, None, out, st, Hin=16), 32) == 0
    assert q(_args(ctx, 3, None, out, st), 32) == 0
    assert q(_args(ctx, 3, None, out, st, cout=64)) == 0
    assert q(_args(ctx, 3, None, out, st, split=False)) == 0
    a = _args(ctx, 3, None, out, st)
    a.split_layout = rt.SPLIT_ROWFOLD
    assert q(a) == 0
    assert q(_args(ctx, ctx["rows"] + 1, None, out, st)) == 0
    bad = _args(ctx, 3, None, out, st, split=False)
    assert lib.gcpx_conv4x4s2_image_fused(out.data_ptr(), ctx["w0"].data_ptr(), ctx["b0"].data_ptr(), rt.ACT_LRELU, None, C.byref(bad),
                                          _stream()) == -1
    assert ctx["G"] >= 1 and ctx["G"] + 3 <= ctx["rows"]


def _op_names(model):
    return [op[0] for p in model._plans.values() for op in p.ops]


def test_plan_keeps_two_launches_for_32x32_images():
    """img_sz = 32: the query answers 0 and the encoder plans hold gcpx_conv4x4s2_image + gcpx_conv4x4s2 as before"""
    from test_gpu_model import _build
    hp, sd, model = _build("c1", img_sz=32, batch_size=2)
    model.train(True)
    inputs, noise, _ = make_inputs(hp, seed=3, variant="B")
    model({k: v.cuda() for k, v in inputs.items()}, "train", noise=noise.cuda())
    torch.cuda.synchronize()
    names = _op_names(model)
    assert not [n for n in names if n.startswith("enc.input+")]
    for tag in ("traj", "I0", "Ig"):
        assert f"enc.input:{tag}" in names and f"enc.pyramid-0:{tag}" in names


def _detach(o):
    if torch.is_tensor(o):
        return o.detach()
    if isinstance(o, dict):
        return {k: _detach(v) for k, v in o.items()}
    if isinstance(o, (list, tuple)):
        return type(o)(_detach(v) for v in o)
    return o


@pytest.fixture(scope="module")
def c2_oracle():
    """c2 with two sequences: the oracle's training-mode forward, losses and autograd gradients, once"""
    import video_gcp_amd as V
    from oracle import gcp_model_oracle as O
    hp = V.config("c2", batch_size=2)
    sd = V.init_params(hp, seed=1, randomize_affine=True)
    inputs, noise, _ = make_inputs(hp, seed=5, variant="B")
    taps = {}
    gref, res, total, ref = O.gradients(sd, hp, inputs, noise, taps=taps)
    return dict(hp=hp, sd=sd, inputs=inputs, noise=noise, gref=_detach(gref), total=float(total.detach()), ref=_detach(ref),
                enc_traj=taps["enc_traj_seq"].detach())


def _forward(o, monkeypatch, fuse):
    """fuse: "none" = GCPX_NO_ENC_FUSE=1, "default" = the plan's own choice per pass, "all" = GCPX_ENC_FUSE_ALL=1"""
    from video_gcp_amd.model import GCPTreeModel
    monkeypatch.delenv("GCPX_NO_ENC_FUSE", raising=False)
    monkeypatch.delenv("GCPX_ENC_FUSE_ALL", raising=False)
    if fuse == "none":
        monkeypatch.setenv("GCPX_NO_ENC_FUSE", "1")
    elif fuse == "all":
        monkeypatch.setenv("GCPX_ENC_FUSE_ALL", "1")
    model = GCPTreeModel(o["hp"], params=o["sd"], device="cuda", materialize_distr=True)
    model.train(True)
    dev_in = {k: v.cuda() for k, v in o["inputs"].items()}
    out = model(dev_in, "train", noise=o["noise"].cuda())
    total = float(model.get_total_loss(dev_in, model.loss(dev_in, out)).value)
    torch.cuda.synchronize()
    return model, out, total


def test_model_c2_fused_and_two_launches_against_the_oracle(c2_oracle, monkeypatch):
    """training-mode forward with losses: with GCPX_NO_ENC_FUSE=1, as planned by default (trajectory and I_g passes fused, the I_0 pass
    two launches) and with GCPX_ENC_FUSE_ALL=1 (the I_0 pass fused too, its map stored for the decoder's skip 0): each within the
    tolerances of tests/test_gpu_model.py against the oracle (_check_common; the total loss within that file's 2e-5 relative + 1e-6),
    and the fused runs' difference from the two-launch run in enc_traj and in the total loss no larger than that run's own distance to
    the oracle.  A fused pass holds one launch in place of two, and no map buffer where the map has no reader"""
    from test_gpu_model import _check_common
    o = c2_oracle
    hp, ref = o["hp"], o["ref"]
    res = {}
    for fuse in ("none", "default", "all"):
        model, out, total = _forward(o, monkeypatch, fuse)
        names = _op_names(model)
        plan = [p for p in model._plans.values() if "enc:traj" in p.rec][0]
        for tag in ("traj", "I0", "Ig"):
            one = fuse == "all" or (fuse == "default" and tag != "I0")
            assert (f"enc.input+pyramid-0:{tag}" in names) == one
            assert (f"enc.input:{tag}" in names) == (not one) and (f"enc.pyramid-0:{tag}" in names) == (not one)
            assert (plan.rec[f"enc:{tag}"]["a0"] is None) == (one and tag != "I0")
        _check_common(hp, model, out, ref, posterior=True)
        assert abs(total - o["total"]) <= 2e-5 * abs(o["total"]) + 1e-6, (fuse, total, o["total"])
        res[fuse] = (out.raw["enc_traj_seq"].detach().cpu().reshape(o["enc_traj"].shape).clone(), total)
    own_enc = float((res["none"][0] - o["enc_traj"]).abs().max())
    own_tot = abs(res["none"][1] - o["total"])
    for fuse in ("default", "all"):
        d_enc = float((res[fuse][0] - res["none"][0]).abs().max())
        d_tot = abs(res[fuse][1] - res["none"][1])
        print(f"{fuse}: enc_traj: vs two launches {d_enc:.3e}, two launches vs oracle {own_enc:.3e}; total loss: {d_tot:.3e}, {own_tot:.3e}")
        assert d_enc <= own_enc and d_tot <= own_tot


def test_trainer_step_c2_gradients_reach_the_first_layer(c2_oracle, monkeypatch):
    """GCPTrainStep on the fused plan: its backward reads the stored map for the first two layers' gradients; every parameter gradient
    within the tolerance of tests/test_gpu_training.py against the oracle's autograd gradients"""
    from test_gpu_training import _compare_grads
    from video_gcp_amd.model import GCPTreeModel
    from video_gcp_amd.training import GCPTrainStep
    o = c2_oracle
    monkeypatch.delenv("GCPX_NO_ENC_FUSE", raising=False)
    monkeypatch.setenv("GCPX_ENC_FUSE_ALL", "1")           # all three passes through the fused launch with the map stored
    model = GCPTreeModel(o["hp"], params=o["sd"], device="cuda")
    model.use_graph = False
    tr = GCPTrainStep(model, lr=1e-3)
    out = tr.backward({k: v.cuda() for k, v in o["inputs"].items()}, o["noise"].cuda())
    torch.cuda.synchronize()
    names = _op_names(model)
    assert all(f"enc.input+pyramid-0:{tag}" in names for tag in ("traj", "I0", "Ig"))
    plan = [p for p in model._plans.values() if "enc:traj" in p.rec][0]
    assert all(plan.rec[f"enc:{tag}"]["a0"] is not None for tag in ("traj", "I0", "Ig"))
    assert abs(float(out.raw["losses"][5]) - o["total"]) <= 2e-5 * abs(o["total"])
    got = tr.named_grads()
    _compare_grads(o["gref"], got)
    for k in ("encoder.net.input.conv.weight", "encoder.net.pyramid-0.conv.weight"):
        assert float(got[k].abs().max()) > 0, k
