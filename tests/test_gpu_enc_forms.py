"""-m gpu: every device body behind gcpx_conv4x4s2 and gcpx_conv4x4s2_image (csrc/conv_enc.hip, csrc/conv_enc_split.hip), at every
frames-per-block choice that changes what a workgroup does, against the float64 reference of tests/enc_refs.py within the rounding
bounds derived there (pinned without a GPU by tests/test_enc_refs_cpu.py).

Fifteen bodies: three direct conv4x4s2_kernel, five conv4x4s2_lds_kernel, five conv4x4s2_split_kernel, conv4x4s2_image_kernel<1>,
conv4x4s2_image_lds_kernel<32> / <64>.  Every test first asks gcpx_conv4x4s2_form / gcpx_conv4x4s2_image_form what the entry point
launches for its arguments and asserts form, frames per block, grid and block count — forms are forced through GCPX_ENC_FPB,
GCPX_ENC_DIRECT, GCPX_ENC_NOSPLIT and GCPX_ENC_IMAGE_DIRECT, which the entry points read on every call; a mismatch fails, nothing
skips.  The launch then writes into NaN-filled `out` and `stats_partial` buffers with a guard frame (a guard row) of NaN behind the last
one, and reads an input with a NaN frame behind frame F - 1: the guards must still be NaN, everything inside finite, every one of the
gcpx_conv4x4s2_grid() statistics rows written and the rows of workgroups without work exactly zero.  Each test prints its worst
error / bound; the worst over its cases on an MI355X stands in its docstring.

The derived split-f16 bound is a ceiling that one-piece f16 arithmetic would pass at K >= 512 (tests/test_enc_refs_cpu.py shows it),
so every test of a split body also launches the LDS body on the same case at the same frames per block and asserts, frame by frame,
the project's criterion for split-f16 kernels: max error <= 2 x the exact body's + 4e-7 scale, rms error <= 1.5 x the exact body's +
1e-12 scale, scale = the frame's largest |reference| (enc_refs.split_vs_exact).  That is what holds "f32-equivalent", and what holds
the small frame of the scale cases to its own magnitude.

  staged    the five LDS and five split bodies x frames per block (enc_refs.STAGED_FPB) x F = 2 fpb + 1 and 2 fpb - 1: a last block
            with one frame and one missing a frame; 32 -> 64 @8 with fpb 2 and 5 leaves LDS wavefronts without a pixel group and with
            unequal counts.  Each with an affine + LeakyReLU source and raw output, and a plain source with LeakyReLU output.
  scale     a block that begins with a frame 1000 times smaller than its others (the block's single scale must come from all frames and
            keep the small frame's bits), an all-zero block, a last block of one frame; split and, beside it, LDS.
  direct    the three direct bodies forced on shapes that have an LDS form, and on the shapes that reach them on their own: non-square
            frames, 4 x 4 and 8 x 8 frames whose last pixel group and last workgroup are partly valid; with statistics (grid not
            clamped: workgroups without a block write zero rows) and without.
  image     both image forms; the direct one on 6 x 10 (masked lanes), 16 x 48, 128 x 128; where both forms exist they must agree bit
            for bit, as the kernel's comment promises.
  wrap      the persistent loops: F = grid + 3 (grid from the query, asked with more frames than any grid has workgroups) for the LDS and split bodies at 32 -> 64 @8 and the image LDS body
            at 64, statistics included; the direct body at 16 -> 32 @64 with more than grid x 256 output pixels (134 MB of input, a fifth
            of a second), held to float64 on the frames around the wrap and on the first and last frame, finite everywhere else.

The bounds are worst-case bounds of f32 (and two-piece f16) roundoff, so ratios far below 1 are what a right kernel gives; a dropped
k-step or an un-zeroed border tap is 1e2 - 1e5 bounds.  No test here found a wrong result.

Planted arithmetic errors, one at a time in scratch builds of the library (numbers only, no address or loop bound; nothing of it is
committed), and the tests of this file that fail with each (85 tests in all):
  * `fetch` of conv4x4s2_lds_kernel returns the loaded value for an invalid tap in the !ZP branch: the three tests that run the one
    body without a zero pixel, 16 -> 32 @32 — staged[LDS-16-32-32-fpb1-F3 / -F1] and scale[16-32-32-fpb1] (its LDS half).  All other
    LDS bodies are ZP and do not contain the line.
  * the LDS kernel's last ping-pong step's `mm` skipped: all 28 staged[LDS-*], all five scale[*] (LDS half) and
    staged_persistent_loop[LDS]: every test that launches an LDS body.
  * the split kernel's block maximum taken over the block's first frame only: the 18 staged[SPLIT-*] with fpb > 1 and the four scale[*]
    with fpb > 1 (outputs not finite: a later, larger frame overflows f16 under the first frame's scale).  With fpb = 1 the first frame
    IS the block: staged[SPLIT-*-fpb1-*], scale[16-32-32-fpb1] and staged_persistent_loop[SPLIT] pass, rightly.  Frames of three
    magnitudes in turn (enc_refs.FRAME_AMP) and a scale case whose block BEGINS with its smallest frame are there for this fault: with
    frames of one magnitude the first frame's maximum has the block's exponent more often than not and the fault went unseen.
  * the split kernel's x2 w1 MFMA (second piece of the activations) left out: all 34 tests that launch a split body, through the
    criterion against the LDS body at 1e2 - 4e2 of it; of the derived ceiling alone it reaches 1.14 at most (the wrap case) and would
    have passed nearly everywhere.
  * `msk` forced to 1 in conv4x4s2_kernel (the load address stays clamped): all 14 direct_bodies[*] and direct_persistent_loop.
  * the `pv[pt]` test removed from conv4x4s2_image_kernel's `xok` only: NO test fails, and none can.  The lanes the test masks are the
    columns of the 16 x 16 output tile behind the last pixel; the kernel never stores them (`if (!pv[pt]) continue`), a column of an
    MFMA's B operand reaches that column of the result alone, and without the test these lanes load pixel 0 of the image, inside the
    buffer.  What image_bodies[direct-6x10] holds of the masked group is that its 13 stored pixels are right and that nothing is
    written behind them.
  * in its place for the image family, a border tap of conv4x4s2_image_kernel reading element 0 of the image instead of the
    out-of-range offset that returns zero: all six image_bodies[*] (those for the LDS form through the bit comparison with the direct
    form) at 3e4 - 5e5 bounds; image_lds_persistent_loop does not launch the direct kernel and passes."""
import ctypes as C

import pytest
import torch

import enc_refs as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    from video_gcp_amd import runtime as rt, packing as pk
    lib = rt.load_library()
    assert torch.cuda.is_available()
    return rt, pk, lib, torch.device("cuda")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _nhwc_guarded(x, dev):
    """[F][C][H][W] -> device NHWC [F + 1][H][W][C] whose last frame is NaN"""
    Fr, c, H, W = x.shape
    buf = torch.full((Fr + 1, H, W, c), R.NAN)
    buf[:Fr] = x.permute(0, 2, 3, 1)
    return buf.to(dev)


def _layer_args(env, c, xd, out, stats, split):
    rt, pk, lib, dev = env
    Fr, cin, Hin, Win = c.x.shape
    cout = c.w.shape[0]
    a = rt.ConvArgs()
    keep = [xd, out, stats, pk.pack_conv4x4(c.w).to(dev), c.bias.to(dev)]
    s = a.src[0]
    s.ptr, s.C, s.frame_div, s.act = xd.data_ptr(), cin, 1, c.act
    if c.scale is not None:
        keep += [c.scale.to(dev), c.shift.to(dev)]
        s.scale, s.shift = keep[-2].data_ptr(), keep[-1].data_ptr()
    a.nsrc, a.Cin, a.F, a.Hin, a.Win, a.Hout, a.Wout, a.Cout, a.out_pitch = 1, cin, Fr, Hin, Win, Hin // 2, Win // 2, cout, cout
    a.wpk, a.bias, a.out, a.out_act = keep[3].data_ptr(), keep[4].data_ptr(), out.data_ptr(), c.out_act
    if stats is not None:
        a.stats_partial = stats.data_ptr()
    if split:
        ws, e = pk.pack_conv4x4_split(c.w)
        keep.append(ws.to(dev))
        a.wpk_split, a.w_split_log2, a.split_layout = keep[-1].data_ptr(), e, rt.SPLIT_PLAIN
    a._keep = keep                      # device tensors must outlive the launch (the struct only holds raw pointers)
    return a


def _check_guarded(name, buf, n):
    """buf[:n] finite, buf[n:] still NaN"""
    assert bool(torch.isnan(buf[n:]).all()), f"{name}: written behind its last frame / row"
    bad = int((~torch.isfinite(buf[:n])).sum())
    assert bad == 0, f"{name}: {bad} elements not finite"


def _run_layer(env, monkeypatch, c, form, fpb=0, stats=True, ref_frames=None):
    """gcpx_conv4x4s2 on Case c as `form`: asserts the query's answer, launches, checks guards and statistics rows and compares with
    float64 (ref_frames: only these frames are compared, the others must be finite).  Returns the worst error / bound per output, the
    compared outputs and their reference."""
    rt, pk, lib, dev = env
    for k, v in R.form_env(form, fpb).items():
        monkeypatch.setenv(k, v)
    Fr, cin, Hin, Win = c.x.shape
    cout, Ho, Wo = c.w.shape[0], Hin // 2, Win // 2
    G = lib.gcpx_conv4x4s2_grid()
    xd = _nhwc_guarded(c.x, dev)
    out = torch.full((Fr + 1, Ho, Wo, cout), R.NAN, device=dev)
    st = torch.full((G + 1, 2, cout), R.NAN, device=dev) if stats else None
    a = _layer_args(env, c, xd, out, st, form == R.SPLIT)
    out4 = (C.c_int32 * 4)()
    rt.check(lib.gcpx_conv4x4s2_form(C.byref(a), out4), "conv4x4s2_form")
    want = R.expected_form(form, Fr, Ho, Wo, cout, fpb, G, stats)
    assert list(out4) == want, f"{c.name}: gcpx_conv4x4s2 would run {list(out4)} (form, fpb, grid, nblk), the test is for {want}"
    rt.check(lib.gcpx_conv4x4s2(C.byref(a), _stream()), c.name)
    torch.cuda.synchronize()
    out = out.cpu()
    _check_guarded(f"{c.name}: out", out, Fr)
    got = {"out": out[:Fr].permute(0, 3, 1, 2).double()}
    if ref_frames is not None:
        idx = torch.tensor(ref_frames)
        c = R.Case(c.name, c.x[idx], c.w, c.bias, c.scale, c.shift, c.act, c.out_act)
        got["out"] = got["out"][idx]
    if stats:
        st = st.cpu()
        _check_guarded(f"{c.name}: stats_partial", st, G)
        busy = min(out4[2], out4[3])
        assert bool((st[busy:G] == 0).all()), f"{c.name}: statistics rows of workgroups without work are not zero"
        got["s1"], got["s2"] = st[:G, 0].double().sum(0), st[:G, 1].double().sum(0)
    ref = R.evaluate(c)
    r = R.ratios(got, ref, R.bounds(c, ref, "split" if form == R.SPLIT else "f32", max(fpb, 1)))
    print(f"{c.name} [{R.FORM_NAMES[form]} fpb {fpb}]: worst err / bound " + " ".join(f"{k} {v:.3g}" for k, v in r.items()))
    for k, v in r.items():
        assert v <= 1.0, f"{c.name}: {k} worst err / bound {v:.3g}"
    return r, got["out"], ref["out"]


def _run_split_beside_exact(env, monkeypatch, c, fpb):
    """the split body and the LDS body on the same case at the same fpb, each within its derived bound; then the split body's error
    frame by frame within the project's criterion against the LDS body's (enc_refs.split_vs_exact)"""
    _, got_s, ref = _run_layer(env, monkeypatch, c, R.SPLIT, fpb)
    _, got_e, _ = _run_layer(env, monkeypatch, c, R.LDS, fpb)
    r = R.split_vs_exact(got_s, got_e, ref)
    print(f"{c.name} [fpb {fpb}]: split against exact, worst frame: max {r['max']:.3g} rms {r['rms']:.3g}")
    assert r["max"] <= 1.0 and r["rms"] <= 1.0, f"{c.name}: split error against the exact body's, worst frame: max {r['max']:.3g} rms {r['rms']:.3g}"


def _probe_grid(env, monkeypatch, form, cin, cout, Hin, fpb=0):
    """the grid gcpx_conv4x4s2_form reports for more frames than any grid has workgroups (the query reads no memory: any address does)"""
    rt, pk, lib, dev = env
    for k, v in R.form_env(form, fpb).items():
        monkeypatch.setenv(k, v)
    Fr = 1 << 16
    a = rt.ConvArgs()
    a.nsrc, a.Cin, a.F, a.Hin, a.Win, a.Hout, a.Wout, a.Cout, a.out_pitch = 1, cin, Fr, Hin, Hin, Hin // 2, Hin // 2, cout, cout
    a.src[0].ptr, a.src[0].C, a.src[0].frame_div = 64, cin, 1
    a.wpk = a.bias = a.out = 64
    if form == R.SPLIT:
        a.wpk_split, a.split_layout = 64, rt.SPLIT_PLAIN
    out4 = (C.c_int32 * 4)()
    rt.check(lib.gcpx_conv4x4s2_form(C.byref(a), out4), "conv4x4s2_form")
    assert out4[0] == form and out4[2] < out4[3], f"probe: {list(out4)}"
    return out4[2]


def _run_image(env, monkeypatch, c, form):
    """gcpx_conv4x4s2_image on Case c as `form`; returns the worst error / bound and the device result (NHWC, F frames)"""
    rt, pk, lib, dev = env
    monkeypatch.delenv("GCPX_ENC_IMAGE_DIRECT", raising=False)
    for k, v in R.form_env(form).items():
        monkeypatch.setenv(k, v)
    Fr, _, Hin, Win = c.x.shape
    out2 = (C.c_int32 * 2)()
    rt.check(lib.gcpx_conv4x4s2_image_form(Fr, Hin, Win, out2), "conv4x4s2_image_form")
    assert out2[0] == form and 1 <= out2[1], f"{c.name}: gcpx_conv4x4s2_image would run form {out2[0]}, the test is for {form}"
    xd = torch.cat([c.x, torch.full((1,) + tuple(c.x.shape[1:]), R.NAN)]).to(dev)
    out = torch.full((Fr + 1, Hin // 2, Win // 2, 16), R.NAN, device=dev)
    wp, bd = pk.pack_conv4x4_image(c.w).to(dev), c.bias.to(dev)
    rt.check(lib.gcpx_conv4x4s2_image(xd.data_ptr(), wp.data_ptr(), bd.data_ptr(), out.data_ptr(), Fr, Hin, Win, 16, c.out_act, _stream()),
             c.name)
    torch.cuda.synchronize()
    out = out.cpu()
    _check_guarded(f"{c.name}: out", out, Fr)
    ref = R.evaluate(c)
    r = R.ratios({"out": out[:Fr].permute(0, 3, 1, 2).double()}, ref, R.bounds(c, ref))
    print(f"{c.name} [{R.FORM_NAMES[form]} grid {out2[1]}]: worst err / bound {r['out']:.3g}")
    assert r["out"] <= 1.0, f"{c.name}: worst err / bound {r['out']:.3g}"
    return r, out[:Fr], out2[1]


def _staged_id(p):
    form, (cin, cout, Hin), fpb, Fr = p
    return f"{R.FORM_NAMES[form]}-{cin}-{cout}-{Hin}-fpb{fpb}-F{Fr}"


@pytest.mark.parametrize("form,shape,fpb,Fr", R.staged_cases(), ids=[_staged_id(p) for p in R.staged_cases()])
def test_enc_staged_bodies_by_frames_per_block(env, monkeypatch, form, shape, fpb, Fr):
    """The five LDS and five split bodies at each frames-per-block value, last block with one frame / missing one, both input variants,
    statistics on.  worst error / bound on an MI355X (out, sum, sum of squares): LDS 0.020, 0.00095, 0.0024; split 0.0048, 0.00020, 0.00061;
    split against the LDS body (1.0 = the criterion), worst frame: max 0.54, rms 0.49."""
    cin, cout, Hin = shape
    for c in R.variants(f"{cin}-{cout}-{Hin}-F{Fr}", cin, cout, Hin, Hin, Fr, seed=fpb):
        if form == R.SPLIT:
            _run_split_beside_exact(env, monkeypatch, c, fpb)
        else:
            _run_layer(env, monkeypatch, c, form, fpb)


@pytest.mark.parametrize("shape,fpb", R.SPLIT_SCALE, ids=[f"{s[0]}-{s[1]}-{s[2]}-fpb{f}" for s, f in R.SPLIT_SCALE])
def test_enc_split_block_scale(env, monkeypatch, shape, fpb):
    """Split bodies: a frame 1000 times smaller than its block's largest, an all-zero block, a one-frame last block; the LDS body on the
    same case beside it.  worst error / bound on an MI355X (out, sum, sum of squares): split 0.0039, 0.00009, 0.00018; LDS 0.016, 0.00038, 0.00055;
    split against the LDS body, worst frame: max 0.37, rms 0.45."""
    c = R.split_scale_case(shape, fpb)
    _run_split_beside_exact(env, monkeypatch, c, fpb)


@pytest.mark.parametrize("stats", [True, False], ids=["stats", "nostats"])
@pytest.mark.parametrize("name,cin,cout,Hin,Win,Fr,forced", R.DIRECT_CASES, ids=[c[0] for c in R.DIRECT_CASES])
def test_enc_direct_bodies(env, monkeypatch, name, cin, cout, Hin, Win, Fr, forced, stats):
    """conv4x4s2_kernel<1,8,2,2>, <4,2,1,4>, <8,2,1,4>: forced on LDS shapes and on the shapes that fall to them, partly valid last
    groups and workgroups, both input variants.  worst error / bound on an MI355X: out 0.018, sum 0.0011, sum of squares 0.0041."""
    for c in R.variants(name, cin, cout, Hin, Win, Fr):
        _run_layer(env, monkeypatch, c, R.DIRECT, stats=stats)


@pytest.mark.parametrize("name,form,Hin,Win,Fr", R.IMAGE_CASES, ids=[c[0] for c in R.IMAGE_CASES])
def test_enc_image_bodies(env, monkeypatch, name, form, Hin, Win, Fr):
    """conv4x4s2_image_kernel<1> and conv4x4s2_image_lds_kernel<32> / <64>, raw and LeakyReLU output; at 32 and 64 the other form must
    give the same bits.  worst error / bound on an MI355X: direct 0.083 (128 x 128), LDS 0.064."""
    for out_act in (R.ACT_NONE, R.ACT_LRELU):
        c = R.image_case(name, Hin, Win, Fr, out_act)
        _, out, _ = _run_image(env, monkeypatch, c, form)
        if Hin == Win and Hin in (32, 64):
            other = R.IMAGE_DIRECT if form == R.IMAGE_LDS else R.IMAGE_LDS
            _, out_o, _ = _run_image(env, monkeypatch, c, other)
            assert torch.equal(out, out_o), f"{name}: the LDS and the direct image kernels differ in {int((out != out_o).sum())} elements"


@pytest.mark.parametrize("form", [R.LDS, R.SPLIT], ids=["LDS", "SPLIT"])
def test_enc_staged_persistent_loop(env, monkeypatch, form):
    """32 -> 64 @8 at one frame per block with F = grid + 3: three workgroups take a second block, statistics carried across the trips.
    worst error / bound on an MI355X (out, sum, sum of squares): LDS 0.013, 0.00003, 0.00008; split 0.0028, 0.00003, 0.00005;
    split against the LDS body, worst frame: max 0.54, rms 0.54."""
    rt, pk, lib, dev = env
    cin, cout, Hin = R.WRAP_STAGED_SHAPE
    Fr = _probe_grid(env, monkeypatch, form, cin, cout, Hin, 1) + 3          # _run_layer asserts grid = F - 3 and F blocks
    c = R.layer_case(f"wrap-{cin}-{cout}-{Hin}-F{Fr}", cin, cout, Hin, Hin, Fr, affine=True, out_act=R.ACT_LRELU)
    if form == R.SPLIT:
        _run_split_beside_exact(env, monkeypatch, c, 1)
    else:
        _run_layer(env, monkeypatch, c, form, 1)


def test_enc_image_lds_persistent_loop(env, monkeypatch):
    """conv4x4s2_image_lds_kernel<64> with F = grid + 3 (grid from the query: the workgroups that fit the CUs' LDS at once).
    worst error / bound on an MI355X: 0.096."""
    rt, pk, lib, dev = env
    out2 = (C.c_int32 * 2)()
    rt.check(lib.gcpx_conv4x4s2_image_form(1 << 14, 64, 64, out2), "conv4x4s2_image_form")
    Fr = out2[1] + 3
    assert out2[0] == R.IMAGE_LDS and Fr < (1 << 14)
    _, _, grid = _run_image(env, monkeypatch, R.image_case(f"wrap-64-F{Fr}", 64, 64, Fr, R.ACT_LRELU), R.IMAGE_LDS)
    assert grid == Fr - 3, "F was sized for another grid"


def test_enc_direct_persistent_loop(env, monkeypatch):
    """conv4x4s2_kernel<1,8,2,2> at 16 -> 32 @64 without statistics, with blocks grid - 1, grid and grid + 1 present: float64 on the
    frames that hold them and on the first and last frame, every other output finite (frames are independent).  About 134 MB of input, 0.2 s.
    worst error / bound on an MI355X: 0.025."""
    rt, pk, lib, dev = env
    cin, cout, Hin = R.WRAP_DIRECT
    grid = _probe_grid(env, monkeypatch, R.DIRECT, cin, cout, Hin)          # without statistics; _run_layer asserts it for F
    per_frame, per_blk = (Hin // 2) ** 2, 16 * 16
    Fr = -(-((grid + 1) * per_blk + 1) // per_frame)
    assert -(-Fr * per_frame // per_blk) >= grid + 2
    c = R.layer_case(f"wrap-direct-F{Fr}", cin, cout, Hin, Hin, Fr, affine=True, out_act=R.ACT_NONE)
    frames = sorted({0, Fr - 1} | set(range((grid - 1) * per_blk // per_frame, ((grid + 2) * per_blk - 1) // per_frame + 1)))
    _run_layer(env, monkeypatch, c, R.DIRECT, stats=False, ref_frames=frames)
