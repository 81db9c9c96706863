"""No GPU: pins tests/enc_refs.py, the float64 reference and the bounds tests/test_gpu_enc_forms.py holds the encoder convs to.

  * the reference equals F.conv2d in float64 on every case;
  * torch's own float32 evaluation of every case lies inside 1.0 x bound (f32 bound), and so does an emulation of the split-f16
    arithmetic (two f16 pieces of both operands under power-of-two scales, three products, float64 accumulation) inside the split bound;
  * a dropped tap, a dropped 16-channel group of one tap, a frame read from its neighbour and a border tap that is not zero each push
    cases above 1.0 — of either bound;
  * an emulation that loses a second f16 piece, or takes a block scale 2^14 too small, stays inside the derived split ceiling at
    K >= 512 but falls outside the criterion against the exact body that the GPU test asserts beside it (enc_refs.split_vs_exact);
  * the tables of forms and frames-per-block values cover what their comments in enc_refs.py say (1, each kernel's maximum, values
    between that leave wavefronts idle), the GPU test parametrizes exactly them, and the dispatch queries (which need no GPU: 256
    CUs are assumed without a device) answer what the tests will assert."""
import ctypes as C
import os
import re

import pytest
import torch
import torch.nn.functional as F

import enc_refs as R

CASES = R.cpu_cases()
IDS = [c.name for c in CASES]
HERE = os.path.dirname(os.path.abspath(__file__))


def _is_image(c):
    return c.x.shape[1] == 3


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_reference_is_conv2d_in_float64(c):
    ref = R.evaluate(c)
    x = c.x.double()
    if c.scale is not None:
        x = F.leaky_relu(x * c.scale.double()[None, :, None, None] + c.shift.double()[None, :, None, None], R.SLOPE)
    want = F.conv2d(x, c.w.double(), c.bias.double(), stride=2, padding=1)
    if c.out_act == R.ACT_LRELU:
        want = F.leaky_relu(want, R.SLOPE)
    scale = float(want.abs().max()) + 1e-300
    assert float((ref["out"] - want).abs().max()) <= 1e-13 * scale
    assert torch.allclose(ref["s1"], want.sum((0, 2, 3)), rtol=1e-12, atol=1e-12 * scale)
    assert torch.allclose(ref["s2"], (want * want).sum((0, 2, 3)), rtol=1e-12, atol=1e-12 * scale)


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_float32_evaluation_is_inside_the_f32_bound(c):
    ref = R.evaluate(c)
    got = R.evaluate(c, torch.float32)
    r = R.ratios({k: got[k].double() for k in ("out", "s1", "s2")}, ref, R.bounds(c, ref))
    print(c.name, r)
    assert max(r.values()) <= 1.0, r


def _split_emulation(c, fpb, fault=None):
    """the arithmetic csrc/conv_enc_split.hip documents, with float64 accumulation: x^ in f32, one power-of-two scale per block of fpb
    frames, two f16 pieces of x^ and of w, x1 w1 + x1 w2 + x2 w1.  fault: "no-x2" / "no-w2" leave a second piece out, "one-piece"
    both, "low-scale" puts a block's maximum in [1, 2) instead of [2^14, 2^15)"""
    xh = R.transformed(c, torch.float32)

    def pieces(v, amax, top=14):
        e = 0 if amax == 0 else top - int(torch.floor(torch.log2(torch.tensor(amax, dtype=torch.float64))))
        vs = v.double() * 2.0 ** e
        p1 = vs.float().half()
        p2 = (vs - p1.double()).float().half()
        return p1.double(), p2.double(), 2.0 ** -e

    w1, w2, iw = pieces(c.w, float(c.w.abs().max()))
    out = torch.zeros(c.F, c.w.shape[0], xh.shape[2] // 2, xh.shape[3] // 2, dtype=torch.float64)
    for f0 in range(0, c.F, fpb):
        blk = xh[f0:f0 + fpb]
        x1, x2, ix = pieces(blk, float(blk.abs().max()), 0 if fault == "low-scale" else 14)
        acc = R.conv_taps(x1, w1)
        if fault not in ("no-w2", "one-piece"):
            acc = acc + R.conv_taps(x1, w2)
        if fault not in ("no-x2", "one-piece"):
            acc = acc + R.conv_taps(x2, w1)
        out[f0:f0 + fpb] = acc * (ix * iw)
    pre = out + c.bias.double()[None, :, None, None]
    out = R._lrelu(pre) if c.out_act == R.ACT_LRELU else pre
    return {"out": out, "s1": out.sum((0, 2, 3)), "s2": (out * out).sum((0, 2, 3))}


@pytest.mark.parametrize("fpb", [1, 3])
@pytest.mark.parametrize("c", [c for c in CASES if not _is_image(c)], ids=[c.name for c in CASES if not _is_image(c)])
def test_split_f16_emulation_is_inside_the_split_bound(c, fpb):
    ref = R.evaluate(c)
    r = R.ratios(_split_emulation(c, fpb), ref, R.bounds(c, ref, "split", fpb))
    print(c.name, fpb, r)
    assert max(r.values()) <= 1.0, r


LAYER_CASES = [c for c in CASES if not _is_image(c)]


def test_split_f16_emulation_is_inside_the_criterion_against_float32_and_faults_are_not():
    """what the GPU test asserts of a split body beside the exact one, with torch's float32 evaluation as the exact body: the right
    emulation passes on every case; a lost second piece fails on every case; the low block scale fails on the cases whose blocks hold a
    frame 1000 times smaller than their maximum — while both stay inside the derived ceiling on cases of K >= 512"""
    under_ceiling = 0
    for c in LAYER_CASES:
        ref = R.evaluate(c)
        exact = R.evaluate(c, torch.float32)["out"].double()
        r = R.split_vs_exact(_split_emulation(c, 3)["out"], exact, ref["out"])
        assert r["max"] <= 1.0 and r["rms"] <= 1.0, (c.name, r)
        for fault in ("no-x2", "no-w2", "one-piece"):
            got = _split_emulation(c, 3, fault)["out"]
            r = R.split_vs_exact(got, exact, ref["out"])
            assert r["max"] > 10.0 and r["rms"] > 10.0, f"{c.name}: {fault} is only {r} of the criterion"
            under_ceiling += float(((got - ref["out"]).abs() / R.bounds(c, ref, "split", 3)["out"]).max()) <= 1.0
        if c.name.startswith("scale"):
            got = _split_emulation(c, 3, "low-scale")["out"]
            r = R.split_vs_exact(got, exact, ref["out"])
            assert r["max"] > 10.0 and r["rms"] > 10.0, f"{c.name}: low-scale is only {r} of the criterion"
            assert float(((got - ref["out"]).abs() / R.bounds(c, ref, "split", 3)["out"]).max()) <= 1.0
    assert under_ceiling > 0, "the derived ceiling alone saw every lost piece: the criterion would not be needed"


def _planted(c, fault):
    """float32 evaluation of c with one fault planted"""
    xh = R.transformed(c, torch.float32)
    w = c.w
    cin = xh.shape[1]
    if fault == "tap":
        pre = R.conv_taps(xh, w, skip=[(3, 1, slice(None))])
    elif fault == "group":                                  # the last 16 channels (the last plane of an image) at one inner tap
        pre = R.conv_taps(xh, w, skip=[(1, 2, slice(cin - 16, cin) if cin >= 16 else slice(cin - 1, cin))])
    elif fault == "neighbour":                              # the last frame computed from the frame before it
        xh = xh.clone()
        xh[-1] = xh[-2] if c.F > 1 else xh[-1].flip(0)
        pre = R.conv_taps(xh, w)
    else:                                                   # "border": the taps left of the image read column 0 instead of zero
        Fr, _, H, W = xh.shape
        xp = torch.zeros(Fr, cin, H, W + 2)
        xp[..., 1:W + 1] = xh
        xp[..., 0] = xh[..., 0]
        pre = F.conv2d(xp, w, stride=2, padding=(1, 0))
    pre = pre + c.bias[None, :, None, None]
    return (R._lrelu(pre) if c.out_act == R.ACT_LRELU else pre).double()


@pytest.mark.parametrize("fault", ["tap", "group", "neighbour", "border"])
def test_a_planted_fault_is_outside_both_bounds(fault):
    """every case with non-zero frames must see the fault, under the f32 bound and under the wider split bound at the largest block"""
    for c in CASES:
        ref = R.evaluate(c)
        got = _planted(c, fault)
        kinds = [("f32", 1)] if _is_image(c) else [("f32", 1), ("split", c.F)]
        for kind, fpb in kinds:
            r = float(((got - ref["out"]).abs() / R.bounds(c, ref, kind, fpb)["out"]).max())
            assert r > 10.0, f"{c.name}: a wrong {fault} is only {r:.3g} of the {kind} bound"


def test_the_tables_cover_what_their_comments_say():
    assert (R.DIRECT, R.LDS, R.SPLIT, R.IMAGE_DIRECT, R.IMAGE_LDS) == _enum_of_the_header() == _enum_of_the_runtime()
    assert R.STAGED_FPB == {(16, 32, 32): (1,), (32, 64, 16): (1, 3, 4), (64, 128, 8): (1, 5, 8), (16, 32, 16): (1, 3, 4),
                            (32, 64, 8): (1, 2, 5, 16)}
    cases = R.staged_cases()
    assert len(cases) == 2 * 2 * 14 and len(set(cases)) == len(cases)
    for form, shape, fpb, Fr in cases:
        assert form in (R.LDS, R.SPLIT) and Fr in (2 * fpb + 1, 2 * fpb - 1) and Fr >= 1
    assert [(c[1], c[2], c[3], c[4], c[5]) for c in R.DIRECT_CASES[3:]] == [(16, 32, 16, 32, 3), (32, 64, 8, 16, 3), (64, 128, 4, 4, 5),
                                                                           (16, 32, 8, 8, 3)]
    assert sorted(c[2] for c in R.DIRECT_CASES[:3]) == [32, 64, 128] and all(c[5] == 3 and c[6] for c in R.DIRECT_CASES[:3])
    assert [(c[1], c[2], c[3]) for c in R.IMAGE_CASES] == [(R.IMAGE_LDS, 32, 32), (R.IMAGE_LDS, 64, 64), (R.IMAGE_DIRECT, 32, 32),
                                                            (R.IMAGE_DIRECT, 6, 10), (R.IMAGE_DIRECT, 16, 48), (R.IMAGE_DIRECT, 128, 128)]
    # the GPU test parametrizes these tables and nothing of its own
    with open(os.path.join(HERE, "test_gpu_enc_forms.py")) as f:
        text = f.read()
    for table in ("R.staged_cases()", "R.SPLIT_SCALE", "R.DIRECT_CASES", "R.IMAGE_CASES"):
        assert re.search(r"parametrize\([^\n]*" + re.escape(table), text), f"test_gpu_enc_forms.py does not parametrize {table}"


def _enum_of_the_header():
    with open(os.path.join(os.path.dirname(HERE), "include", "gcpx.h")) as f:
        text = f.read()
    return tuple(int(re.search(r"GCPX_ENC_FORM_" + n + r" = (\d+)", text).group(1)) for n in ("DIRECT", "LDS", "SPLIT", "IMAGE_DIRECT", "IMAGE_LDS"))


def _enum_of_the_runtime():
    from video_gcp_amd import runtime as rt
    return rt.ENC_FORM_DIRECT, rt.ENC_FORM_LDS, rt.ENC_FORM_SPLIT, rt.ENC_FORM_IMAGE_DIRECT, rt.ENC_FORM_IMAGE_LDS


@pytest.fixture(scope="module")
def lib():
    from video_gcp_amd import runtime as rt
    if not os.path.exists(rt.LIB_PATH):
        import sys
        sys.path.insert(0, os.path.dirname(HERE))
        import __graft_entry__
        __graft_entry__.build()
    return rt, rt.load_library()


def _query(lib, cin, cout, Hin, Win, Fr, split=False, stats=False):
    rt, L = lib
    a = rt.ConvArgs()
    a.nsrc, a.Cin, a.F, a.Hin, a.Win, a.Hout, a.Wout, a.Cout, a.out_pitch = 1, cin, Fr, Hin, Win, Hin // 2, Win // 2, cout, cout
    a.src[0].ptr, a.src[0].C, a.src[0].frame_div = 64, cin, 1
    a.wpk = a.bias = a.out = 64                              # the query reads no memory: any non-null address
    if split:
        a.wpk_split, a.split_layout = 64, rt.SPLIT_PLAIN
    if stats:
        a.stats_partial = 64
    out4 = (C.c_int32 * 4)()
    st = L.gcpx_conv4x4s2_form(C.byref(a), out4)
    return st, list(out4)


def test_the_query_answers_what_the_gpu_tests_assert(lib, monkeypatch):
    rt, L = lib
    G = L.gcpx_conv4x4s2_grid()
    for form, (cin, cout, Hin), fpb, Fr in R.staged_cases():
        for k, v in R.form_env(form, fpb).items():
            monkeypatch.setenv(k, v)
        st, got = _query(lib, cin, cout, Hin, Hin, Fr, split=form == R.SPLIT, stats=True)
        assert st == 0 and got == R.expected_form(form, Fr, Hin // 2, Hin // 2, cout, fpb, G, True), (form, cin, cout, Hin, fpb, Fr, got)
    monkeypatch.delenv("GCPX_ENC_FPB")
    # without the switch, frames up to the CU count are one round of workgroups for every candidate: one frame per block in both
    # cost models (what the older tests ran)
    for (cin, cout, Hin) in R.STAGED_FPB:
        for split in (False, True):
            assert _query(lib, cin, cout, Hin, Hin, min(63, G // 8), split=split)[1][:2] == [R.SPLIT if split else R.LDS, 1]
    # a value outside 1 .. the shape's maximum is ignored
    monkeypatch.setenv("GCPX_ENC_FPB", "5")
    assert _query(lib, 32, 64, 16, 16, min(63, G // 8))[1][:2] == [R.LDS, 1]
    monkeypatch.delenv("GCPX_ENC_FPB")
    for name, cin, cout, Hin, Win, Fr, forced in R.DIRECT_CASES:
        if forced:
            assert _query(lib, cin, cout, Hin, Win, Fr)[1][0] == R.LDS
            for k, v in R.form_env(R.DIRECT).items():
                monkeypatch.setenv(k, v)
        for stats in (False, True):
            st, got = _query(lib, cin, cout, Hin, Win, Fr, split=True, stats=stats)
            assert st == 0 and got == R.expected_form(R.DIRECT, Fr, Hin // 2, Win // 2, cout, 0, G, stats), (name, got)
        for k in R.form_env(R.DIRECT):
            monkeypatch.delenv(k, raising=False)
    # GCPX_ENC_DIRECT alone leaves the split form in place; GCPX_ENC_NOSPLIT alone gives the LDS form
    monkeypatch.setenv("GCPX_ENC_DIRECT", "1")
    assert _query(lib, 32, 64, 8, 8, 3, split=True)[1][0] == R.SPLIT
    monkeypatch.delenv("GCPX_ENC_DIRECT")
    monkeypatch.setenv("GCPX_ENC_NOSPLIT", "1")
    assert _query(lib, 32, 64, 8, 8, 3, split=True)[1][0] == R.LDS
    monkeypatch.delenv("GCPX_ENC_NOSPLIT")
    # training size: 1280 frames run several frames per block, and on 256 CUs (what the library assumes without a device, and what
    # an MI355X has) 5 in the LDS form of 32 -> 64 @8, 3 in the split form of 32 -> 64 @16.  The cost models read the CU count of a
    # device when there is one: the figures are asserted only where it is 256
    for got in (_query(lib, 32, 64, 8, 8, 1280)[1], _query(lib, 32, 64, 16, 16, 1280, split=True)[1]):
        assert got[1] >= 1 and got[3] == -(-1280 // got[1]) and got[2] == min(got[3], G)
    if G == 8 * 256:
        assert _query(lib, 32, 64, 8, 8, 1280)[1] == [R.LDS, 5, 256, 256]
        assert _query(lib, 32, 64, 16, 16, 1280, split=True)[1] == [R.SPLIT, 3, 427, 427]
    # argument errors as the launch gives them
    assert _query(lib, 24, 32, 8, 8, 3)[0] == -1 and _query(lib, 16, 48, 6, 10, 3)[0] == -2
    assert L.gcpx_conv4x4s2_form(None, (C.c_int32 * 4)()) == -1
    out2 = (C.c_int32 * 2)()
    for name, form, Hin, Win, Fr in R.IMAGE_CASES:
        for k, v in (R.form_env(form).items() if form == R.IMAGE_DIRECT else ()):
            monkeypatch.setenv(k, v)
        assert L.gcpx_conv4x4s2_image_form(Fr, Hin, Win, out2) == 0 and out2[0] == form, name
        monkeypatch.delenv("GCPX_ENC_IMAGE_DIRECT", raising=False)
    assert L.gcpx_conv4x4s2_image_form(3, 7, 8, out2) == -1 and L.gcpx_conv4x4s2_image_form(0, 8, 8, out2) == -1
    assert L.gcpx_conv4x4s2_image_form(1 << 16, 64, 64, out2) == -1
