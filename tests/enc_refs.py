"""FLOAT64 reference, rounding bounds and the shared cases of the encoder convs' form tests (tests/test_gpu_enc_forms.py runs
gcpx_conv4x4s2 and gcpx_conv4x4s2_image on them once per device body and frames-per-block choice, tests/test_enc_refs_cpu.py pins
everything here without a GPU).

The reference is plain torch in float64: `evaluate(case)` applies the source's per-channel affine, LeakyReLU(0.2), the 4x4 stride-2
pad-1 conv as sixteen strided slices of the zero-padded input times the tap's [Cout, Cin] matrix, bias, the output activation, and
per-channel sum and sum of squares over frames and pixels.  It is no transcription of csrc/conv_enc*.hip and does not call F.conv2d
(the CPU test compares it with F.conv2d).  The image layer is the same function on a 3-channel input without affine.

Bounds (derived, nothing measured).  u = 2^-24, K = 16 Cin (48 for the image layer), x^ = the transformed input in float64,
S = sum_k |w_k| |x^_k| over the taps inside the image, b = the bias.

  exact f32 bodies (direct, LDS, image):
    * an f32 dot product of length K, in any order, with or without fma, errs by at most K u S to first order;
    * the fused affine is one fma and LeakyReLU one multiply: the x^ a kernel holds is x^ (1 + d)^2, |d| <= u, carried through
      sum |w| |x^|: 2 u S;
    * the bias add and the output LeakyReLU: 2 roundings of a value of at most S + |b|.
    Four roundings besides the dot product, taken as 8 as tests/gemm_refs.py does:
        e = (K + 8) u (S + |b|) + 2^-126                (2^-126: an f32 result below the normal range may be flushed)
    LeakyReLU is 1-Lipschitz, so the bound holds behind the output activation.

  split-f16 bodies (csrc/split_mfma.h, csrc/conv3x3_split.hip, csrc/conv_enc_split.hip) — DERIVED, not the comparison with the f32
  body that tests/test_gpu_kernels.py::test_conv4x4s2_split_error_vs_float64 uses:
    a block of fpb frames is staged as x^ in f32, X = the block's largest |x^| gives ONE power of two 2^Ex with X 2^Ex in [2^14, 2^15),
    xs = x^ 2^Ex = x1 + x2 + dx with x1 = rn16(xs), x2 = rn16(xs - x1).  rn16 errs by 2^-11 relatively on a normal f16 and by at
    most 2^-25 absolutely on a subnormal one: |xs - x1| <= 2^-11 |xs| and |dx| <= 2^-22 |xs| + 2^-25.  The weights likewise with
    one 2^Ew for the tensor (packing.split_f16): |dw| <= 2^-22 |ws| + 2^-25.  The kernel adds x1 w1 + x1 w2 + x2 w1 — each product of
    two f16 is exact in f32 — so against xs ws it lacks x2 w2 + dx ws + (xs - dx) dw:
        |x2 w2| <= (2^-11 |xs| + 2^-25)(2^-11 |ws| + 2^-25),    |dx ws| <= (2^-22 |xs| + 2^-25) |ws|,    likewise dw:
        per product 3 2^-22 |xs ws| + (2^-25 + 2^-36)(|xs| + |ws|) + 2^-50, and unscaled, with 2^-Ex <= 2^-14 X and 2^-Ew <= 2^-14 Wmax:
        12 u |x^ w| + 2^-38 (X |w| + Wmax |x^|) + 2^-78 X Wmax        (2^-38: the 2^-39 floor of split_mfma.h, doubled for 2^-36);
    the f32 accumulator takes 3 K terms of total magnitude (1 + 2^-10) S: 3 K u S (1 + 2^-10), taken as (3 K + 1) u S;
    the affine (2 u S, and X is taken as the float64 maximum times 1 + 2^-20), the epilogue's fma with the bias, LeakyReLU: as above.
        e = (3 K + 24) u (S + |b|) + 2^-38 (X sum|w| + Wmax sum|x^|) + 2^-78 K X Wmax + 2^-126
    with sum|w| over the taps inside the image and X per block — so the bound of a frame depends on fpb and on its neighbours in
    the block, and a small frame beside a 1000 times larger one is still held to 1e-4 of its own S + |b| at K = 512.

  The derived split bound is a ceiling, about 1e-4 S: no right kernel can exceed it, but one-piece f16 arithmetic at K >= 512 stays
  under it too.  What the split bodies are FOR — f32-equivalent results — is held by the project's criterion for every split-f16
  kernel (tests/test_gpu_kernels.py::test_conv4x4s2_split_error_vs_float64), against the exact body run on the same
  case, here PER FRAME so that a small frame beside a large one is judged on its own scale (`split_vs_exact`):
        max |err split| <= 2 max |err exact| + 4e-7 scale,    rms err split <= 1.5 rms err exact + 1e-12 scale,    scale = max |ref|
  over the frame.  A lost second piece of either operand (2^-12 relative per product) or a block scale 2^14 too small (the second
  piece of a frame 1000 times below the block's maximum turns subnormal) is 10 - 1000 times outside it (tests/test_enc_refs_cpu.py).

  statistics: the rows of stats_partial are summed in float64 by the test.  The output tile of a 16 x 16 MFMA gives a lane one pixel of
  a 16-pixel group, so of a channel's n = F Hout Wout outputs v at most ceil(n / 16) pass through one lane's running sum; four steps
  join the 16 lanes of a row and at most three additions the wavefronts: a summation tree of depth d = ceil(n / 16) + 8 at the most,
  and a tree of depth d errs by at most d u sum |v| whatever its order:
        sum:             sum e + d u sum |v|
        sum of squares:  sum (2 |v| e + e^2 + u v^2) + d u sum v^2.

Inputs are unit scale, weights 1 / sqrt(K), bias 0.1: S is about 0.5 sqrt(K) and the f32 bound 2e-4 at K = 256, 6e-4 at K = 1024;
a dropped tap or 16-channel group changes an output by about 1 / sqrt(16) resp. 1 / sqrt(K / 16): 1e2 - 1e3 bounds."""
import dataclasses
import functools

import numpy as np
import torch

U = 2.0 ** -24
NAN = float("nan")
SLOPE = float(np.float32(0.2))          # the kernels' LeakyReLU slope: the f32 constant 0.2f
ACT_NONE, ACT_LRELU = 0, 1
ROUNDINGS = 8
TINY = 2.0 ** -126
# gcpx_enc_form_id (include/gcpx.h)
DIRECT, LDS, SPLIT, IMAGE_DIRECT, IMAGE_LDS = 0, 1, 2, 3, 4
FORM_NAMES = {DIRECT: "DIRECT", LDS: "LDS", SPLIT: "SPLIT", IMAGE_DIRECT: "IMAGE_DIRECT", IMAGE_LDS: "IMAGE_LDS"}

# (Cin, Cout, Hin) of the five square shapes with an LDS and a split form -> the frames-per-block values under test: 1, the largest
# the kernel stages, and between them values that leave the last pixel-group row of wavefronts short or idle
STAGED_FPB = {(16, 32, 32): (1,), (32, 64, 16): (1, 3, 4), (64, 128, 8): (1, 5, 8), (16, 32, 16): (1, 3, 4), (32, 64, 8): (1, 2, 5, 16)}
STAGED_MAX_FPB = {s: v[-1] for s, v in STAGED_FPB.items()}


def staged_cases():
    """(form, (Cin, Cout, Hin), fpb, F): F = 2 fpb + 1 (a last block with one frame) and 2 fpb - 1 (a last block missing one)"""
    return [(form, s, fpb, F) for form in (LDS, SPLIT) for s, fpbs in STAGED_FPB.items() for fpb in fpbs for F in (2 * fpb + 1, 2 * fpb - 1)]


# split-f16 scale cases: (shape, fpb): block 0 begins with a frame 1000 times smaller than its others, block 1 is all zero, the last block
# has one frame
SPLIT_SCALE = [((16, 32, 32), 1), ((32, 64, 16), 3), ((64, 128, 8), 5), ((16, 32, 16), 3), ((32, 64, 8), 5)]

# direct bodies: (name, Cin, Cout, Hin, Win, F, forced).  forced: a shape with an LDS form under GCPX_ENC_DIRECT=1
DIRECT_CASES = [
    ("forced-16-32-16", 16, 32, 16, 16, 3, True), ("forced-32-64-8", 32, 64, 8, 8, 3, True), ("forced-64-128-8", 64, 128, 8, 8, 3, True),
    ("16-32-16x32", 16, 32, 16, 32, 3, False),        # 384 pixels = 24 groups: the second workgroup is half valid
    ("32-64-8x16", 32, 64, 8, 16, 3, False),          # 96 pixels = 6 groups of 8
    ("64-128-4x4", 64, 128, 4, 4, 5, False),          # 20 pixels: the second group has 4 valid lanes, 6 groups of the workgroup none
    ("16-32-8x8", 16, 32, 8, 8, 3, False),            # 48 pixels = 3 groups of 16
]

# image bodies: (name, form, Hin, Win, F)
IMAGE_CASES = [
    ("lds-32", IMAGE_LDS, 32, 32, 3), ("lds-64", IMAGE_LDS, 64, 64, 3), ("direct-32", IMAGE_DIRECT, 32, 32, 3),
    ("direct-6x10", IMAGE_DIRECT, 6, 10, 3),          # 45 output pixels: 13 valid lanes in the last group
    ("direct-16x48", IMAGE_DIRECT, 16, 48, 1), ("direct-128", IMAGE_DIRECT, 128, 128, 2),
]
WRAP_STAGED_SHAPE = (32, 64, 8)         # persistent loops: F = grid + 3 at fpb = 1
WRAP_DIRECT = (16, 32, 64)              # more than grid * 16 * 16 output pixels


def form_env(form, fpb=0):
    """environment that forces a form (every switch is read by the entry points on each call)"""
    if form == DIRECT:
        return {"GCPX_ENC_DIRECT": "1", "GCPX_ENC_NOSPLIT": "1"}
    if form == IMAGE_DIRECT:
        return {"GCPX_ENC_IMAGE_DIRECT": "1"}
    return {"GCPX_ENC_FPB": str(fpb)} if fpb else {}


def expected_form(form, F, Hout, Wout, Cout, fpb, nrows, stats):
    """what gcpx_conv4x4s2_form answers: [form, fpb, grid, nblk] with nrows = gcpx_conv4x4s2_grid()"""
    if form == DIRECT:
        per_blk = 16 if Cout == 32 else 8
        nblk = -(-(-(-F * Hout * Wout // 16)) // per_blk)
        return [DIRECT, 0, nrows if stats else min(nrows, nblk), nblk]
    nblk = -(-F // fpb)
    return [form, fpb, min(nblk, nrows), nblk]


@dataclasses.dataclass
class Case:
    name: str
    x: torch.Tensor                     # f32 [F][Cin][Hin][Win]
    w: torch.Tensor                     # f32 [Cout][Cin][4][4]
    bias: torch.Tensor                  # f32 [Cout]
    scale: torch.Tensor = None          # f32 [Cin]: the source's affine, with shift
    shift: torch.Tensor = None
    act: int = ACT_NONE                 # activation on load
    out_act: int = ACT_NONE

    @property
    def F(self):
        return self.x.shape[0]

    @property
    def K(self):
        return 16 * self.x.shape[1]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def layer_case(name, cin, cout, Hin, Win, F, *, affine, out_act, seed=0, frame_amp=None):
    """unit-scale frames (frame f times frame_amp[f] when given), weights 1 / sqrt(K), bias 0.1; affine: scale in [0.5, 1.5), shift
    0.2, LeakyReLU on load"""
    g = _gen(1000 * Hin + 10 * cin + F + seed)
    x = torch.randn(F, cin, Hin, Win, generator=g)
    if frame_amp is not None:
        x = x * torch.tensor(frame_amp, dtype=torch.float32)[:, None, None, None]
    w = torch.randn(cout, cin, 4, 4, generator=g) / (16 * cin) ** 0.5
    b = torch.randn(cout, generator=g) * 0.1
    c = Case(name, x, w, b, out_act=out_act)
    if affine:
        c.scale, c.shift, c.act = torch.rand(cin, generator=g) + 0.5, torch.randn(cin, generator=g) * 0.2, ACT_LRELU
    return c


FRAME_AMP = (1.0, 4.0, 0.25)            # frame f is scaled by FRAME_AMP[f % 3]: no frame of a block stands for the block's magnitude


def variants(name, cin, cout, Hin, Win, F, seed=0):
    """the two input variants every layer test runs: affine + LeakyReLU on load with a raw output, and a plain source with LeakyReLU
    out; frames of three magnitudes in turn"""
    amp = [FRAME_AMP[f % 3] for f in range(F)]
    return [layer_case(f"{name}/affine", cin, cout, Hin, Win, F, affine=True, out_act=ACT_NONE, seed=seed, frame_amp=amp),
            layer_case(f"{name}/lrelu-out", cin, cout, Hin, Win, F, affine=False, out_act=ACT_LRELU, seed=seed + 1, frame_amp=amp)]


def split_scale_case(shape, fpb):
    cin, cout, Hin = shape
    F = 2 * fpb + 1
    amp = [1.0] * F
    if fpb > 1:
        amp[0] = 1e-3                   # the block's FIRST frame is the small one: its scale must come from all of its frames
    for f in range(fpb, 2 * fpb):
        amp[f] = 0.0
    c = layer_case(f"scale-{cin}-{cout}-{Hin}-fpb{fpb}", cin, cout, Hin, Hin, F, affine=False, out_act=ACT_NONE, seed=7, frame_amp=amp)
    c.bias = c.bias * 1e-3              # of the small frame's size: its outputs, and so the scale it is judged on, are its own
    return c


def image_case(name, Hin, Win, F, out_act):
    g = _gen(100 * Hin + Win + F + out_act)
    x = torch.rand(F, 3, Hin, Win, generator=g) * 2 - 1
    return Case(name, x, torch.randn(16, 3, 4, 4, generator=g) / 7.0, torch.randn(16, generator=g) * 0.1, out_act=out_act)


def _lrelu(v):
    return torch.where(v > 0, v, v * SLOPE)


def transformed(c, dtype=torch.float64):
    x = c.x.to(dtype)
    if c.scale is not None:
        x = x * c.scale.to(dtype)[None, :, None, None] + c.shift.to(dtype)[None, :, None, None]
    return _lrelu(x) if c.act == ACT_LRELU else x


def conv_taps(xh, w, skip=()):
    """4x4 stride-2 pad-1 conv of xh [F][Cin][H][W] with w [Cout][Cin][4][4]: sixteen strided slices of the padded input.
    skip: (ky, kx, channel slice) terms left out (the CPU test's planted faults)"""
    Fr, cin, H, W = xh.shape
    Ho, Wo = H // 2, W // 2
    xp = torch.zeros(Fr, cin, H + 2, W + 2, dtype=xh.dtype)
    xp[:, :, 1:H + 1, 1:W + 1] = xh
    out = torch.zeros(Fr, w.shape[0], Ho, Wo, dtype=xh.dtype)
    for ky in range(4):
        for kx in range(4):
            wt = w[:, :, ky, kx].clone()
            for sky, skx, sl in skip:
                if (sky, skx) == (ky, kx):
                    wt[:, sl] = 0
            out += torch.einsum("fchw,oc->fohw", xp[:, :, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2], wt)
    return out


def evaluate(c, dtype=torch.float64):
    """{"xh": transformed input, "pre": conv + bias, "out": behind out_act [F][Cout][Hout][Wout], "s1", "s2": per-channel sums}"""
    xh = transformed(c, dtype)
    pre = conv_taps(xh, c.w.to(dtype)) + c.bias.to(dtype)[None, :, None, None]
    out = _lrelu(pre) if c.out_act == ACT_LRELU else pre
    return {"xh": xh, "pre": pre, "out": out, "s1": out.sum((0, 2, 3)), "s2": (out * out).sum((0, 2, 3))}


def bounds(c, ref, kind="f32", fpb=1):
    """elementwise bound of "out" and the bounds of the two statistics (module docstring).  kind "split": blocks of fpb frames"""
    xa, wa = ref["xh"].abs(), c.w.double().abs()
    S = conv_taps(xa, wa) + c.bias.double().abs()[None, :, None, None]
    if kind == "f32":
        e = (c.K + ROUNDINGS) * U * S + TINY
    else:
        Fr = c.F
        X = torch.zeros(Fr, dtype=torch.float64)
        for f0 in range(0, Fr, fpb):
            X[f0:f0 + fpb] = xa[f0:f0 + fpb].max() * (1 + 2.0 ** -20)
        wmax = float(wa.max())
        sum_w = conv_taps(torch.ones_like(xa[:1]), wa)                                # taps inside the image only
        sum_x = conv_taps(xa, torch.ones_like(wa[:1]))
        floor = 2.0 ** -38 * (X[:, None, None, None] * sum_w + wmax * sum_x) + 2.0 ** -78 * c.K * X[:, None, None, None] * wmax
        e = (3 * c.K + 24) * U * S + floor + TINY
    v = ref["out"].abs()
    d = -(-v.shape[0] * v.shape[2] * v.shape[3] // 16) + 8
    b1 = e.sum((0, 2, 3)) + d * U * v.sum((0, 2, 3))
    b2 = (2 * v * e + e * e + U * v * v).sum((0, 2, 3)) + d * U * (v * v).sum((0, 2, 3))
    return {"out": e, "s1": b1, "s2": b2}


def split_vs_exact(got_split, got_exact, ref_out):
    """the project's split-f16 criterion, frame by frame: {"max": worst of max|err split| / (2 max|err exact| + 4e-7 scale), "rms":
    worst of rms err split / (1.5 rms err exact + 1e-12 scale)} with scale = the frame's max |ref|; all three [F][Cout][Hout][Wout]"""
    es, ee = (got_split - ref_out).abs().flatten(1), (got_exact - ref_out).abs().flatten(1)
    scale = ref_out.abs().flatten(1).max(1).values
    r_max = es.max(1).values / (2.0 * ee.max(1).values + 4e-7 * scale + TINY)
    r_rms = es.pow(2).mean(1).sqrt() / (1.5 * ee.pow(2).mean(1).sqrt() + 1e-12 * scale + TINY)
    return {"max": float(r_max.max()), "rms": float(r_rms.max())}


def ratios(got, ref, bnd):
    """worst |got - ref| / bound of each of out, s1, s2 present in got (float64 tensors in the reference's layout)"""
    return {k: float(((got[k] - ref[k]).abs() / bnd[k]).max()) for k in got}


@functools.lru_cache(maxsize=None)
def cpu_cases():
    """one small case of every family (the CPU test evaluates them in float32 and plants faults in them)"""
    cs = []
    for (cin, cout, Hin), fpbs in STAGED_FPB.items():
        cs += variants(f"{cin}-{cout}-{Hin}", cin, cout, Hin, Hin, 3)
    for name, cin, cout, Hin, Win, F, _ in DIRECT_CASES[3:]:
        cs += variants(name, cin, cout, Hin, Win, F)
    cs += [split_scale_case(s, fpb) for s, fpb in SPLIT_SCALE[1:3]]
    cs += [image_case(name, Hin, Win, F, ACT_LRELU) for name, _, Hin, Win, F in IMAGE_CASES if Hin <= 32]
    return tuple(cs)
