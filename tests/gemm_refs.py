"""FLOAT64 reference, rounding bounds and the shared cases of the exact row GEMM's form tests (tests/test_gpu_gemm_forms.py runs
gcpx_gemm on them once per gemm_tile body, tests/test_gemm_refs_cpu.py pins everything here without a GPU).

The reference is plain torch: `evaluate(p, torch.float64)` follows the semantics include/gcpx.h states for gcpx_gemm_args — sources
gathered row by row (shift with zero rows outside [0, rpb), rowidx), affine + activation on load with channel = k % cmod, concatenated
along K, one F.linear per batch, bias, LReLU or the LSTM cell, per-row-block column sums — and is no transcription of csrc/gemm_tile.h.
The same function at torch.float32 is torch's own f32 result: the CPU test shows it inside the bounds before any kernel is asked to be.

Bounds (derived, nothing measured), u = 2^-24:
  * an f32 dot product of length K, in any order, with or without fma, errs by at most K u sum_k |x_k w_k| to first order;
  * further roundings of one output: the fma and the LReLU multiply of the affine on load (2, relative to x' and so to every product),
    three split-K combine adds, the bias add, the epilogue's LReLU multiply: 7, taken as 8:
        pre-activation bound = (K + 8) u (|x'| |w|^T + |b|)            elementwise, x' = the transformed input;
    LReLU is 1-Lipschitz, so the bound holds behind it too;
  * the LSTM cell: the four gates' bounds go through sigmoid / tanh, c = f c_prev + i g and h = o tanh(c) to first order in float64;
    on top the allowance test_gemm_lstm_epilogue_with_saturated_gates (tests/test_gpu_kernels.py) gives the device's activation forms:
    1e-5 for a gate, 1e-5 + 2 u |c| for c, h and h_copy;
  * a row block's column sum over n rows: the rows' element bounds + n u sum |v| (fewer than n additions, each on a partial sum of at
    most sum |v|); its sum of squares: sum (2 |v| e + e^2 + u v^2) + n u sum v^2, e = the element bound.
Inputs are unit scale, weights 1 / sqrt(K): |x'| |w|^T is about 0.6 sqrt(K), the bound about 2e-4 at K = 272, 6e-4 at K = 640 and
1e-3 at K = 1312 — two to three orders of magnitude below what a dropped or doubled k-group changes (about 4 / sqrt(K))."""
import dataclasses
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
NAN = float("nan")
SLOPE = float(np.float32(0.2))          # the kernels' LeakyReLU slope: the f32 constant 0.2f
ACT_NONE, ACT_LRELU = 0, 1
EPI_NONE, EPI_LRELU, EPI_LSTM = 0, 1, 2
ROUNDINGS = 8                           # see above
ACT_ALLOWANCE = 1e-5

# block shapes gemm_tile is instantiated with: (PR, CR) in 16 x 16 tiles
W_FORMS = [(4, 4), (4, 2), (4, 1), (2, 4), (2, 2), (2, 1), (1, 4), (1, 2), (1, 1)]
# split-K shapes and an (M, N) at which gcpx_gemm's cost models choose each one on 256 CUs for any K >= 256 (ks_block_choice: cost =
# rounds of workgroups over the CUs x (PR + CR), first minimum of <1,1>, <1,2>, <2,2>, <4,2>, <2,4>, taken when it is not <1,1> and
# <= 6; below 64 rows choose_tile's <1,1> runs as split-K single tiles)
KS_FORMS = {(1, 1): (37, 64), (1, 2): (70, 832), (2, 2): (130, 1024), (4, 2): (200, 2048), (2, 4): (70, 4160)}
KS_BATCHED = {(2, 2): (64, 512, 6)}     # (M, N, nbatch)
FORMS = [("W", pr, cr) for pr, cr in W_FORMS] + [("KS", pr, cr) for pr, cr in KS_FORMS]
K_SETS = {"k272": (16, 112, 144),       # k-groups 1, 7, 9: no multiple of UK = 2, 4, 8; one past 8; the first leaves wavefronts 1-3 idle
          "k1312": (1040, 272)}         # 65 k-groups: the ping-pong loop's last trip has one valid group for every UK
# Source widths of the other cases.  Under split-K wavefront w starts at k-group w UK: a source of fewer than 3 UK + 1 groups (25 for
# UK = 8) leaves wavefront 3 without work, and a wrong combine of its partial sum would go unseen — as it did with K = 272 alone.
# 33 groups = 4 x 8 + 1: every wavefront of every form works, wavefront 0 ends on a set with one valid group; 7 groups: a short source.
WIDE = (112, 528)


def form_id(form):
    kind, pr, cr = form
    return f"{kind}{pr}{cr}"


def form_shape(form):
    """(M, N) of a form's cases: W forms one full row block + a second with 5 rows (one partly valid tile, PR - 1 masked ones) and
    five column strips (the second column block keeps one wavefront); split-K forms the shape the cost model gives them"""
    kind, pr, cr = form
    return (16 * pr + 5, 16 * cr * 5) if kind == "W" else KS_FORMS[(pr, cr)]


def tile_env(form):
    """environment that forces a one-wavefront form (read by gcpx_gemm on every call); {} for the split-K forms"""
    kind, pr, cr = form
    return {"GCPX_GEMM_TILE": f"{pr},{cr},0", "GCPX_GEMM_NO_KS_BLOCKS": "1", "GCPX_GEMM_NOKS": "1"} if kind == "W" else {}


def expected_form(form, M, N, nbatch=1):
    """what gcpx_gemm_form answers for the form's case: [form, PR, CR, grid x, y, z]"""
    kind, pr, cr = form
    gx = -(-M // (16 * pr))
    return [0, pr, cr, gx, -(-(N // 16) // (4 * cr)), nbatch] if kind == "W" else [1, pr, cr, gx, N // (16 * cr), nbatch]


@dataclasses.dataclass
class Src:
    off: int                            # first float of the source in Problem.xbuf
    sb: int
    sr: int
    width: int
    shift: int = 0
    rowidx: torch.Tensor = None         # int32 [M]
    scale: torch.Tensor = None          # f32 [cmod]
    shiftv: torch.Tensor = None
    act: int = ACT_NONE
    cmod: int = 0


@dataclasses.dataclass
class Problem:
    name: str
    xbuf: torch.Tensor                  # f32, flat: every source lives in it (batch z of a source at + z * z_src_off)
    srcs: list
    M: int
    N: int
    K: int
    rpb: int
    w: torch.Tensor                     # f32 [nbatch][N][K]
    bias: torch.Tensor                  # f32 [nbatch][N]
    epi: int = EPI_NONE
    nbatch: int = 1
    z_src_off: int = 0
    stats: bool = False
    c_prev: torch.Tensor = None         # f32 [M][c_prev_stride], LSTM
    c_prev_stride: int = 0


def _gen(seed):
    return torch.Generator().manual_seed(seed)


class _Layout:
    """places sources in one flat buffer with padded row and batch strides (multiples of 4 floats: the kernel reads 16 bytes)"""

    def __init__(self):
        self.size = 0

    def dense(self, nbat, rpb, width, pad_r=4, pad_b=8):
        off, sr = self.size, width + pad_r
        sb = rpb * sr + pad_b
        self.size += nbat * sb + 16
        return off, sb, sr

    def table(self, rows, width, pad_r=12):
        off, sr = self.size, width + pad_r
        self.size += rows * sr + 16
        return off, sr


def _weights(g, nb, N, K):
    return torch.randn(nb, N, K, generator=g) / math.sqrt(K), torch.randn(nb, N, generator=g)


# ------------------------------------------------------------------------------------------------------------------------------
# the cases (cached: a reference is computed once and shared)
# ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tails_case(form, kset):
    """plain epilogue with bias; M, N of form_shape; sources of K_SETS[kset]; rows in batches of rpb = M (one batch)"""
    M, N = form_shape(form)
    widths = K_SETS[kset]
    g, lay = _gen(1000 + 7 * M + N + len(kset)), _Layout()
    srcs = [Src(*lay.dense(1, M, wd), width=wd) for wd in widths]
    w, b = _weights(g, 1, N, sum(widths))
    return Problem(f"tails-{form_id(form)}-{kset}", torch.randn(lay.size, generator=g), srcs, M, N, sum(widths), M, w, b)


@functools.lru_cache(maxsize=None)
def sources_case(form):
    """the conv1d-over-time form: three 256-wide sources shifted -1, 0, +1 inside batches of rpb = 20 rows with affine + LReLU on load
    (cmod = width), a 528-wide source gathered through rowidx, LReLU epilogue; the one-wavefront forms carry stats_partial (the
    split-K blocks refuse it).  K = 1296; the 33 k-groups of the gathered source give all four wavefronts of every split-K form work
    (see WIDE)."""
    M, N = form_shape(form)
    rpb, Cc, Wr, R = 20, 256, WIDE[1], 50
    g, lay = _gen(2000 + 7 * M + N), _Layout()
    nbat = -(-M // rpb)
    off, sb, sr = lay.dense(nbat, rpb, Cc)
    sc, sh = torch.rand(Cc, generator=g) + 0.5, torch.randn(Cc, generator=g) * 0.3
    srcs = [Src(off, sb, sr, Cc, shift=d, scale=sc, shiftv=sh, act=ACT_LRELU, cmod=Cc) for d in (-1, 0, 1)]
    toff, tsr = lay.table(R, Wr)
    srcs.append(Src(toff, 0, tsr, Wr, rowidx=torch.randint(0, R, (M,), generator=g, dtype=torch.int32)))
    K = 3 * Cc + Wr
    w, b = _weights(g, 1, N, K)
    return Problem(f"sources-{form_id(form)}", torch.randn(lay.size, generator=g), srcs, M, N, K, rpb, w, b, epi=EPI_LRELU,
                   stats=form[0] == "W")


@functools.lru_cache(maxsize=None)
def stats_on_split_k_case():
    """sources_case of split-K single tiles WITH stats_partial: below 64 rows nothing refuses the statistics, and wavefront 0 of each
    workgroup writes its 16-row block's sums behind the combine"""
    return dataclasses.replace(sources_case(("KS", 1, 1)), name="sources-KS11-stats", stats=True)


@functools.lru_cache(maxsize=None)
def batched_case(form, M, N, nb):
    """nbatch problems with their own rows, weights and bias; two sources of widths WIDE (K = 640), rows in batches of rpb = 7"""
    rpb = 7
    g, lay = _gen(3000 + 7 * M + N + nb), _Layout()
    srcs = [Src(*lay.dense(-(-M // rpb), rpb, wd), width=wd) for wd in WIDE]
    z = lay.size + 12
    w, b = _weights(g, nb, N, sum(WIDE))
    return Problem(f"batched-{form_id(form)}-x{nb}", torch.randn(z * nb, generator=g), srcs, M, N, sum(WIDE), rpb, w, b, nbatch=nb, z_src_off=z)


def batched_cases():
    out = [(f, *form_shape(f), 2) for f in FORMS if f[0] == "W"] + [(("KS", 1, 1), *KS_FORMS[(1, 1)], 2)]
    return out + [(("KS", pr, cr), M, N, nb) for (pr, cr), (M, N, nb) in KS_BATCHED.items()]


@functools.lru_cache(maxsize=None)
def lstm_case(form):
    """the LSTM cell epilogue: N = 4 H gate-interleaved columns, sources x and h of widths WIDE (K = 640), rows in batches of rpb = 7,
    c_prev rows at a stride > H; c_prev up to a few units so that f c_prev matters"""
    M, N = form_shape(form)
    H, rpb = N // 4, 7
    g, lay = _gen(4000 + 7 * M + N), _Layout()
    srcs = [Src(*lay.dense(-(-M // rpb), rpb, wd), width=wd) for wd in WIDE]
    w, b = _weights(g, 1, N, sum(WIDE))
    cps = H + 8
    return Problem(f"lstm-{form_id(form)}", torch.randn(lay.size, generator=g), srcs, M, N, sum(WIDE), rpb, w, b, epi=EPI_LSTM,
                   c_prev=torch.randn(M, cps, generator=g) * 1.5, c_prev_stride=cps)


def all_cases():
    """every Problem tests/test_gpu_gemm_forms.py runs"""
    out = [tails_case(f, k) for f in FORMS for k in K_SETS] + [sources_case(f) for f in FORMS] + [stats_on_split_k_case()]
    return out + [batched_case(*c) for c in batched_cases()] + [lstm_case(f) for f in FORMS]


def gemm_args(rt, p, addr, ob=0, orow=0, z_out_off=0, hb=0, hrow=0):
    """the runtime.GemmArgs of Problem p.  addr(name) -> address of the buffer `name`: "xbuf", "w" (the nbatch packs, N * K floats
    apart), "bias", "rowidx<s>" / "scale<s>" / "shiftv<s>" of source s, "out", "stats", "c_prev", "h_out", "c_out", "h_copy", "gates_out"."""
    a = rt.GemmArgs()
    for i, s in enumerate(p.srcs):
        a.src[i].ptr, a.src[i].sb, a.src[i].sr, a.src[i].width = addr("xbuf") + 4 * s.off, s.sb, s.sr, s.width
        a.src[i].shift, a.src[i].act, a.src[i].cmod = s.shift, s.act, s.cmod
        if s.rowidx is not None:
            a.src[i].rowidx = addr(f"rowidx{i}")
        if s.scale is not None:
            a.src[i].scale, a.src[i].shiftv = addr(f"scale{i}"), addr(f"shiftv{i}")
    a.nsrc, a.M, a.N, a.K, a.rpb, a.epi = len(p.srcs), p.M, p.N, p.K, p.rpb, p.epi
    a.wpk, a.bias = addr("w"), addr("bias")
    if p.nbatch > 1:
        a.nbatch, a.z_src_off, a.z_w_off, a.z_bias_off, a.z_out_off = p.nbatch, p.z_src_off, p.N * p.K, p.N, z_out_off
    if p.epi == EPI_LSTM:
        a.c_prev, a.c_prev_stride, a.h_out, a.c_out, a.hb, a.hrow = addr("c_prev"), p.c_prev_stride, addr("h_out"), addr("c_out"), hb, hrow
        a.h_copy, a.gates_out = addr("h_copy"), addr("gates_out")
    else:
        a.out, a.ob, a.orow = addr("out"), ob, orow
        if p.stats:
            a.stats_partial = addr("stats")
    return a


# ------------------------------------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------------------------------------
def row_offsets(M, rpb, sb, sr):
    """first element of row r = (b, j) in a buffer addressed as b * sb + j * sr"""
    r = torch.arange(M)
    return (r // rpb) * sb + (r % rpb) * sr


def source_rows(p, s, z, dtype):
    """the transformed input x' of source s for batch z: [M][width]"""
    r = torch.arange(p.M)
    if s.rowidx is not None:
        base, ok = s.rowidx.long() * s.sr, torch.ones(p.M, dtype=torch.bool)
    else:
        jj = r % p.rpb + s.shift
        ok = (jj >= 0) & (jj < p.rpb)
        base = (r // p.rpb) * s.sb + jj.clamp(0, p.rpb - 1) * s.sr
    x = p.xbuf[s.off + z * p.z_src_off + base[:, None] + torch.arange(s.width)[None]].to(dtype)
    if s.scale is not None:
        c = torch.arange(s.width) % s.cmod
        x = x * s.scale[c].to(dtype) + s.shiftv[c].to(dtype)
    if s.act == ACT_LRELU:
        x = torch.where(x > 0, x, x * SLOPE)
    return x * ok[:, None].to(dtype)


def inputs(p, z, dtype):
    return torch.cat([source_rows(p, s, z, dtype) for s in p.srcs], 1)


def stats_blocks(v, rows_per_block):
    """[row blocks][2][N]: column sums and sums of squares of each block of rows of v [M][N]"""
    return torch.stack([torch.stack([blk.sum(0), (blk * blk).sum(0)]) for blk in v.split(rows_per_block)])


def evaluate(p, dtype=torch.float64):
    """gcpx_gemm_args semantics in `dtype` -> dict: pre [nbatch][M][N] (bias added), out (behind the plain / LReLU epilogue), or for
    the LSTM cell gates [M][H][4] = (i, f, g, o), c, h [M][H]"""
    pre = torch.stack([F.linear(inputs(p, z, dtype), p.w[z].to(dtype), p.bias[z].to(dtype)) for z in range(p.nbatch)])
    res = {"pre": pre}
    if p.epi == EPI_LSTM:
        H = p.N // 4
        q = pre[0].view(p.M, H, 4)
        gates = torch.stack([torch.sigmoid(q[..., 0]), torch.sigmoid(q[..., 1]), torch.tanh(q[..., 2]), torch.sigmoid(q[..., 3])], -1)
        c = gates[..., 1] * p.c_prev[:, :H].to(dtype) + gates[..., 0] * gates[..., 2]
        res.update(gates=gates, c=c, h=gates[..., 3] * torch.tanh(c))
    else:
        res["out"] = torch.where(pre > 0, pre, pre * SLOPE) if p.epi == EPI_LRELU else pre
    return res


def bounds(p, ref):
    """the bounds of the module docstring for the float64 `ref` = evaluate(p): dict with the keys of ref"""
    pre_b = torch.stack([(p.K + ROUNDINGS) * U * (F.linear(inputs(p, z, torch.float64).abs(), p.w[z].double().abs()) + p.bias[z].double().abs())
                         for z in range(p.nbatch)])
    res = {"pre": pre_b}
    if p.epi == EPI_LSTM:
        H = p.N // 4
        e, gt, c = pre_b[0].view(p.M, H, 4), ref["gates"], ref["c"]
        i, f, g, o = gt.unbind(-1)
        di, df, dg, do = i * (1 - i) * e[..., 0], f * (1 - f) * e[..., 1], (1 - g * g) * e[..., 2], o * (1 - o) * e[..., 3]
        dc = p.c_prev[:, :H].double().abs() * df + g.abs() * di + i * dg
        th = torch.tanh(c)
        allow = ACT_ALLOWANCE + 2 * U * c.abs()
        res.update(gates=torch.stack([di, df, dg, do], -1) + ACT_ALLOWANCE, c=dc + allow, h=th.abs() * do + o * (1 - th * th) * dc + allow)
    else:
        res["out"] = pre_b
    return res


def stats_ref(p, ref, bnd, rows_per_block):
    """per-row-block sums of the reference's rows and their bounds: ([blocks][2][N], [blocks][2][N])"""
    v, e = ref["out"][0], bnd["out"][0]
    want = stats_blocks(v, rows_per_block)
    tol = []
    for vb, eb in zip(v.split(rows_per_block), e.split(rows_per_block)):
        n, a = vb.shape[0], vb.abs() + eb
        tol.append(torch.stack([eb.sum(0) + n * U * a.sum(0), (2 * a * eb + eb * eb + U * a * a).sum(0) + n * U * (a * a).sum(0)]))
    return want, torch.stack(tol)
