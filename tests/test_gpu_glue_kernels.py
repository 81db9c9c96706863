"""-m gpu: the forward / planner glue kernels (index builders, row copies and gathers, masked reductions, planner costs, the sampled
length, image metrics, the parameter re-pack, batch assembly) against plain FLOAT64 (or index-built, bit-exact) references of the
formula include/gcpx.h states, at the edges their model-level tests never reach: lengths 0, 1 and beyond T, leading dimensions with
padding columns, row widths one past a workgroup, non-square frames, skipped frames, counts that are no multiple of the vector width.

Conventions of every test here (those of tests/test_gpu_backward_kernels.py):
  * the kernel is called through video_gcp_amd.runtime with the argument conventions of its call site in the planner (cited);
  * every output starts as NaN (integer outputs: a sentinel): elements the kernel must write are checked finite (and against the
    reference), elements it must leave alone still hold the NaN;
  * a tolerance is stated with its derivation.  eps = 2^-24 (f32 unit roundoff).  "abs-terms" of a quantity = the same expression with
    every term replaced by its absolute value, in float64: a sum of n f32 terms is within n eps x abs-terms of the exact sum
    (the deterministic summation orders here are serial or shallower), a product chain of k roundings within k eps relative.
    "worst" beside a tolerance = the largest error / tolerance measured on an MI355X over the cases of that test."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
NAN = float("nan")
SENT = 1.0e6            # finite sentinel in positions a kernel must not read: one read shows as an error of ~1e6, not as a NaN
ISENT = -77             # sentinel of integer outputs
INVALID_ARG = -1        # GCPX_ERR_INVALID_ARG


@pytest.fixture(scope="module")
def env():
    from video_gcp_amd import runtime as rt
    lib = rt.load_library()
    assert torch.cuda.is_available()
    return rt, lib, torch.device("cuda")


def _st():
    return torch.cuda.current_stream().cuda_stream


def _nan(*shape, dev="cuda"):
    return torch.full(shape, NAN, device=dev)


def _i32(x, dev="cuda"):
    return torch.as_tensor(x, dtype=torch.int32).to(dev)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _within(got, ref, tol, name):
    """|got - ref| <= tol element-wise (tol a tensor or a number); got must be finite.  Returns the worst error / tolerance."""
    got, ref = got.double(), torch.as_tensor(ref).double().to(got.device)
    tol = torch.as_tensor(tol, dtype=torch.float64, device=got.device).expand_as(ref)
    assert bool(torch.isfinite(got).all()), f"{name}: {int((~torch.isfinite(got)).sum())} elements not written (or not finite)"
    err = (got - ref).abs()
    bad = err > tol
    if bool(bad.any()):
        i = int(torch.nonzero(bad.flatten())[0])
        raise AssertionError(f"{name}: {int(bad.sum())}/{bad.numel()} elements outside the bound; first at flat index {i}: got "
                             f"{float(got.flatten()[i])} want {float(ref.flatten()[i])} tol {float(tol.flatten()[i]):.3e}; "
                             f"worst err/tol {float((err / tol.clamp_min(1e-300)).max()):.3g}")
    w = float((err / tol.clamp_min(1e-300)).max())
    print(f"[ratio] {name}: worst err/tol {w:.3g}")
    return w


def _untouched(t, name):
    assert bool(torch.isnan(t).all()), f"{name}: {int((~torch.isnan(t)).sum())} elements written that the kernel must leave alone"


def _same(got, ref, name):
    """bit-exact copies / index arithmetic: every element equal (a NaN left in `got` is an element the kernel did not write)"""
    got, ref = got.cpu(), torch.as_tensor(ref).cpu()
    assert got.shape == ref.shape and got.dtype == ref.dtype, f"{name}: {got.shape} {got.dtype} against {ref.shape} {ref.dtype}"
    bad = ~(got == ref)
    if bool(bad.any()):
        i = int(torch.nonzero(bad.flatten())[0])
        raise AssertionError(f"{name}: {int(bad.sum())}/{bad.numel()} elements differ; first at flat index {i}: got "
                             f"{got.flatten()[i].item()} want {ref.flatten()[i].item()}")


# ------------------------------------------------------------------------------------------------------------------------------
# a. gcpx_rollout_cost: the hand-written planner costs over padded device rollouts
# ------------------------------------------------------------------------------------------------------------------------------
_RC_LENGTHS = [9, 1, 0, 4, 5, 8, 2]      # T = 9, four waves per trip: full (2 trips + 1), one step, empty, exactly one trip, one plus one


def _rollout_cost_ref(x, lengths, goals, T, D, kind, dense, fw):
    """CostFcn arithmetic of the header comment in float64 -> (out [n], abs-terms [n]); x [n][T][>= D], goals [n][D]"""
    out, absum = [], []
    for i, ln in enumerate(lengths):
        L = min(ln, T)
        if L <= 0:
            out.append(0.0)
            absum.append(0.0)
            continue
        xi, g = x[i, :L, :D].double(), goals[i].double()
        if kind in (0, 3):
            steps = (xi - g).pow(2).sum(1).sqrt()
        elif kind == 1:
            nxt = torch.cat([xi[1:], g[None]])
            steps = (nxt - xi).pow(2).sum(1).sqrt()
        else:
            steps = torch.zeros(L, dtype=torch.float64)
            steps[-1] = float(L)
        steps[-1] = steps[-1] * fw
        out.append(float(steps.sum()) if dense else float(steps[-1]))
        absum.append(float(steps.abs().sum()) if dense else float(steps[-1].abs()))
    return torch.tensor(out, dtype=torch.float64), torch.tensor(absum, dtype=torch.float64)


@pytest.mark.parametrize("fw", [1.0, 1.5])
@pytest.mark.parametrize("dense", [0, 1])
@pytest.mark.parametrize("kind", [0, 1, 2, 3])
def test_rollout_cost_matches_float64(env, kind, dense, fw):
    """gcpx_rollout_cost as CostFcn.rollout_cost_device calls it (planning.py:227: x [n][T][ld], D <= ld columns used, int32 lengths,
    out [n]), with per-candidate goals as well (goal_stride != 0).  lengths 9, 1, 0, 4, 5, 8, 2 at T = 9; D = 5 (part of a wavefront),
    64 (one element per lane) and 100 (two trips of the lane loop, the second partial); ld = D + 3 with 1e6 in the padding columns, in
    every row at or past a candidate's length and between the per-candidate goals.  The path length without dense_cost is an argument
    error (cost_fcn.py:52) and writes nothing."""
    rt, lib, dev = env
    n, T = len(_RC_LENGTHS), 9
    worst = 0.0
    for D in (5, 64, 100):
        for per_goal in (False, True):
            g = _gen(100 * kind + 10 * dense + D + int(per_goal))
            ld = D + 3
            x = torch.full((n, T, ld), SENT)
            for i, ln in enumerate(_RC_LENGTHS):
                x[i, :ln, :D] = torch.randn(ln, D, generator=g)
            gs = D + 1 if per_goal else 0
            goals = torch.randn(n if per_goal else 1, D, generator=g)
            gbuf = torch.full((goals.shape[0], D + 1), SENT)
            gbuf[:, :D] = goals
            lengths = _i32(_RC_LENGTHS)
            out = _nan(n + 2)
            xd, gd = x.to(dev), gbuf.to(dev)
            status = lib.gcpx_rollout_cost(xd.data_ptr(), ld, lengths.data_ptr(), gd.data_ptr(), gs, out.data_ptr(), n, T, D, kind, dense,
                                           fw, _st())
            torch.cuda.synchronize()
            if kind == 1 and not dense:
                assert status == INVALID_ARG, status
                _untouched(out, "out after the rejected call")
                continue
            rt.check(status, "rollout_cost")
            ref, absum = _rollout_cost_ref(x, _RC_LENGTHS, goals.expand(n, D), T, D, kind, dense, fw)
            # a step: D f32 squares of a rounded difference, summed over 64 lanes serially (ceil(D / 64) terms) and by a 6-level
            # butterfly, then a correctly rounded sqrt: (D + 3) / 2 + 1 <= D + 2 roundings relative on the step for D >= 1; the
            # one product with final_step_weight fits in that slack for D >= 3.  The steps are then added serially: len eps x
            # abs-terms.  tol = (D + 2 + len) eps x abs-terms.  worst 0.14 (kind 2 is exact: 0).
            lens = torch.tensor([min(max(v, 0), T) for v in _RC_LENGTHS], dtype=torch.float64)
            worst = max(worst, _within(out[:n], ref, (D + 2 + lens) * EPS * absum, f"rollout_cost kind {kind} dense {dense} D {D} gs {gs}"))
            assert float(out[2]) == 0.0, "an empty candidate costs exactly 0"
            _untouched(out[n:], "out past n")
    print(f"[ratio] rollout_cost kind {kind} dense {dense} fw {fw}: {worst:.3g}")


# ------------------------------------------------------------------------------------------------------------------------------
# b. gcpx_seq_pairs / gcpx_masked_row_sum: the learned pairwise cost's operand builder and its masked sum
# ------------------------------------------------------------------------------------------------------------------------------
def _seq_pairs_case(env, lengths, nz, with_goal, seed):
    """lat is allocated with ONE extra row of sentinels behind candidate n-1: a kernel that reads lat[i][T] stays inside the buffer"""
    rt, lib, dev = env
    n, T = len(lengths), 6
    g = _gen(seed)
    lat = torch.randn(n * T + 1, nz, generator=g)
    lat[n * T] = SENT
    goal = torch.randn(n, nz, generator=g) if with_goal else None
    nxt = _nan(n, T, nz)
    latd, goald = lat.to(dev), (goal.to(dev) if with_goal else None)
    rt.check(lib.gcpx_seq_pairs(latd.data_ptr(), _i32(lengths).data_ptr(), rt.ptr(goald), nxt.data_ptr(), n, T, nz, _st()), "seq_pairs")
    torch.cuda.synchronize()
    ref = torch.empty(n, T, nz)
    l3 = lat[:n * T].view(n, T, nz)
    for i, ln in enumerate(lengths):
        L = min(ln, T)                                         # lat has T rows per candidate
        for t in range(T):
            if t + 1 < L:
                ref[i, t] = l3[i, t + 1]
            elif with_goal:
                ref[i, t] = goal[i]
            else:
                ref[i, t] = l3[i, max(L - 1, 0)]             # the sequence's own last latent; row 0 of an empty sequence
    _same(nxt, ref, f"nxt lengths {lengths} nz {nz} goal {with_goal}")


@pytest.mark.parametrize("with_goal", [True, False])
@pytest.mark.parametrize("nz", [4, 512])
def test_seq_pairs_is_bit_exact(env, nz, with_goal):
    """gcpx_seq_pairs as LearnedCostEstimate.sequence_cost_device calls it (planning.py:174: lat [n][T][nz], int32 lengths, goal [n][nz]
    or NULL, nxt [n][T][nz]).  nz = 4 is one float4 per row, nz = 512 loops the 64 threads twice; lengths 6 (= T), 1, 0, 3, 2."""
    _seq_pairs_case(env, [6, 1, 0, 3, 2], nz, with_goal, 7 + nz)


@pytest.mark.parametrize("with_goal", [True, False])
def test_seq_pairs_clamps_a_length_beyond_T(env, with_goal):
    """lengths[i] > T: the length is clamped to T, as gcpx_masked_row_sum and gcpx_rollout_cost clamp it, so the partner of row T-1
    is the goal (goal == NULL: the last latent lat[i][T-1]) and never lat[i][T], which is candidate i+1's first row."""
    _seq_pairs_case(env, [6, 8, 0, 3, 7], 8, with_goal, 21)


def test_masked_row_sum_matches_float64(env):
    """gcpx_masked_row_sum as planning.py:178 calls it (vals [n][T], int32 lengths, out [n]).  n = 65 is one more than a workgroup;
    lengths cycle through 0, 1, T, T + 1, 40 and -1: the clamp to T and a non-positive length giving exactly 0.  Values of mixed sign
    over four decades; every position at or past the length holds 1e6."""
    rt, lib, dev = env
    n, T = 65, 11
    g = _gen(5)
    lengths = [(0, 1, 11, 12, 40, -1)[i % 6] for i in range(n)]
    vals = torch.randn(n, T, generator=g) * 10.0 ** torch.randint(-2, 3, (n, T), generator=g).float()
    ref, absum, lens = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for i, ln in enumerate(lengths):
        L = max(min(ln, T), 0)
        vals[i, L:] = SENT
        ref[i], absum[i], lens[i] = vals[i, :L].double().sum(), vals[i, :L].double().abs().sum(), L
    out = _nan(n + 3)
    vd = vals.to(dev)
    rt.check(lib.gcpx_masked_row_sum(vd.data_ptr(), _i32(lengths).data_ptr(), out.data_ptr(), n, T, _st()), "masked_row_sum")
    torch.cuda.synchronize()
    # a serial f32 sum of len terms: len eps x abs-terms.  worst 0.17
    _within(out[:n], ref, lens * EPS * absum, "masked_row_sum")
    assert bool((out[:n][lens.to(dev) == 0] == 0).all()), "a non-positive length sums to exactly 0"
    _untouched(out[n:], "out past n")


# ------------------------------------------------------------------------------------------------------------------------------
# c. row movers: gcpx_gather_rows_rest / gcpx_gather_rows, gcpx_copy_rows, gcpx_fill_zero
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx_offset", [0, 1])
@pytest.mark.parametrize("row_floats", [4, 1028])
def test_gather_rows_rest_is_bit_exact(env, row_floats, idx_offset):
    """gcpx_gather_rows_rest as the forward plan gathers what the output head has not stored (forward_plan.py:660, :670: src [B][N] rows,
    idx [B][T], out [B][T] rows, written [B*T]) and gcpx_gather_rows (forward_plan.py:664; idx_offset 1: forward_plan.py:454).
    row_floats = 1028 is 257 float4, one past the 256 threads.  Rows with written >= 0 keep their NaN, rows with a negative idx are
    zeros, the others are copies; gcpx_gather_rows is the same reference with nothing written."""
    rt, lib, dev = env
    B, T, N = 3, 5, 7
    g = _gen(11 + row_floats + idx_offset)
    src = torch.randn(B, N, row_floats, generator=g)
    idx = torch.randint(-2, N - idx_offset, (B, T), generator=g).clamp_min(-1)
    idx[0, 0], idx[1, 2], idx[2, 4] = -1, N - 1 - idx_offset, 0
    written = torch.where(torch.rand(B * T, generator=g) < 0.4, torch.arange(B * T), torch.full((B * T,), -1))
    written[0], written[1], written[B * T - 1] = -1, 0, -1
    assert bool((idx < 0).any()) and bool((idx >= 0).any()) and bool((written >= 0).any())
    ref = torch.zeros(B, T, row_floats)
    for b in range(B):
        for t in range(T):
            if idx[b, t] >= 0:
                ref[b, t] = src[b, idx[b, t] + idx_offset]
    srcd, idxd, wd = src.to(dev), _i32(idx), _i32(written)
    out = _nan(B * T, row_floats)
    rt.check(lib.gcpx_gather_rows_rest(srcd.data_ptr(), idxd.data_ptr(), out.data_ptr(), B, T, N, idx_offset, row_floats, wd.data_ptr(),
                                       _st()), "gather_rows_rest")
    full = _nan(B * T, row_floats)
    rt.check(lib.gcpx_gather_rows(srcd.data_ptr(), idxd.data_ptr(), full.data_ptr(), B, T, N, idx_offset, row_floats, _st()), "gather_rows")
    torch.cuda.synchronize()
    keep = written >= 0
    _untouched(out[keep.to(dev)], "rows their producer has written")
    _same(out[(~keep).to(dev)], ref.view(B * T, row_floats)[~keep], "gather_rows_rest")
    _same(full, ref.view(B * T, row_floats), "gather_rows (= gather_rows_rest with nothing written)")


@pytest.mark.parametrize("row_floats", [4, 1028])
def test_copy_rows_is_bit_exact(env, row_floats):
    """gcpx_copy_rows in its call-site forms: images = cat(I_0, decoded) of the sequential model (sequential.py:514-515: one row per
    sequence, then T - 1 rows at a row offset, into a T-row destination) and the slice out of a much wider source of
    backward_plan.py:309-310 (src_batch_rows = PS >> dst_batch_rows = 2).  Destination rows outside a copy keep their NaN."""
    rt, lib, dev = env
    B, T, rf = 3, 5, row_floats
    g = _gen(17 + rf)
    i0, dec = torch.randn(B, 1, rf, generator=g), torch.randn(B, T - 1, rf, generator=g)
    i0d, decd = i0.to(dev), dec.to(dev)
    images = _nan(B, T, rf)
    rt.check(lib.gcpx_copy_rows(i0d.data_ptr(), images.data_ptr(), B, 1, rf, 1, T, _st()), "copy_rows")
    torch.cuda.synchronize()
    _same(images[:, :1], i0, "cat.I0")
    _untouched(images[:, 1:], "rows 1.. after cat.I0")
    images2 = _nan(B, T, rf)
    rt.check(lib.gcpx_copy_rows(decd.data_ptr(), images2.data_ptr() + 4 * rf, B, T - 1, rf, T - 1, T, _st()), "copy_rows")
    torch.cuda.synchronize()
    _same(images2[:, 1:], dec, "cat.dec")
    _untouched(images2[:, 0], "row 0 after cat.dec")
    PS, at = 33, 16
    hid = torch.randn(B, PS, rf, generator=g)
    hidd = hid.to(dev)
    dinit = _nan(B, 2, rf)
    rt.check(lib.gcpx_copy_rows(hidd.data_ptr() + 4 * at * rf, dinit.data_ptr() + 4 * rf, B, 1, rf, PS, 2, _st()), "copy_rows")
    torch.cuda.synchronize()
    _same(dinit[:, 1], hid[:, at], "bw.dinit.r")
    _untouched(dinit[:, 0], "row 0 after bw.dinit.r")
    rt.check(lib.gcpx_copy_rows(hidd.data_ptr(), dinit.data_ptr(), B, 1, rf, PS, 2, _st()), "copy_rows")
    torch.cuda.synchronize()
    _same(dinit, torch.stack([hid[:, 0], hid[:, at]], 1), "bw.dinit.l + bw.dinit.r")


@pytest.mark.parametrize("nbytes", [1, 6, 4096 + 3])
def test_fill_zero_touches_only_its_range(env, nbytes):
    """gcpx_fill_zero (sequential.py:261, backward_plan.py:39: pointer + byte count) on a 0xFF buffer at a start offset of 16 bytes"""
    rt, lib, dev = env
    buf = torch.full((16 + nbytes + 16,), 0xFF, dtype=torch.uint8, device=dev)
    rt.check(lib.gcpx_fill_zero(buf.data_ptr() + 16, nbytes, _st()), "fill_zero")
    torch.cuda.synchronize()
    assert bool((buf[16:16 + nbytes] == 0).all())
    assert bool((buf[:16] == 0xFF).all()) and bool((buf[16 + nbytes:] == 0xFF).all()), "bytes outside the range changed"


# ------------------------------------------------------------------------------------------------------------------------------
# d. index builders: gcpx_seq_index, gcpx_aux_index_rows
# ------------------------------------------------------------------------------------------------------------------------------
def test_seq_index_is_bit_exact(env):
    """gcpx_seq_index (sequential.py:205, forward_plan.py:646: int64 end_ind [B] -> int32 idx [B][T], seq_len [B]).  B T = 259 is one past
    a workgroup; end_ind 0, 1, T - 1 and T + 2 (a whole row selected)."""
    rt, lib, dev = env
    B, T = 37, 7
    end = torch.tensor([(0, 1, T - 1, T + 2)[b % 4] for b in range(B)], dtype=torch.int64)
    idx = torch.full((B * T + 5,), ISENT, dtype=torch.int32, device=dev)
    sl = torch.full((B + 5,), ISENT, dtype=torch.int32, device=dev)
    endd = end.to(dev)
    rt.check(lib.gcpx_seq_index(endd.data_ptr(), B, T, idx.data_ptr(), sl.data_ptr(), _st()), "seq_index")
    torch.cuda.synchronize()
    t = torch.arange(T)[None, :].expand(B, T)
    ref = torch.where(t <= end[:, None], t, torch.full_like(t, -1)).to(torch.int32)
    _same(idx[:B * T].view(B, T), ref, "idx")
    _same(sl[:B], (end + 1).to(torch.int32), "seq_len")
    assert bool((idx[B * T:] == ISENT).all()) and bool((sl[B:] == ISENT).all())


def test_aux_index_rows_is_bit_exact(env):
    """gcpx_aux_index_rows (forward_plan.py:473, sequential.py:453: four int64 [B] -> int32 rows [4][B]) with T != Wd, so a swapped stride
    shows; B = 70 is more than a workgroup of 64; the first sequences sit at the extremes t0 = 0, t1 = end, start = 0, end = Wd - 1."""
    rt, lib, dev = env
    B, T, Wd = 70, 9, 15
    g = _gen(23)
    t0 = torch.randint(0, T, (B,), generator=g)
    t1, cs, ce = (torch.randint(0, Wd, (B,), generator=g) for _ in range(3))
    t0[:4], t1[:4], cs[:4], ce[:4] = 0, Wd - 1, 0, Wd - 1
    t0[4], t1[B - 1], cs[5], ce[B - 1] = T - 1, Wd - 1, Wd - 2, Wd - 1
    rows = torch.full((4 * B + 3,), ISENT, dtype=torch.int32, device=dev)
    d = [v.to(dev) for v in (t0, t1, cs, ce)]
    rt.check(lib.gcpx_aux_index_rows(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), B, T, Wd, rows.data_ptr(), _st()),
             "aux_index_rows")
    torch.cuda.synchronize()
    b = torch.arange(B)
    ref = torch.stack([b * T + t0, b * Wd + t1, b * Wd + cs, b * Wd + ce]).to(torch.int32)
    _same(rows[:4 * B].view(4, B), ref, "rows")
    assert bool((rows[4 * B:] == ISENT).all())


# ------------------------------------------------------------------------------------------------------------------------------
# e. gcpx_bn_fold, gcpx_gauss_nll
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cn", [1, 65, 100])
def test_bn_fold_matches_float64(env, Cn):
    """gcpx_bn_fold (plan_ops.py:340: running_mean, running_var, gamma, beta [C], eps -> scale, shift [C]).  running_var holds 0 and
    1e-12, where eps is the whole denominator; gamma holds 0 and negatives; running_mean sits around 1e3, so shift = beta - mean scale
    is a difference of a small and a large number."""
    rt, lib, dev = env
    g = _gen(31 + Cn)
    eps_bn = 1e-5
    rm = 1e3 + 10 * torch.randn(Cn, generator=g)
    rv = torch.randn(Cn, generator=g).abs()
    gamma, beta = torch.randn(Cn, generator=g), torch.randn(Cn, generator=g)
    rv[0], gamma[0] = 0.0, -1.3
    if Cn > 1:
        rv[1], gamma[2], rv[64] = 1e-12, 0.0, 0.0
    scale, shift = _nan(Cn + 3), _nan(Cn + 3)
    d = [v.to(dev) for v in (rm, rv, gamma, beta)]
    rt.check(lib.gcpx_bn_fold(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), eps_bn, Cn, scale.data_ptr(),
                              shift.data_ptr(), _st()), "bn_fold")
    torch.cuda.synchronize()
    e32 = float(np.float32(eps_bn))                             # the argument is a float
    sc = gamma.double() / torch.sqrt(rv.double() + e32)
    sh = beta.double() - rm.double() * sc
    # scale: one add, one sqrt (which halves the add's error), one divide, each correctly rounded: within 3 eps relative.
    # worst 0.48
    _within(scale[:Cn], sc, 3 * EPS * sc.abs(), "scale")
    # shift: scale's error (2.5 eps at most: 0.5 + 1 + 1) times |mean|, then the multiply-add: within 3 eps x (|beta| + |mean scale|)
    # when the compiler fuses it, as it does here.  worst 0.74: with |mean scale| ~ 1e3 |beta| the bound is scale's bound plus half a
    # rounding, so 166 channels come close to it; a wider bound would have to assume roundings the kernel does not perform
    _within(shift[:Cn], sh, 3 * EPS * (beta.double().abs() + (rm.double() * sc).abs()), "shift")
    _untouched(scale[Cn:], "scale past C")
    _untouched(shift[Cn:], "shift past C")


@pytest.mark.parametrize("log_sigma", [0.0, -3.0, 2.0])
@pytest.mark.parametrize("nelem", [100, 256, 3 * 32 * 32 + 4])
def test_gauss_nll_matches_float64(env, nelem, log_sigma):
    """gcpx_gauss_nll (forward_plan.py:709, sequential.py:539: mu, target [rows][nelem], one log_sigma, nll_out [rows]):
    nll[row] = sum of 0.5 ((x - mu) / sigma)^2 + log_sigma + 0.5 log(2 pi).  nelem = 100 leaves 156 threads idle, 256 is one element
    per thread, 3076 is 12 trips and a partial one; row 1 has target == mu exactly, so its value is nelem (log_sigma + 0.5 log 2 pi)."""
    rt, lib, dev = env
    rows = 3
    g = _gen(41 + nelem)
    mu = torch.rand(rows, nelem, generator=g) * 2 - 1
    tgt = (mu + 0.3 * torch.randn(rows, nelem, generator=g)).clamp(-1, 1)
    tgt[1] = mu[1]
    ls = torch.tensor([log_sigma])
    out = _nan(rows + 2)
    mud, tgtd, lsd = mu.to(dev), tgt.to(dev), ls.to(dev)
    rt.check(lib.gcpx_gauss_nll(mud.data_ptr(), tgtd.data_ptr(), lsd.data_ptr(), out.data_ptr(), rows, nelem, _st()), "gauss_nll")
    torch.cuda.synchronize()
    q = 0.5 * ((tgt.double() - mu.double()) * math.exp(-log_sigma)) ** 2
    c = 0.5 * math.log(2 * math.pi)
    ref = (q + log_sigma + c).sum(1)
    absum = (q + abs(log_sigma) + c).sum(1)
    # per element: expf(-ls) within 1 ulp = 2 eps (the documented bound of HIP's expf), the difference and its product with it 2 more:
    # 4 eps on d, 8 + 1 on d^2 (the 0.5 is exact): 9 eps on the quadratic term; the two additions and the rounded constant: 3 eps of
    # the element's abs-terms: k = 12.  Each thread adds nelem / 256 elements serially, the workgroup's tree has 8 levels.
    # tol = (nelem / 256 + 8 + 12) eps x abs-terms.  worst 0.078 (with k = 12; 0.02 at the least)
    _within(out[:rows], ref, (nelem / 256 + 8 + 12) * EPS * absum, f"gauss_nll nelem {nelem} log_sigma {log_sigma}")
    _untouched(out[rows:], "nll_out past rows")


# ------------------------------------------------------------------------------------------------------------------------------
# f. gcpx_path_cost: the cost model's ground-truth path length
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,row_len", [(7, 5), (12, 64), (300, 100)])
def test_path_cost_matches_float64(env, rows, row_len):
    """gcpx_path_cost (forward_plan.py:293, sequential.py:221: x [B][T][rows][row_len], int64 start / end [B], partial [B][rows], out [B])
    against oracle.aux_models_oracle.euclidean_path_cost's formula in float64.  rows = 7 leaves one wavefront of the second workgroup
    idle and row_len = 5 most of a wavefront; (12, 64) is one element per lane; (300, 100) makes two trips of the lane loop and of the
    finish kernel's loop.  Segments: the whole sequence, one step, the last step, and start == end (exactly 0).  Frames outside
    [start, end] hold 1e6."""
    from oracle import aux_models_oracle as AO
    rt, lib, dev = env
    B, T = 4, 6
    seg = [(0, T - 1), (2, 3), (T - 2, T - 1), (3, 3)]
    g = _gen(51 + rows)
    x = torch.full((B, T, rows, row_len), SENT)
    for b, (s, e) in enumerate(seg):
        x[b, s:e + 1] = torch.randn(e + 1 - s, rows, row_len, generator=g)
    s_idx = torch.tensor([s for s, _ in seg], dtype=torch.int64)
    e_idx = torch.tensor([e for _, e in seg], dtype=torch.int64)
    partial, out = _nan(B * rows + 3), _nan(B + 3)
    xd, sd, ed = x.to(dev), s_idx.to(dev), e_idx.to(dev)
    rt.check(lib.gcpx_path_cost(xd.data_ptr(), sd.data_ptr(), ed.data_ptr(), B, T, rows, row_len, partial.data_ptr(), out.data_ptr(), _st()),
             "path_cost")
    torch.cuda.synchronize()
    ref_p, tol_p = torch.zeros(B, rows, dtype=torch.float64), torch.zeros(B, rows, dtype=torch.float64)
    for b, (s, e) in enumerate(seg):
        steps = (x[b, s + 1:e + 1].double() - x[b, s:e].double()).pow(2).sum(-1).sqrt()       # [e - s][rows]
        ref_p[b] = steps.sum(0)
        # a step: row_len fused multiply-adds of a rounded difference, a 6-level butterfly, a sqrt: (row_len + 2) eps relative (as
        # for gcpx_rollout_cost); the e - s steps of a row are added serially: (e - s) eps x abs-terms (the steps are not negative)
        tol_p[b] = (row_len + 2 + (e - s)) * EPS * ref_p[b]
    ref = ref_p.sum(1)
    oracle = torch.from_numpy(AO.euclidean_path_cost(x.numpy(), s_idx.numpy(), e_idx.numpy()))[:, 0].double()
    assert bool(((oracle - ref).abs() <= 1e-4 * ref).all()), "the float64 restatement left the oracle's formula"
    # worst 0.16 for partial, 0.017 for out (whose bound adds up the partials' worst cases, all taken with one sign)
    _within(partial[:B * rows].view(B, rows), ref_p, tol_p, f"partial rows {rows} row_len {row_len}")
    # the finish: rows / 256 serial additions per thread and an 8-level tree: (rows / 256 + 8) eps x abs-terms, on top of the partials'
    _within(out[:B], ref, tol_p.sum(1) + (rows / 256 + 8) * EPS * ref, f"out rows {rows} row_len {row_len}")
    assert float(out[3]) == 0.0 and bool((partial[3 * rows:4 * rows] == 0).all()), "start == end costs exactly 0"
    _untouched(partial[B * rows:], "partial past B rows")
    _untouched(out[B:], "out past B")


# ------------------------------------------------------------------------------------------------------------------------------
# g. gcpx_sample_length: inverse CDF of softmax(logits) at a fed uniform number
# ------------------------------------------------------------------------------------------------------------------------------
def _sample_length_ref(logits, u, min_len):
    """oracle.aux_models_oracle.sample_length with the clamp's lower bound as an argument (the oracle's is the call site's 2)"""
    from oracle import aux_models_oracle as AO
    p = torch.softmax(torch.as_tensor(logits).double(), dim=1)
    cdf = torch.cumsum(p, dim=1)
    idx = (cdf <= torch.as_tensor(u).double()[:, None]).sum(1).clamp(max=p.shape[1] - 1)
    ref = torch.clamp(idx, min=min_len)
    if min_len == 2:
        assert torch.equal(ref, AO.sample_length(logits, u))
    return ref


def _sample_length(env, logits, u, min_len):
    rt, lib, dev = env
    B, T = logits.shape
    end = torch.full((B + 3,), ISENT, dtype=torch.int64, device=dev)
    ld, ud = logits.to(dev), u.to(dev)
    # forward_plan.py:318: logits [B][T], u [B], min_len, int64 end_ind [B]
    rt.check(lib.gcpx_sample_length(ld.data_ptr(), ud.data_ptr(), B, T, min_len, end.data_ptr(), _st()), "sample_length")
    torch.cuda.synchronize()
    assert bool((end[B:] == ISENT).all())
    return end[:B].cpu()


def _midpoint_draws(logits):
    """sequence b draws the midpoint of the b-th interval of its own float64 CDF, rounded to f32; every interval must be wide enough
    (2^-20) that neither that rounding (2^-25) nor the kernel's own float64 sums (1e-15) can move the draw across an edge"""
    cdf = torch.cumsum(torch.softmax(logits.double(), dim=1), dim=1)
    lo = torch.cat([torch.zeros(cdf.shape[0], 1, dtype=torch.float64), cdf[:, :-1]], 1)
    hi = cdf.clone()
    hi[:, -1] = 1.0
    assert float((hi - lo).diagonal().min()) >= 2.0 ** -20, "an interval too narrow for an f32 midpoint: no case may be left out"
    return ((lo + hi) / 2).diagonal().float()


@pytest.mark.parametrize("min_len", [0, 2])
@pytest.mark.parametrize("T", [4, 65, 130])
def test_sample_length_hits_every_interval(env, T, min_len):
    """B = T sequences of unit-scale logits, sequence b drawing the middle of its b-th CDF interval: every index is produced once
    (T = 4, 65, 130: one, two and three trips of the lane loops), and min_len lifts the first ones."""
    logits = torch.randn(T, T, generator=_gen(61 + T))
    u = _midpoint_draws(logits)
    ref = _sample_length_ref(logits, u, min_len)
    assert torch.equal(ref, torch.arange(T).clamp(min=min_len))
    _same(_sample_length(env, logits, u, min_len), ref, f"end_ind T {T} min_len {min_len}")


def test_sample_length_exact_edges(env):
    """Draws that need no margin.  Four equal logits: the CDF is 0.25, 0.5, 0.75, 1 exactly, and a draw ON an edge belongs to the
    interval above it (cdf <= u counts the edge), which tells <= from <.  Logits shifted by 1e4: exp overflows without the subtraction
    of the maximum.  One logit 60 above the rest, first, in the middle and last: all the mass in one interval."""
    u5 = torch.tensor([0.0, 0.25, 0.5, 0.75, 0.99999994])
    logits = torch.full((5, 4), 0.7)
    ref = _sample_length_ref(logits, u5, 0)
    assert ref.tolist() == [0, 1, 2, 3, 3]
    _same(_sample_length(env, logits, u5, 0), ref, "equal logits")
    T = 65
    shifted = torch.randn(T, T, generator=_gen(67)) + 1e4
    u = _midpoint_draws(shifted)
    ref = _sample_length_ref(shifted, u, 0)
    assert torch.equal(ref, torch.arange(T))
    _same(_sample_length(env, shifted, u, 0), ref, "logits + 1e4")
    for p in (0, 31, T - 1):
        peak = torch.randn(3, T, generator=_gen(68 + p))
        peak[:, p] = peak.max() + 60.0
        u3 = torch.tensor([0.0, 0.5, 0.99999994])
        ref = _sample_length_ref(peak, u3, 0)
        assert ref.tolist() == [0, p, p]
        _same(_sample_length(env, peak, u3, 0), ref, f"peak at {p}")


# ------------------------------------------------------------------------------------------------------------------------------
# h. gcpx_image_metrics
# ------------------------------------------------------------------------------------------------------------------------------
def _ssim_bound(g01, t01):
    """First-order bound on the error of the mean SSIM of planes g01, t01 [P][H][W] (float64, [0, 1]) -> [P], from the kernel's
    arithmetic: a plane is rescaled in f32 (1 rounding per pixel), the five window sums are 49-term serial f32 sums (fused
    multiply-adds for the products: 49 roundings), everything after them is float64.  With r = 52 eps for those roundings:
      d mean_x = r mean_x;   d var_x = cn r (E[x^2] + 2 mean_x^2);   d cov = cn r (E[|x y|] + 2 mean_x mean_y)    (cn = 49 / 48)
    pushed through S = N1 N2 / (D1 D2), N1 = 2 mx my + C1, N2 = 2 cov + C2, D1 = mx^2 + my^2 + C1, D2 = vx + vy + C2:
      dS <= |S| (dN1 / N1 + dD1 / D1 + dD2 / D2) + N1 dN2 / (D1 D2)."""
    r = 52 * EPS
    cn = 49.0 / 48.0
    box = lambda v: F.avg_pool2d(v[:, None], 7, stride=1)[:, 0]
    mx, my = box(g01), box(t01)
    exx, eyy, exy = box(g01 * g01), box(t01 * t01), box(g01 * t01)
    vx, vy, cov = cn * (exx - mx * mx), cn * (eyy - my * my), cn * (exy - mx * my)
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    N1, N2, D1, D2 = 2 * mx * my + C1, 2 * cov + C2, mx * mx + my * my + C1, vx + vy + C2
    S = N1 * N2 / (D1 * D2)
    dN1 = 4 * r * mx * my
    dD1 = 2 * r * (mx * mx + my * my)
    dN2 = 2 * cn * r * (exy + 2 * mx * my)
    dD2 = cn * r * (exx + 2 * mx * mx + eyy + 2 * my * my)
    dS = S.abs() * (dN1 / N1 + dD1 / D1 + dD2 / D2) + N1 * dN2 / (D1 * D2)
    return dS.mean((1, 2))


def _check_metrics(got, gen, tgt, name):
    """one sequence: got [3] against oracle.metrics_oracle.sequence_metrics(gen, tgt) (gen, tgt [n][C][H][W] in [-1, 1])"""
    from oracle import metrics_oracle as MO
    mse, psnr, ssim = MO.sequence_metrics(gen.numpy(), tgt.numpy())
    n, Cc, H, W = gen.shape
    # mse: accumulated in double from f32 differences, stored as f32: 1e-6 relative.  worst 0.04 (the f32 store alone is 0.06 at most)
    w0 = _within(got[0:1], torch.tensor([mse], dtype=torch.float64), 1e-6 * mse, name + " mse")
    # psnr = mean of 10 log10(1 / mse_frame): the frame's sum of squares carries 2 eps relative (the rounded difference, squared in
    # double), the logarithm turns that into 10 / ln 10 x 2 eps absolute (3 allowed for the double arithmetic behind it); the f32
    # store adds eps |psnr|.  worst 0.43
    w1 = _within(got[1:2], torch.tensor([psnr], dtype=torch.float64), 10 / math.log(10) * 3 * EPS + EPS * abs(psnr), name + " psnr")
    # ssim: _ssim_bound per plane, averaged like the metric, plus the f32 store.  worst 0.009.  The bound lines up, with one sign, the
    # 52 roundings of every window sum in every window of every plane, while the metric averages hundreds of windows whose errors have
    # both signs; it is still the bound that follows from the arithmetic, and it is tight enough to tell the sample covariance from
    # the population covariance on the low-contrast sequence (an error of 28 x the bound)
    tol = float(_ssim_bound((gen.double().reshape(n * Cc, H, W) + 1) / 2, (tgt.double().reshape(n * Cc, H, W) + 1) / 2).mean())
    w2 = _within(got[2:3], torch.tensor([ssim], dtype=torch.float64), tol + EPS * abs(ssim), name + " ssim")
    return w0, w1, w2


def _metrics_inputs(H, W, Cc, seed):
    """B = 5 sequences of T = 4 frames: 0 noisy estimates of random targets; 1 estimate == target; 2 a constant bright plane (0.9 on
    the [0, 1] scale) against a slightly noisy bright target — var = E[x^2] - mean^2 cancels worst there; 3 scored over an empty range;
    4 two dim planes of low contrast (variance 4e-4, about C2 / 2), where the window sums are small, the bound is tight and the sample
    covariance factor 49 / 48 moves the result by 1 % (on textured frames it cancels between numerator and denominator)"""
    g = _gen(seed)
    B, T = 5, 4
    tgt = torch.rand(B, T, Cc, H, W, generator=g) * 2 - 1
    est = (tgt + 0.2 * torch.randn(B, T, Cc, H, W, generator=g)).clamp(-1, 1)
    est[1] = tgt[1]
    est[2] = 0.8
    tgt[2] = (0.8 + 0.02 * torch.randn(T, Cc, H, W, generator=g)).clamp(-1, 1)
    est[4] = -0.8 + 0.04 * torch.randn(T, Cc, H, W, generator=g)
    tgt[4] = -0.8 + 0.04 * torch.randn(T, Cc, H, W, generator=g)
    first = torch.tensor([0, 0, 1, 2, 0], dtype=torch.int32)
    last = torch.tensor([T, T, T, 2, T], dtype=torch.int32)
    return tgt, est, first, last


def _image_metrics(env, pool, tgt, fmap, first, last):
    """evaluation.py:211: est pool [R][C][H][W], tgt [B][T][C][H][W], int32 frame_map [B][T] or NULL, int32 first / last [B], a scratch
    of 2 B T C doubles, out [B][3]"""
    rt, lib, dev = env
    B, T, Cc, H, W = tgt.shape
    scratch = torch.full((2 * B * T * Cc,), NAN, dtype=torch.float64, device=dev)
    out = _nan(B * 3 + 3)
    pd, td, fd, ld = pool.to(dev), tgt.to(dev), first.to(dev), last.to(dev)
    md = fmap.to(dev) if fmap is not None else None
    rt.check(lib.gcpx_image_metrics(pd.data_ptr(), td.data_ptr(), rt.ptr(md), fd.data_ptr(), ld.data_ptr(), B, T, Cc, H, W,
                                    scratch.data_ptr(), out.data_ptr(), _st()), "image_metrics")
    torch.cuda.synchronize()
    _untouched(out[B * 3:], "out past B")
    return out[:B * 3].view(B, 3).cpu()


@pytest.mark.parametrize("mapped", [False, True])
@pytest.mark.parametrize("Cc", [1, 3])
@pytest.mark.parametrize("H,W", [(7, 7), (7, 12), (12, 7), (16, 16)])
def test_image_metrics_matches_oracle(env, H, W, Cc, mapped):
    """Direct calls at 7 x 7 (one window), both non-square orientations and 16 x 16, one and three channels, with frame_map NULL and
    with the estimates permuted in their pool."""
    tgt, est, first, last = _metrics_inputs(H, W, Cc, 71 + H * W + Cc)
    B, T = tgt.shape[:2]
    pool, fmap = est.reshape(B * T, Cc, H, W), None
    if mapped:
        perm = torch.randperm(B * T, generator=_gen(72))
        pool = pool[perm]                                       # pool[j] = est frame perm[j]: frame f sits at argsort(perm)[f]
        fmap = torch.argsort(perm).to(torch.int32).view(B, T)
    got = _image_metrics(env, pool, tgt, fmap, first, last)
    for b in (0, 2, 4):
        lo, hi = int(first[b]), int(last[b])
        _check_metrics(got[b], est[b, lo:hi], tgt[b, lo:hi], f"{H}x{W} C {Cc} sequence {b}")
    assert float(got[1, 0]) == 0.0 and float(got[1, 1]) == 300.0, got[1]          # estimate == target: psnr of the 1e-30 floor
    assert abs(float(got[1, 2]) - 1.0) <= 1e-6, got[1]
    assert bool(torch.isnan(got[3]).all()), f"first == last must give three NaNs, got {got[3]}"


def test_image_metrics_leaves_skipped_frames_out(env):
    """A negative frame_map entry inside [first, last) is left out of the averages — not counted, in no sum — so the sequence scores
    as the oracle scores its remaining frames; a sequence whose frames are all skipped gives NaN like an empty range."""
    H, W, Cc = 12, 7, 3
    tgt, est, _, _ = _metrics_inputs(H, W, Cc, 79)
    B, T = tgt.shape[:2]
    fmap = torch.arange(B * T, dtype=torch.int32).view(B, T).clone()
    fmap[0, 2] = -1                                             # in the middle of sequence 0's range
    fmap[2, :] = -1                                             # all of sequence 2
    fmap[3, 0] = -3                                             # first frame of a full range
    first = torch.zeros(B, dtype=torch.int32)
    last = torch.full((B,), T, dtype=torch.int32)
    got = _image_metrics(env, est.reshape(B * T, Cc, H, W), tgt, fmap, first, last)
    _check_metrics(got[0], est[0, [0, 1, 3]], tgt[0, [0, 1, 3]], "one skipped frame in the middle")
    _check_metrics(got[3], est[3, 1:], tgt[3, 1:], "the first frame skipped")
    assert float(got[1, 0]) == 0.0 and float(got[1, 1]) == 300.0
    assert bool(torch.isnan(got[2]).all()), f"every frame skipped must give three NaNs, got {got[2]}"


# ------------------------------------------------------------------------------------------------------------------------------
# i. gcpx_repack / gcpx_repack_blocks: the packed-weight arena as a gather of the flat parameter vector
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("two", [False, True])
@pytest.mark.parametrize("max_blocks", [0, 1, 3])
@pytest.mark.parametrize("n", [4, 1024 + 4, 4 * (3 * 256 * 2 + 1), 6, 1024 + 7])
def test_repack_is_a_bit_exact_gather(env, n, max_blocks, two):
    """gcpx_repack (weights.py:354, :356) and gcpx_repack_blocks (weights.py:344): theta, int32 idx0, idx1 or NULL, dst, n [, max_blocks].
    With max_blocks = 1 and 3 the grid-stride loop of the idx1 == NULL path, which keeps two float4 in flight, makes no trip
    (n = 4), one, and several followed by its single tail trip (n = 6148 is 1537 float4: 3 x 256 x 2 + 1); n = 6 and 1031 end in a
    partial float4, which the scalar tail writes (every call site passes a multiple of 4, the kernel does not depend on it).
    Negative indices read as 0; the 8 floats behind dst[n] keep their NaN."""
    rt, lib, dev = env
    g = _gen(83 + n)
    P = 500
    theta = torch.randn(P, generator=g)
    idx0 = torch.randint(-P // 4, P, (n,), generator=g).clamp_min(-1)
    idx1 = torch.randint(-P, P, (n,), generator=g).clamp_min(-1)
    idx0[0], idx0[n - 1] = -1, P - 1
    pad = (-n) % 4                                             # index arrays as the arena keeps them: padded to a float4 with -1
    i0d, i1d = _i32(torch.cat([idx0, torch.full((pad,), -1)])), _i32(torch.cat([idx1, torch.full((pad,), -1)]))
    ref = torch.where(idx0 >= 0, theta[idx0.clamp_min(0)], torch.zeros(n))
    if two:
        ref = ref + torch.where(idx1 >= 0, theta[idx1.clamp_min(0)], torch.zeros(n))        # one f32 addition, as in the kernel
    thd = theta.to(dev)
    dst = _nan(n + 8)
    rt.check(lib.gcpx_repack_blocks(thd.data_ptr(), i0d.data_ptr(), i1d.data_ptr() if two else None, dst.data_ptr(), n, max_blocks, _st()),
             "repack_blocks")
    torch.cuda.synchronize()
    _same(dst[:n], ref, f"repack_blocks n {n} max_blocks {max_blocks} two {two}")
    _untouched(dst[n:], "dst past n")
    if max_blocks == 0:
        dst2 = _nan(n + 8)
        rt.check(lib.gcpx_repack(thd.data_ptr(), i0d.data_ptr(), i1d.data_ptr() if two else None, dst2.data_ptr(), n, _st()), "repack")
        torch.cuda.synchronize()
        _same(dst2[:n], ref, f"repack n {n} two {two}")
        _untouched(dst2[n:], "dst past n")


# ------------------------------------------------------------------------------------------------------------------------------
# j. gcpx_assemble_batch: one uploaded batch into the model's inputs
# ------------------------------------------------------------------------------------------------------------------------------
def test_assemble_batch_direct_call_is_bit_exact(env):
    """gcpx_assemble_batch (dataset.py:496) at the smallest shapes of tests/test_gpu_dataset.py (T = 8, 8 x 8 frames, 2 states, 2
    actions) against the loader arithmetic of the header: output frame t reads window frame s = min(t + chop, T - 1) when
    t < zero_from and s < n_frames, else uint8 0; states standardised with a correctly rounded subtraction and division; actions with
    T - 1 steps.  Sequences: a full recording, one that ends after 5 frames, a chopped one that repeats nothing past zero_from."""
    rt, lib, dev = env
    B, T, H, W, S, A = 3, 8, 8, 8, 2, 2
    r = np.random.RandomState(91)
    frames = r.randint(0, 256, (B, T, H, W, 3)).astype(np.uint8)
    pad_in = (r.rand(B, T) < 0.7).astype(np.float32)
    st_in, ac_in = r.randn(B, T, S).astype(np.float32), r.randn(B, T - 1, A).astype(np.float32)
    mean, den = np.array([0.3, -1.2], np.float32), np.array([1.5, 0.25], np.float32)
    # n_frames, n_states, n_actions, chop, zero_from, end_ind, 0, 0
    info = np.array([[8, 8, 7, 0, 8, 7, 0, 0], [5, 5, 4, 0, 8, 4, 0, 0], [8, 8, 7, 2, 4, 3, 0, 0]], np.int32)
    lut = np.arange(256, dtype=np.uint8).astype(np.float32) / 255 * 2 - 1
    traj = np.empty((B, T, 3, H, W), np.float32)
    states, actions = np.empty((B, T, S), np.float32), np.empty((B, T - 1, A), np.float32)
    for b in range(B):
        nf, ns, na, chop, zf, _ = info[b, :6]
        for t in range(T):
            s = min(t + chop, T - 1)
            px = frames[b, s] if (t < zf and s < nf) else np.zeros((H, W, 3), np.uint8)
            traj[b, t] = lut[px].transpose(2, 0, 1)
            x = st_in[b, s] if (t < zf and s < ns) else np.zeros(S, np.float32)
            states[b, t] = (x - mean) / den
            if t < T - 1:
                sa = min(t + chop, T - 2)
                actions[b, t] = ac_in[b, sa] if (t < zf and sa < na) else 0.0
    up = lambda a: torch.from_numpy(a).to(dev)
    out = dict(traj=_nan(B, T, 3, H, W), I0=_nan(B, 3, H, W), Ig=_nan(B, 3, H, W), pad=_nan(B, T), st=_nan(B, T, S), ac=_nan(B, T - 1, A),
               end=torch.full((B,), ISENT, dtype=torch.int64, device=dev), start=torch.full((B,), ISENT, dtype=torch.int64, device=dev))
    d = dict(frames=up(frames), info=up(info), lut=up(lut), pad=up(pad_in), st=up(st_in), ac=up(ac_in), mean=up(mean), den=up(den))
    rt.check(lib.gcpx_assemble_batch(d["frames"].data_ptr(), d["info"].data_ptr(), d["lut"].data_ptr(), d["pad"].data_ptr(),
                                     d["st"].data_ptr(), d["ac"].data_ptr(), d["mean"].data_ptr(), d["den"].data_ptr(), B, T, H, W, S, A,
                                     out["traj"].data_ptr(), out["I0"].data_ptr(), out["Ig"].data_ptr(), out["pad"].data_ptr(),
                                     out["end"].data_ptr(), out["start"].data_ptr(), out["st"].data_ptr(), out["ac"].data_ptr(), _st()),
             "assemble_batch")
    torch.cuda.synchronize()
    _same(out["traj"], torch.from_numpy(traj), "traj_seq")
    _same(out["I0"], torch.from_numpy(traj[:, 0]), "I_0")
    _same(out["Ig"], torch.from_numpy(traj[np.arange(B), info[:, 5]]), "I_g")
    _same(out["pad"], torch.from_numpy(pad_in), "pad_mask")
    _same(out["st"], torch.from_numpy(states), "states")
    _same(out["ac"], torch.from_numpy(actions), "actions")
    _same(out["end"], torch.from_numpy(info[:, 5].astype(np.int64)), "end_ind")
    _same(out["start"], torch.zeros(B, dtype=torch.int64), "start_ind")
    assert bool((out["traj"][1, 5:] == -1.0).all()), "frames past the recording are uint8 0 = -1.0"
