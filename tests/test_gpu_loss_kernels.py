"""-m gpu: the loss, KL and BatchNorm-statistics kernels (csrc/loss.hip: gcpx_kl_gauss, gcpx_loss_combine, gcpx_loss_pre, gcpx_loss_final;
csrc/misc.hip: gcpx_bn_finalize) against the FLOAT64 references of tests/loss_refs.py, at the shapes where their loops wrap and with
the arguments their model-level tests never set: node weights with a batch stride, a state_mask, a KL weight in device memory, NULL
optional terms, weights <= 0, a partial table with replicas, padding columns and thousands of rows.

Conventions of every test here (those of tests/test_gpu_glue_kernels.py):
  * the kernel is called through video_gcp_amd.runtime with the argument conventions of its call site in the forward (cited);
  * every output starts as NaN: elements the kernel must write are checked finite (and against the reference), elements it must leave
    alone still hold the NaN (out[9..15] of the loss kernels, kl_out past B, scale past C);
  * every position a kernel must not read holds the finite sentinel SENT = 1e6 (gap rows and columns of the latent buffers, the weight
    of frame 0, states beyond max(seq_len), action rows other than inv_t0[b]); reconstruction rows of weight 0 hold values of 1e4 size;
  * a tolerance is stated with its derivation — in tests/loss_refs.py, beside the reference it belongs to (kl_tol, loss_tol,
    bn_finalize), from counted f32 roundings and abs-terms, nothing measured; tests/test_loss_refs_cpu.py shows that a float32
    restatement meets every bound on these inputs and that fourteen planted mistakes do not;
  * "worst" in a docstring = the largest error / tolerance measured on an MI355X over the cases of that test."""
import ctypes as C

import pytest
import torch

import loss_refs as R
from loss_refs import NAN, SENT

pytestmark = pytest.mark.gpu


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


def _within(got, ref, tol, name):
    """|got - ref| <= tol element-wise (tol a tensor or a number); got must be finite.  Returns the worst error / tolerance."""
    got, ref = got.double().cpu(), torch.as_tensor(ref).double().cpu()
    tol = torch.as_tensor(tol, dtype=torch.float64).cpu().expand_as(ref)
    assert got.shape == ref.shape, f"{name}: {tuple(got.shape)} against {tuple(ref.shape)}"
    assert bool(torch.isfinite(got).all()), f"{name}: {int((~torch.isfinite(got)).sum())} elements not written (or not finite)"
    err = (got - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / tol.clamp_min(1e-300))
    bad = err > tol
    if bool(bad.any()):
        i = int(torch.nonzero(bad.flatten())[0])
        raise AssertionError(f"{name}: {int(bad.sum())}/{bad.numel()} elements outside the bound; first at flat index {i}: got "
                             f"{float(got.flatten()[i])} want {float(ref.flatten()[i])} tol {float(tol.flatten()[i]):.3e}; "
                             f"worst err/tol {float(ratio.max()):.3g}")
    w = float(ratio.max())
    print(f"[ratio] {name}: worst err/tol {w:.3g}")
    return w


def _untouched(t, name):
    assert bool(torch.isnan(t).all()), f"{name}: {int((~torch.isnan(t)).sum())} elements written that the kernel must leave alone"


def _at(t, off=0):
    """address of element `off` of a float32 device tensor"""
    return t.data_ptr() + 4 * off


# ------------------------------------------------------------------------------------------------------------------------------
# a. gcpx_kl_gauss, alone and as the first B workgroups of gcpx_loss_pre
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.KL_CASES))
def test_kl_gauss_matches_float64(env, name):
    """gcpx_kl_gauss in its two call conventions — the tree's (forward_plan.py:523: rows [mu | log_sigma] inside [B][PS][2 nz], PS > N, base
    one slot in, no weights) and the sequential model's (sequential.py:543: N = T - 1, node_weight = pad_mask + 1, weight_bstride = T) —
    and with a node stride wider than the row and weights 0 / 0.5 / 1 / 2.5 (`wide`).  nz 4 / 32 / 256; N nz / 4 = 4, 19, 248, 960, 1024
    (exactly the workgroup), 1040, 1100, 2112 (the thread loop wraps once and twice); B 1 / 5; free_nats 0 / 0.1 / 1 with at least 15 %
    of the dimensions on either side of the clamp; q == p on every fourth node and on all of sequence 1 (exactly 0 at free_nats 0, else
    the floor per dimension: within the additions' roundings alone);
    log-sigmas over [-4, 2] with both ends present.  kl_out[b] per sequence within kl_tol; entries past B stay NaN.
    gcpx_loss_pre on the same arguments (loss terms all NULL) writes the same kl_out bits, 0 into out[2], [3], [4], [7], [8] and nothing else.
    worst 0.0631 (seq-nz32-N130-B5-fn1)."""
    rt, lib, dev = env
    c = R.kl_case(name)
    B, N, nz = c["B"], c["N"], c["nz"]
    low, high = R.kl_clamp_shares(c)
    assert low >= 0.15 and high >= 0.15, (low, high)
    qd, pd = c["q_buf"].to(dev), c["p_buf"].to(dev)
    wd = c["w_buf"].to(dev) if c["w_buf"] is not None else None
    args = (N, nz, c["bs"], c["ns"], c["fn"], _at(wd, c["w_off"]) if wd is not None else None, c["w_bs"])
    kl = _nan(B + 3)
    rt.check(lib.gcpx_kl_gauss(_at(qd, c["off"]), _at(pd, c["off"]), B, *args, kl.data_ptr(), _st()), "kl_gauss")
    torch.cuda.synchronize()
    ref, _ = R.kl_gauss(c["q"], c["p"], c["fn"], c["w"])
    worst = _within(kl[:B], ref, R.kl_tol(c["q"], c["p"], c["fn"], c["w"]), f"kl_out {name}")
    _untouched(kl[B:], "kl_out past B")
    if B > 1:
        # q == p on every node of sequence 1: each dimension is exactly the floor (exactly 0 at free_nats 0), only the additions round
        wsum = float(c["w"][1].double().abs().sum()) if c["w"] is not None else float(N)
        assert abs(float(kl[1]) - float(ref[1])) <= R.kl_depth(N, nz) * R.EPS * nz * c["fn"] * wsum, (float(kl[1]), float(ref[1]))
    kl2, out = _nan(B + 3), _nan(16)
    la = rt.LossArgs()
    la.out, la.B, la.T, la.N = out.data_ptr(), B, N + 1, N
    rt.check(lib.gcpx_loss_pre(C.byref(la), _at(qd, c["off"]), _at(pd, c["off"]), *args, kl2.data_ptr(), _st()), "loss_pre")
    torch.cuda.synchronize()
    assert torch.equal(kl2[:B], kl[:B]), "gcpx_loss_pre and gcpx_kl_gauss: different kl_out bits"
    _untouched(kl2[B:], "kl_out of loss_pre past B")
    assert bool((out[[2, 3, 4, 7, 8]] == 0).all()), "absent terms report 0"
    _untouched(out[[0, 1, 5, 6] + list(range(9, 16))], "out slots gcpx_loss_pre does not own")
    print(f"[ratio] kl_gauss {name}: {worst:.3g}")


# ------------------------------------------------------------------------------------------------------------------------------
# b. gcpx_loss_combine and gcpx_loss_pre + gcpx_loss_final
# ------------------------------------------------------------------------------------------------------------------------------
def _loss_args(rt, c, dev, out, kl_b):
    """gcpx_loss_args of a loss case (forward_plan.py:525-551 / sequential.py:545-563); returns (args, the device tensors it points to)"""
    keep = {k: c[k].to(dev) for k in ("nll_bt", "pad_mask", "len_logits", "end_ind", "existence", "leave", "regressed_state", "state_target",
                                      "seq_len", "state_mask", "action_pred", "action_seq", "inv_t0", "cost_pred", "cost_target")
            if c[k] is not None}
    assert keep["end_ind"].dtype == torch.int64 and keep["inv_t0"].dtype == torch.int64
    assert keep["leave"].dtype == torch.int32 and keep["seq_len"].dtype == torch.int32
    la = rt.LossArgs()
    for k, t in keep.items():
        setattr(la, k, t.data_ptr())
    la.kl_b = kl_b.data_ptr() if c["kl_b"] is not None else None
    la.out, la.B, la.T, la.N, la.state_dim, la.n_actions = out.data_ptr(), c["B"], c["T"], c["N"], c["state_dim"], c["n_actions"]
    for k in R.WEIGHTS:
        setattr(la, k, c[k])
    la.total_div = c["total_div"]
    if c["w_kl_dev"] is not None:                       # burn-in schedule: the weight in force lives in device memory
        keep["w_kl_dev"] = torch.tensor([c["w_kl_dev"]], dtype=torch.float32, device=dev)
        la.w_kl_dev = keep["w_kl_dev"].data_ptr()
    return la, keep


@pytest.mark.parametrize("form", ["combine", "pre+final"])
@pytest.mark.parametrize("name", R.LOSS_CASES)
def test_loss_terms_match_float64(env, name, form):
    """Every output slot 0..8 of gcpx_loss_combine (one 256-thread workgroup) and of gcpx_loss_pre + gcpx_loss_final (the five latent-side
    terms in 1024-thread workgroups of their own) against loss_terms in float64, within loss_tol; out[9..15] stay NaN.
    Shapes (tests/loss_refs.py: _SHAPES): T 5 / 64 / 65 / 130 (the lane loop of the length cross entropy: part of a trip, exactly one, one
    and a lane, three) with B 1 / 4 / 5 / 17 (17 sequences wrap the wavefront-per-sequence loop of both forms), end_ind at 0 and T - 1,
    logits over +-50; existence logits to +-30 with B N = 7, 252, 527, 1275, `leave` all 0 / all 1 for a sequence; max(seq_len) < T and
    = T, state_dim 1 / 2 / 5, state_mask NULL and given (then frame 0 differs from pad_mask, sequential.py:546-557), states beyond
    max(seq_len) = SENT; n_actions 1 / 2 / 7, inv_t0 at 0 and T - 2, every other action row = SENT; B T = 325 and 2210, pad_mask rows
    of 0 over values of 1e4 size.  The variants of T20-B5 set each weight in turn to 0 and to -0.5 (reported, not added), read the KL
    weight from a device scalar (0.25, 0 and -1 against w_kl = 0.5) and NULL each optional pointer in turn (the term is 0 and out of
    the total).  total_div = T x 3 x 8 x 8 as the model sets it.
    pre+final: kl_b is what gcpx_loss_pre wrote (checked against kl_gauss within kl_tol, tree layout, free_nats 0.1); the KL term's
    reference is the mean of those f32 values.
    worst combine 0.156 (T5-B1), pre+final 0.143 (T5-B1)."""
    rt, lib, dev = env
    c = R.loss_case(name)
    B, N = c["B"], c["N"]
    out = _nan(16)
    if form == "combine":
        kl_b = torch.full((B + 2,), SENT, device=dev)
        if c["kl_b"] is not None:
            kl_b[:B] = c["kl_b"].to(dev)
        la, keep = _loss_args(rt, c, dev, out, kl_b)
        rt.check(lib.gcpx_loss_combine(C.byref(la), _st()), "loss_combine")
        torch.cuda.synchronize()
        cref, threads = c, 256
    else:
        kl_b = _nan(B + 2)
        la, keep = _loss_args(rt, c, dev, out, kl_b)
        nz = R.KL_NZ
        bufs = []
        for rows in (c["q"], c["p"]):                   # forward_plan.py:523: PS = N + 1 slots, the rows one slot in
            buf = torch.full((B, N + 1, 2 * nz), SENT)
            buf[:, 1:] = rows
            bufs.append(buf.to(dev))
        rt.check(lib.gcpx_loss_pre(C.byref(la), _at(bufs[0], 2 * nz), _at(bufs[1], 2 * nz), N, nz, (N + 1) * 2 * nz, 2 * nz, c["kl_fn"],
                                   None, 0, kl_b.data_ptr(), _st()), "loss_pre")
        torch.cuda.synchronize()
        pre = out.clone()
        _untouched(pre[[0, 1, 5, 6] + list(range(9, 16))], "out slots gcpx_loss_pre does not own")
        kref, _ = R.kl_gauss(c["q"], c["p"], c["kl_fn"])
        _within(kl_b[:B], kref, R.kl_tol(c["q"], c["p"], c["kl_fn"]), f"kl_out of loss_pre {name}")
        _untouched(kl_b[B:], "kl_out past B")
        rt.check(lib.gcpx_loss_final(C.byref(la), _st()), "loss_final")
        torch.cuda.synchronize()
        assert torch.equal(out[[2, 3, 4, 7, 8]], pre[[2, 3, 4, 7, 8]]), "gcpx_loss_final changed a term of gcpx_loss_pre"
        cref = dict(c, kl_b=kl_b[:B].cpu()) if c["kl_b"] is not None else c
        threads = 1024
    ref, _ = R.loss_terms(cref)
    tol = R.loss_tol(cref, threads)
    for s, slot in enumerate(R.SLOTS):
        print(f"  out[{s}] {slot}: got {float(out[s])!r} want {float(ref[s])!r} tol {float(tol[s]):.3e}")
    worst = _within(out[:9], ref, tol, f"loss {form} {name}")
    _untouched(out[9:], "out[9..15]")
    # an absent term is exactly 0; a term of weight <= 0 is still reported
    absent = {1: c["kl_b"] is None, 2: c["len_logits"] is None, 3: c["existence"] is None,
              4: c["regressed_state"] is None or c["state_target"] is None, 7: c["action_pred"] is None, 8: c["cost_pred"] is None}
    for s, gone in absent.items():
        assert (float(out[s]) == 0.0) == gone, (s, float(out[s]))
    print(f"[ratio] loss {form} {name}: {worst:.3g}")


# ------------------------------------------------------------------------------------------------------------------------------
# c. gcpx_bn_finalize
# ------------------------------------------------------------------------------------------------------------------------------
# momentum, running buffers given, mean_out / rstd_out given
_BN_VARIANTS = [(0.1, True, True), (1.0, True, False), (0.0, False, True), (0.0, False, False)]


@pytest.mark.parametrize("shape", R.BN_CASES, ids=lambda s: "%dx%dx%d" % s)
def test_bn_finalize_matches_float64(env, shape):
    """gcpx_bn_finalize as the forward calls it (plan_ops.py:336; pitch = 16 C for the decoder input, forward_plan.py:122; pitch = cpad > C
    with padding columns, forward_plan.py:173) against float64 sums of the SAME f32 partial table: indexing and reduction alone.
    (n_partial, pitch, C): (1, 1, 1) with count = 1 (the running variance takes the biased form); (3, 48, 48); (2047 | 2048 | 2049, ..):
    one short of an 8-deep unrolled trip, exactly one, one and a remainder — the last with C = 100 in a pitch of 112 whose 12 padding
    columns hold SENT; (130, 128, 8) and (600, 64, 4): 16 replicas per row, 2080 and 9600 entries per channel.  Channels with
    |mean| = 1e3 std, a constant channel (variance exactly 0: the clamp), a channel of zeros.  scale, shift, mean_out and rstd_out
    (given and NULL) and the running statistics (given and NULL; momentum 0.1 and 1) within the bounds of loss_refs.bn_finalize;
    scale / shift past C and every buffer not handed over stay NaN.
    worst 0.945 (rstd_out at 2048 x 16 x 16: the cast's own half ulp is the bound)."""
    rt, lib, dev = env
    c = R.bn_case(*shape)
    n, pitch, Cc = shape
    part, gamma, beta = c["partial"].to(dev), c["gamma"].to(dev), c["beta"].to(dev)
    worst = 0.0
    for momentum, running, stats in _BN_VARIANTS:
        scale, shift, mean, rstd = _nan(Cc + 3), _nan(Cc + 3), _nan(Cc + 2), _nan(Cc + 2)
        rm, rvar = _nan(Cc + 2), _nan(Cc + 2)
        rm[:Cc], rvar[:Cc] = c["running_mean"].to(dev), c["running_var"].to(dev)
        rt.check(lib.gcpx_bn_finalize(part.data_ptr(), n, pitch, Cc, c["count"], gamma.data_ptr(), beta.data_ptr(), R.BN_EPS,
                                      scale.data_ptr(), shift.data_ptr(), rm.data_ptr() if running else None,
                                      rvar.data_ptr() if running else None, momentum, mean.data_ptr() if stats else None,
                                      rstd.data_ptr() if stats else None, _st()), "bn_finalize")
        torch.cuda.synchronize()
        kw = dict(momentum=R.f32(momentum), running_mean=c["running_mean"], running_var=c["running_var"]) if running else {}
        ref, tol = R.bn_finalize(c["partial"], n, pitch, Cc, c["count"], c["gamma"], c["beta"], R.BN_EPS, **kw)
        got = dict(scale=scale, shift=shift)
        if stats:
            got.update(mean=mean, rstd=rstd)
        else:
            _untouched(mean, "mean_out not handed over")
            _untouched(rstd, "rstd_out not handed over")
        if running:
            got.update(running_mean=rm, running_var=rvar)
        else:
            assert torch.equal(rm[:Cc].cpu(), c["running_mean"]) and torch.equal(rvar[:Cc].cpu(), c["running_var"])
        for k, t in got.items():
            worst = max(worst, _within(t[:Cc], ref[k], tol[k], f"bn_finalize {shape} momentum {momentum} {k}"))
            _untouched(t[Cc:], f"{k} past C")
    print(f"[ratio] bn_finalize {shape}: {worst:.3g}")
