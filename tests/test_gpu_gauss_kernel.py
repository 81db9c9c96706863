"""-m gpu: gcpx_gauss_nll_bwd (csrc/loss.hip), the gaussian head's likelihood and its gradient w.r.t. the head's pre-tanh output in one
pass, alone through the C ABI against the FLOAT64 restatement and the derived bounds of tests/gauss_refs.py (pinned on the CPU by
tests/test_gauss_refs_cpu.py).  Conventions of tests/test_gpu_loss_kernels.py: every output starts as NaN, a tolerance is derived
beside its reference, nothing measured; "worst" in a docstring = the largest error / tolerance measured on an MI355X."""
import pytest
import torch

import gauss_refs as G

pytestmark = pytest.mark.gpu
NAN = float("nan")


@pytest.fixture(scope="module")
def env():
    from video_gcp_amd import runtime as rt
    lib = rt.load_library()
    assert torch.cuda.is_available()
    return rt, lib, torch.device("cuda")


def _st():
    return torch.cuda.current_stream().cuda_stream


def _nan(*shape):
    return torch.full(shape, NAN, device="cuda")


def _within(got, ref, tol, name):
    got, ref, tol = got.double().cpu(), ref.double(), tol.double()
    assert got.shape == ref.shape, f"{name}: {tuple(got.shape)} against {tuple(ref.shape)}"
    assert bool(torch.isfinite(got).all()), f"{name}: {int((~torch.isfinite(got)).sum())} elements not written (or not finite)"
    err = (got - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / tol.clamp_min(1e-300))
    w = float(ratio.max())
    print(f"[ratio] {name}: worst err/tol {w:.3g}")
    assert bool((err <= tol).all()), f"{name}: {int((err > tol).sum())}/{err.numel()} elements outside the bound; worst err/tol {w:.3g}"
    return w


def _call(env, c, dev, with_colsum=True, with_nll=True):
    rt, lib, _ = env
    rows, C, npix, pitch = G.ROWS, G.CH, c["npix"], c["pitch"]
    dy, colsum, nll, dls = _nan(rows, npix, pitch), _nan(rows, pitch), _nan(rows), _nan(rows)
    rt.check(lib.gcpx_gauss_nll_bwd(dev["mu"].data_ptr(), dev["x"].data_ptr(), dev["w"].data_ptr(), dev["ls"].data_ptr(), c["scale"],
                                    dy.data_ptr(), colsum.data_ptr() if with_colsum else None, nll.data_ptr() if with_nll else None,
                                    dls.data_ptr(), rows, C, npix, pitch, _st()), "gauss_nll_bwd")
    torch.cuda.synchronize()
    return dy, colsum, nll, dls


@pytest.mark.parametrize("npix", G.NPIX)
@pytest.mark.parametrize("ls", G.LOG_SIGMAS)
def test_gauss_nll_bwd_matches_float64(env, npix, ls):
    """rows 5, C 3, pitch 16, 8 x 8 and 32 x 32 pixels, log_sigma 0 / -2.5 / 1.5; a row of weight 0, one of weight 0.37, mu with exact
    +-1 entries and entries equal to their target; every output pre-filled with NaN.  dy: every slot finite, slots >= C and the
    weight-0 row exactly 0, saturated mu exactly 0, the rest within the element bound; colsum, nll_out, dls_rows within their sum
    bounds; nll_out within the same bound of gcpx_gauss_nll; the colsum = NULL / nll_out = NULL forms write the same bits into the
    outputs they keep and leave the others alone; a second call gives identical bits.
    worst: dy 0.367 (npix 1024, log_sigma -2.5), colsum 0.027, nll_out 0.061, dls_rows 0.082, nll_out against gcpx_gauss_nll 0.071."""
    rt, lib, devc = env
    c = G.case(npix, ls)
    args = (c["mu"], c["x"], c["w"], c["ls"], c["scale"], c["pitch"])
    ref, tol = G.reference(*args), G.tolerances(*args)
    dev = dict(mu=c["mu"].to(devc), x=c["x"].to(devc), w=c["w"].to(devc), ls=torch.tensor([c["ls"]], device=devc))
    dy, colsum, nll, dls = _call(env, c, dev)
    assert bool(torch.isfinite(dy).all()), "every slot of the gradient rows is written"
    assert bool((dy[:, :, G.CH:] == 0).all()), "slots >= C are exactly 0"
    assert bool((dy[G.ZERO_ROW] == 0).all()) and bool((colsum[G.ZERO_ROW] == 0).all()) and float(dls[G.ZERO_ROW]) == 0, "weight-0 row"
    sat = (c["mu"].abs() == 1).permute(0, 2, 1)
    assert bool((dy[:, :, :G.CH].cpu()[sat] == 0).all()), "saturated tanh: gradient exactly 0"
    tag = f"npix={npix} ls={ls}"
    _within(dy, ref["dy"], tol["dy"], f"dy {tag}")
    _within(colsum, ref["colsum"], tol["colsum"], f"colsum {tag}")
    _within(nll, ref["nll"], tol["nll"], f"nll_out {tag}")
    _within(dls, ref["dls"], tol["dls"], f"dls_rows {tag}")
    # what the forward without a backward reports
    nll_fwd = _nan(G.ROWS)
    rt.check(lib.gcpx_gauss_nll(dev["mu"].data_ptr(), dev["x"].data_ptr(), dev["ls"].data_ptr(), nll_fwd.data_ptr(), G.ROWS,
                                G.CH * npix, _st()), "gauss_nll")
    torch.cuda.synchronize()
    _within(nll_fwd, ref["nll"], tol["nll"], f"gcpx_gauss_nll {tag}")
    _within(nll, nll_fwd.double().cpu(), tol["nll"], f"nll_out against gcpx_gauss_nll {tag}")
    # optional outputs
    dy2, colsum2, nll2, dls2 = _call(env, c, dev, with_colsum=False)
    assert torch.equal(dy2, dy) and torch.equal(nll2, nll) and torch.equal(dls2, dls) and bool(torch.isnan(colsum2).all())
    dy3, colsum3, nll3, dls3 = _call(env, c, dev, with_nll=False)
    assert torch.equal(dy3, dy) and torch.equal(colsum3, colsum) and torch.equal(dls3, dls) and bool(torch.isnan(nll3).all())
    # deterministic
    dy4, colsum4, nll4, dls4 = _call(env, c, dev)
    assert torch.equal(dy4, dy) and torch.equal(colsum4, colsum) and torch.equal(nll4, nll) and torch.equal(dls4, dls)


@pytest.mark.parametrize("what", ["npix", "pitch", "C>pitch", "C>4"])
def test_gauss_nll_bwd_refuses_shapes_outside_its_contract(env, what):
    """include/gcpx.h: 1 <= C <= 4, C <= pitch, pitch % 4 == 0, npix % 64 == 0.  Anything else returns a negative code and launches
    nothing: the outputs keep their NaN."""
    rt, lib, devc = env
    rows, C, npix, pitch = {"npix": (2, 3, 96, 16), "pitch": (2, 3, 64, 18), "C>pitch": (2, 3, 64, 0), "C>4": (2, 5, 64, 16)}[what]
    mu, x = torch.zeros(rows, max(C, 1), 128, device=devc), torch.zeros(rows, max(C, 1), 128, device=devc)
    w, ls = torch.ones(rows, device=devc), torch.zeros(1, device=devc)
    dy, colsum, nll, dls = _nan(rows, 128, 32), _nan(rows, 32), _nan(rows), _nan(rows)
    code = lib.gcpx_gauss_nll_bwd(mu.data_ptr(), x.data_ptr(), w.data_ptr(), ls.data_ptr(), 1.0, dy.data_ptr(), colsum.data_ptr(),
                                  nll.data_ptr(), dls.data_ptr(), rows, C, npix, pitch, _st())
    torch.cuda.synchronize()
    assert code < 0, code
    for t in (dy, colsum, nll, dls):
        assert bool(torch.isnan(t).all())
