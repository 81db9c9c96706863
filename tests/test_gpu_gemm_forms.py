"""-m gpu: every device body of the exact row GEMM (csrc/gemm_tile.h: gemm_tile<PR, CR, LSTM, KS>, launched by gcpx_gemm) against the
float64 reference of tests/gemm_refs.py, within the rounding bounds derived there (pinned without a GPU by tests/test_gemm_refs_cpu.py).

gemm_tile exists as nine one-wavefront block shapes and five split-K block shapes, each with the plain / LReLU epilogue and with the
LSTM cell: 28 bodies, with three different k-unrolls and so three different k-tails and ping-pong loops.  Every test here first asks
gcpx_gemm_form which body gcpx_gemm launches for its arguments and asserts that it is the one the test is named for — the
one-wavefront forms are forced through GCPX_GEMM_TILE / GCPX_GEMM_NO_KS_BLOCKS / GCPX_GEMM_NOKS (read on each call), the split-K forms
come from the cost models at the shapes of gemm_refs.KS_FORMS (256 CUs); a mismatch fails, nothing skips.

  tails    plain epilogue + bias; one-wavefront forms at M = 16 PR + 5, N = 16 CR 5 (a row block with one partly valid tile and PR - 1
           masked ones, a column block with three wavefronts leaving early); sources of 1, 7, 9 k-groups, and of 65 + 17; the output
           has padded strides in a NaN-filled buffer: nothing but the M x N outputs may be written.
  sources  shifts -1, 0, +1 inside batches of 20 rows with affine + LReLU on load, a rowidx source (33 k-groups: work for all four
           split-K wavefronts, as in batched and lstm), LReLU epilogue; the one-wavefront forms also write stats_partial: each row
           block's sum and sum of squares against the float64 sums of that block's rows.
  batched  nbatch problems with their own rows, weights, bias and output (all z offsets).
  lstm     the cell epilogue: h, c (strided rows, NaN canaries between them), h_copy, gates_out; c_prev at a stride > H.

The bounds are worst-case bounds of f32 roundoff, so ratios far below 1 are what a right kernel gives; one dropped, doubled or
uncombined k-group is 1e2 - 1e3 bounds.  With `kg + u < nkg - 1` planted in mfma_set every test of this file fails; with the last
split-K partial left out of the combine every split-K test fails except tails[KS11 / KS12 / KS22 - k272], whose sources are too short
to give wavefront 3 work.  Each test prints its worst error / bound; the worst over the forms on an MI355X stands in its docstring."""
import ctypes as C

import pytest
import torch

import gemm_refs as R

pytestmark = pytest.mark.gpu
FORM_IDS = [R.form_id(f) for f in R.FORMS]


@pytest.fixture(scope="module")
def env():
    from video_gcp_amd import runtime as rt, packing as pk
    lib = rt.load_library()
    assert torch.cuda.is_available()
    return rt, pk, lib, torch.device("cuda")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _nan(n, dev):
    return torch.full((n,), R.NAN, device=dev)


def _run(env, monkeypatch, p, form):
    """gcpx_gemm on Problem p as the body `form`: asserts the query's answer, launches, and returns the float64 reference, its bounds
    and the outputs picked out of their NaN-filled buffers (everything outside the picked elements is asserted to be NaN still)."""
    rt, pk, lib, dev = env
    for k, v in R.tile_env(form).items():
        monkeypatch.setenv(k, v)
    M, N, nb, rpb = p.M, p.N, p.nbatch, p.rpb
    nbat = -(-M // rpb)
    bufs = {"xbuf": p.xbuf.to(dev), "w": torch.stack([pk.pack_gemm(p.w[z]) for z in range(nb)]).contiguous().to(dev),
            "bias": p.bias.contiguous().to(dev)}
    for i, s in enumerate(p.srcs):
        if s.rowidx is not None:
            bufs[f"rowidx{i}"] = s.rowidx.to(dev)
        if s.scale is not None:
            bufs[f"scale{i}"], bufs[f"shiftv{i}"] = s.scale.to(dev), s.shiftv.to(dev)
    kw = {}
    if p.epi == R.EPI_LSTM:
        H = N // 4
        hrow = H + 3
        hb = rpb * hrow + 5
        kw = dict(hb=hb, hrow=hrow)
        bufs.update(c_prev=p.c_prev.contiguous().to(dev), h_out=_nan(nbat * hb + 64, dev), c_out=_nan(nbat * hb + 64, dev),
                    h_copy=_nan((M + 2) * H, dev), gates_out=_nan((M + 2) * H * 4, dev))
    else:
        orow = N + 12
        ob = rpb * orow + 20
        zo = nbat * ob + 28
        kw = dict(ob=ob, orow=orow, z_out_off=zo)
        bufs["out"] = _nan(nb * zo + 2 * orow, dev)
        if p.stats:
            nrb = lib.gcpx_gemm_row_blocks(M, N)
            assert nrb == -(-M // (16 * form[1]))
            bufs["stats"] = _nan((nrb + 1) * 2 * N, dev)
    a = R.gemm_args(rt, p, lambda name: bufs[name].data_ptr(), **kw)
    out6 = (C.c_int32 * 6)()
    rt.check(lib.gcpx_gemm_form(C.byref(a), out6), "gemm_form")
    assert list(out6) == R.expected_form(form, M, N, nb), f"{p.name}: gcpx_gemm would not run {R.form_id(form)}"
    rt.check(lib.gcpx_gemm(C.byref(a), _stream()), p.name)
    torch.cuda.synchronize()

    def pick(name, idx):
        """elements idx of the flat buffer; the rest must be untouched"""
        buf = bufs[name].cpu()
        got = buf[idx]
        rest = torch.ones_like(buf, dtype=torch.bool)
        rest[idx.flatten()] = False
        assert bool(torch.isnan(buf[rest]).all()), f"{p.name}: {name} written outside its rows / columns"
        assert bool(torch.isfinite(got).all()), f"{p.name}: {name} has {int((~torch.isfinite(got)).sum())} elements not finite"
        return got.double()

    ref = R.evaluate(p)
    bnd = R.bounds(p, ref)
    got = {}
    if p.epi == R.EPI_LSTM:
        H = N // 4
        pos = R.row_offsets(M, rpb, hb, hrow)[:, None] + torch.arange(H)[None]
        got["h"], got["c"] = pick("h_out", pos), pick("c_out", pos)
        got["h_copy"] = pick("h_copy", torch.arange(M * H).view(M, H))
        got["gates"] = pick("gates_out", torch.arange(M * H * 4).view(M, H, 4))
        ref["h_copy"], bnd["h_copy"] = ref["h"], bnd["h"]
    else:
        pos = R.row_offsets(M, rpb, ob, orow)[None, :, None] + torch.arange(nb)[:, None, None] * zo + torch.arange(N)[None, None]
        got["out"] = pick("out", pos)
        if p.stats:
            got["stats"] = pick("stats", torch.arange(nrb * 2 * N).view(nrb, 2, N))
            ref["stats"], bnd["stats"] = R.stats_ref(p, ref, bnd, 16 * form[1])
    ratios = {k: float(((got[k] - ref[k]).abs() / bnd[k]).max()) for k in got}
    print(f"{p.name}: worst err / bound " + " ".join(f"{k} {v:.3g}" for k, v in ratios.items()))
    for k, v in ratios.items():
        assert v <= 1.0, f"{p.name}: {k} worst err / bound {v:.3g}"
    return ratios


@pytest.mark.parametrize("kset", list(R.K_SETS))
@pytest.mark.parametrize("form", R.FORMS, ids=FORM_IDS)
def test_gemm_form_tails(env, monkeypatch, form, kset):
    """Row, column and k tails of each of the 14 plain-epilogue bodies (see the module docstring).
    worst error / bound on an MI355X: k272 one-wavefront 0.015, split-K 0.013; k1312 one-wavefront 0.0032, split-K 0.0014."""
    _run(env, monkeypatch, R.tails_case(form, kset), form)


@pytest.mark.parametrize("form", R.FORMS, ids=FORM_IDS)
def test_gemm_form_sources(env, monkeypatch, form):
    """Shifted sources with affine + LReLU on load, a rowidx source, LReLU epilogue, per-row-block statistics (one-wavefront forms).
    worst error / bound on an MI355X: one-wavefront out 0.0027, block sums 0.0023; split-K out 0.0015."""
    _run(env, monkeypatch, R.sources_case(form), form)


def test_gemm_form_sources_stats_on_split_k_tiles(env, monkeypatch):
    """Below 64 rows a problem with stats_partial still runs as split-K single tiles: the 16-row blocks' sums behind the combine.
    worst error / bound on an MI355X: out 0.0011, block sums 0.0006."""
    _run(env, monkeypatch, R.stats_on_split_k_case(), ("KS", 1, 1))


@pytest.mark.parametrize("form,M,N,nb", R.batched_cases(), ids=[f"{R.form_id(c[0])}-x{c[3]}" for c in R.batched_cases()])
def test_gemm_form_batched(env, monkeypatch, form, M, N, nb):
    """nbatch > 1 with distinct rows, weights, bias and outputs: every one-wavefront form, split-K single tiles, a split-K block.
    worst error / bound on an MI355X: one-wavefront 0.008, split-K 0.0025."""
    _run(env, monkeypatch, R.batched_case(form, M, N, nb), form)


@pytest.mark.parametrize("form", R.FORMS, ids=FORM_IDS)
def test_gemm_form_lstm(env, monkeypatch, form):
    """The LSTM cell epilogue of each of the 14 LSTM bodies: h, c, h_copy and gates_out within the propagated bound, all finite.
    worst error / bound on an MI355X (gates, c, h = h_copy): one-wavefront 0.0067, 0.0032, 0.0051; split-K 0.0061, 0.0066, 0.0030."""
    _run(env, monkeypatch, R.lstm_case(form), form)
