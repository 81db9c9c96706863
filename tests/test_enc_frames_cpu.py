"""CPU checks of the frame-independent encoder's host side (csrc/enc_frames.hip: gcpx_encode_frames): the weight blob and its mirror,
the folded BatchNorm affine against the float64 formula, the entry point's argument validation (before any HIP call: there is no GPU
here), and the opt-in plumbing through ImageCEMPolicy and the control entry point's arguments.

Bounds of the folded affine: scale = weight / sqrt(running_var + eps) is three float32 roundings of the formula (the sum, the root, the
quotient): 1e-6 relative, ~17 ulp, holds them with room.  shift = bias - running_mean * scale subtracts two rounded numbers, so its error
is relative to their magnitudes, not to the difference: 1e-6 * (|bias| + |running_mean * scale|)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import video_gcp_amd as V  # noqa: E402
from video_gcp_amd import packing as pk  # noqa: E402
from video_gcp_amd.hparams import GCPHParams  # noqa: E402
from video_gcp_amd.params import encoder_layers  # noqa: E402

# the nav-env test model (tests/test_gpu_nav_env.py), c1, and c1 at 64 x 64
NAV_HP = GCPHParams(batch_size=1, max_seq_len=12, img_sz=32, hierarchy_levels=4, nz_mid_lstm=64, n_lstm_layers=2, nz_mid=32, nz_enc=32,
                    nz_vae=32, state_dim=2, ngf=16, n_actions=2)
MODELS = {"nav": lambda: NAV_HP, "c1": lambda: V.config("c1"), "c1_64": lambda: V.config("c1", img_sz=64)}


@pytest.fixture(scope="module")
def lib():
    from video_gcp_amd import runtime
    if not os.path.exists(runtime.LIB_PATH):
        sys.path.insert(0, ROOT)
        import __graft_entry__
        __graft_entry__.build()
    return runtime.load_library()


@pytest.fixture(scope="module", params=sorted(MODELS))
def packed(request):
    hp = MODELS[request.param]()
    sd = V.init_params(hp, seed=3, randomize_affine=True)
    return hp, sd, pk.pack_encoder_frames(sd, hp)


def test_pack_round_trip_is_bit_exact(packed):
    hp, sd, blob = packed
    lay, total = pk.encoder_frames_layout(hp)
    assert blob.dtype == torch.float32 and blob.numel() == total and all(off % 4 == 0 for off, _ in lay.values())
    back = pk.unpack_encoder_frames(blob, hp)
    layers, c_top = encoder_layers(hp)
    assert len(layers) - 1 == {32: 2, 64: 3}[hp.img_sz]
    keys = ["encoder.net.input.conv.weight", "encoder.net.input.conv.bias", "encoder.net.head.weight", "encoder.net.head.bias"]
    for name, cin, cout, norm in layers[1:]:
        keys += [f"encoder.net.{name}.conv.weight", f"encoder.net.{name}.conv.bias"]
    for k in keys:
        assert back[k].shape == sd[k].shape and torch.equal(back[k], sd[k]), k
    # every float of the blob is accounted for: the parts tile it without a gap
    ends = sorted((off, off + int(np.prod(shp))) for off, shp in lay.values())
    assert ends[0][0] == 0 and ends[-1][1] == total and all(a[1] == b[0] for a, b in zip(ends[:-1], ends[1:]))


def test_folded_affine_against_float64(packed):
    hp, sd, blob = packed
    back = pk.unpack_encoder_frames(blob, hp)
    layers, _ = encoder_layers(hp)
    for name, cin, cout, norm in layers[1:]:
        p = f"encoder.net.{name}.norm"
        w, b, rm, rv = (sd[f"{p}.{k}"].double() for k in ("weight", "bias", "running_mean", "running_var"))
        scale = w / torch.sqrt(rv + hp.bn_eps)
        shift = b - rm * scale
        got_scale, got_shift = back[f"{p}.scale"].double(), back[f"{p}.shift"].double()
        assert got_scale.shape == (cout,) and got_shift.shape == (cout,)
        rel = ((got_scale - scale).abs() / scale.abs()).max()
        print(f"{name}: scale max rel err {float(rel):.3e}, shift max err / bound "
              f"{float(((got_shift - shift).abs() / (1e-6 * (b.abs() + (rm * scale).abs()))).max()):.3e}")
        assert ((got_scale - scale).abs() <= 1e-6 * scale.abs()).all(), name
        assert ((got_shift - shift).abs() <= 1e-6 * (b.abs() + (rm * scale).abs())).all(), name
        assert (rm != 0).any() and (rv != 1).any() and (b != 0).any()          # randomize_affine: the statistics are not the defaults


def test_unsupported_shapes_raise_value_error():
    from types import SimpleNamespace
    for over in (dict(img_sz=16), dict(img_sz=128), dict(ngf=8), dict(nz_enc=40), dict(nz_enc=512), dict(input_nc=1)):
        hp = SimpleNamespace(**dict(dict(input_nc=3, img_sz=32, ngf=16, nz_enc=128), **over))   # (GCPHParams itself refuses some of these)
        assert pk.encoder_frames_unsupported(hp)
        with pytest.raises(ValueError):
            pk.encoder_frames_layout(hp)
    assert pk.encoder_frames_unsupported(V.config("c1")) is None and pk.encoder_frames_unsupported(V.config("c2")) is None


def test_invalid_args_are_rejected_without_a_gpu(lib):
    """argument validation happens before any HIP call"""
    x = np.zeros(3 * 64 * 64 + 8, dtype=np.float32)
    w = np.zeros(64, dtype=np.float32)
    o = np.zeros(512, dtype=np.float32)
    al = lambda a: (a.ctypes.data + 15) // 16 * 16                   # 16-byte aligned addresses inside the arrays
    good = dict(images=al(x), weights=al(w), out=o.ctypes.data, out_stride=32, F=1, S=32, ngf=16, nz=32)

    def call(**over):
        a = dict(good, **over)
        return lib.gcpx_encode_frames(a["images"], a["weights"], a["out"], a["out_stride"], a["F"], a["S"], a["ngf"], a["nz"], 0.2, None)

    for over, word in ((dict(F=0), b"F <= 0"), (dict(F=-3), b"F <= 0"), (dict(S=48), b"S must be 32 or 64"), (dict(ngf=8), b"ngf must be 16"),
                       (dict(nz=40), b"nz_enc"), (dict(nz=272), b"nz_enc"), (dict(nz=0), b"nz_enc"), (dict(images=None), b"null"),
                       (dict(weights=None), b"null"), (dict(out=None), b"null"), (dict(out_stride=16), b"out_stride"),
                       (dict(images=al(x) + 4), b"aligned")):
        assert call(**over) == -1, over
        msg = lib.gcpx_last_error()
        assert b"gcpx_encode_frames" in msg and word in msg, (over, msg)
    assert not o.any()


class _StubModel:
    """records which encoder ImageCEMPolicy._infer_action calls"""
    device = torch.device("cpu")

    def __init__(self):
        self.calls = []
        self.inv_mdl = self

    def encoder(self, img):
        self.calls.append(("encoder", tuple(img.shape)))
        return torch.full((img.shape[0], 4, 1, 1), 1.0), None

    def encode_frames(self, img):
        self.calls.append(("encode_frames", tuple(img.shape)))
        return torch.full((img.shape[0], 4), 2.0)

    def run_single(self, enc, target):
        return enc[:, :2] + target[:, :2]


class _StubPlanner:
    def __call__(self, state, goal):
        return np.zeros((3, 8, 8, 3), dtype=np.float32), np.zeros((2, 2), dtype=np.float32), np.ones((3, 4), dtype=np.float32), 0.0


@pytest.mark.parametrize("flag", [True, False])
def test_policy_encodes_with_the_chosen_encoder(flag):
    from video_gcp_amd import planning as P
    m = _StubModel()
    kw = dict(batch_encode=True) if flag else {}
    policy = P.ImageCEMPolicy(m, _StubPlanner(), closed_loop_execution=True, **kw)
    assert policy.batch_encode is flag
    frames = np.zeros((1, 8, 8, 3), dtype=np.uint8)
    a = policy.act(t=0, i_tr=0, images=frames, goal_image=frames)
    want, other = ("encode_frames", "encoder") if flag else ("encoder", "encode_frames")
    assert [c[0] for c in m.calls] == [want] and m.calls[0][1] == (1, 3, 8, 8) and other not in [c[0] for c in m.calls]
    assert np.array_equal(np.asarray(a.actions), np.full(2, 3.0 if flag else 2.0, dtype=np.float32))
    # open loop: neither encoder is called, with or without the flag
    m2 = _StubModel()
    P.ImageCEMPolicy(m2, _StubPlanner(), closed_loop_execution=False, **kw).act(t=0, i_tr=0, images=frames, goal_image=frames)
    assert m2.calls == []


def test_control_arguments_accept_batch_encode():
    from video_gcp_amd import control as CT
    base = ["--experiment", "conf.py", "--out", "out"]
    assert CT.get_args(base).batch_encode == 0
    a = CT.get_args(base + ["--batch_encode", "1", "--batch_plans", "1"])
    assert a.batch_encode == 1 and a.batch_plans == 1
    assert CT.get_args(base + ["--batch_encode", "1", "--reference_rng"]).reference_rng


def test_runner_refuses_an_unsupported_shape():
    from video_gcp_amd import control as CT

    class M:
        _hp = V.config("c1", nz_enc=40)
    with pytest.raises(ValueError):
        CT.ControlRunner(M(), None, None, batch_encode=True)
    CT.ControlRunner(M(), None, None)                                 # the default path asks nothing of the shape
