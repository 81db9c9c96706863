"""The reformulation behind csrc/conv3x3_lowres.hip (GCPX_SPLIT_LOWRES), in float64 on the CPU: tap products on the source grid, then the
separable interpolate + shift-sum (packing.lowres_up_reference), against conv3x3(bilinear_x2(x)) as torch computes it.  Covers the
separable stage, the upsample's edge clamp and the conv's zero padding."""
import pytest
import torch
import torch.nn.functional as F

from video_gcp_amd import packing as pk


@pytest.mark.parametrize("Hin", [1, 2, 4, 8])
@pytest.mark.parametrize("cin,cout,bias", [(5, 3, True), (32, 16, False)])
def test_lowres_reference_equals_conv_of_upsampled(Hin, cin, cout, bias):
    torch.manual_seed(Hin * 100 + cin)
    x = torch.randn(3, cin, Hin, Hin, dtype=torch.float64)
    w = torch.randn(cout, cin, 3, 3, dtype=torch.float64)
    b = torch.randn(cout, dtype=torch.float64) if bias else None
    want = F.conv2d(F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False), w, b, padding=1)
    got = pk.lowres_up_reference(x, w, b)
    assert got.shape == want.shape and got.dtype == torch.float64
    err = float((got - want).abs().max())
    print(f"Hin {Hin}: max error {err:.3e}, max |out| {float(want.abs().max()):.3e}")
    assert err <= 1e-12 * float(want.abs().max())


@pytest.mark.parametrize("n", [1, 2, 4, 8])
def test_bilinear_matrix_equals_interpolate(n):
    eye = torch.eye(n, dtype=torch.float64)[None, None]                       # [1, 1, n (source index), n]
    want = F.interpolate(eye, scale_factor=(1, 2), mode="bilinear", align_corners=False)[0, 0]      # [source, 2 n] -> transpose
    assert float((pk.bilinear_x2_matrix(n) - want.t()).abs().max()) <= 1e-15          # (weights are multiples of 1/4)
