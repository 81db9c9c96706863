"""The 16-channel row-folded weight packs (GCPX_SPLIT_ROWFOLD16, conv3x3_up16_fold16_kernel): pieces against the folded weights, and the
index map the device-side split gathers through."""
import pytest
import torch

from video_gcp_amd import packing as pk


@pytest.fixture(scope="module")
def weights():
    torch.manual_seed(16)
    w = torch.randn(16, 32, 3, 3) / (9 * 32) ** 0.5
    w[3, 5] *= 2.0 ** -9                      # a few small weights: their second piece is a subnormal f16
    return w


@pytest.mark.parametrize("cbase", [0, 16])
def test_pack_fold16_pieces_recombine_to_the_folded_weights(weights, cbase):
    """(w1 + w2) 2^-e against conv3x3_fold16_gather(fold_up_weights(w)) in float64.  Bound, from split_f16: the scaled weight ws = w 2^e
    has |ws| < 2^15; w1 = f16(ws) leaves r = ws - w1 with |r| <= 2^-11 |ws|, exactly an f32; w2 = f16(r) leaves 2^-11 |r| where w2 is a
    normal f16 and at most half the subnormal spacing, 2^-25, where it is not: |w - (w1 + w2) 2^-e| <= max(2^-22 |w|, 2^-25 2^-e),
    and both are <= 2^-22 max|w| because the largest |ws| is >= 2^14 — half the issue's starting figure 2^-21 max|w|."""
    packed, e = pk.pack_conv3x3_fold16(weights, cbase)
    assert packed.dtype == torch.int16 and tuple(packed.shape) == (16, 2, 64, 8)
    want = pk.conv3x3_fold16_gather(pk.fold_up_weights(weights), cbase).double()
    pieces = packed.view(torch.float16).double()
    got = (pieces[:, 0] + pieces[:, 1]) * 2.0 ** -e
    err = (got - want).abs()
    bound = torch.maximum(2.0 ** -22 * want.abs(), torch.full_like(want, 2.0 ** (-25 - e)))
    print(f"worst error / bound = {float((err / bound).max()):.3f}; bound / (2^-22 max|w|) <= {float(bound.max() / (2.0 ** -22 * want.abs().max())):.3f}")
    assert bool((err <= bound).all())
    assert float(bound.max()) <= 2.0 ** -22 * float(want.abs().max())
    assert 2.0 ** 14 <= float(want.abs().max()) * 2.0 ** e < 2.0 ** 15


@pytest.mark.parametrize("cbase", [0, 16])
def test_fold16_index_reproduces_the_gather(weights, cbase):
    """gathering the flat [24, 16, 32] folded weights through conv3x3_fold16_index (-1 = zero) is the gather itself, and the -1 entries
    are exactly the zero half of the single-tap k-steps: fragments of kind 1 (odd fragment number), lane groups q >> 1 = 1"""
    fw = pk.fold_up_weights(weights)
    idx = pk.conv3x3_fold16_index(32, cbase)
    assert idx.dtype == torch.int32 and idx.numel() == 16 * 512
    flat = fw.reshape(-1)
    got = torch.where(idx >= 0, flat[idx.clamp(min=0).long()], torch.zeros(()))
    assert torch.equal(got.view(16, 64, 8), pk.conv3x3_fold16_gather(fw, cbase))
    assert int(idx.max()) < flat.numel()
    frag = torch.arange(16)[:, None, None]
    lane = torch.arange(64)[None, :, None]
    zero_half = ((frag % 2 == 1) & (lane >> 5 == 1)).expand(16, 64, 8)
    assert torch.equal(idx.view(16, 64, 8) < 0, zero_half)
    # the node pack and the skip pack read disjoint channels of the same scratch
    ch = idx[idx >= 0] % 32
    assert int(ch.min()) == cbase and int(ch.max()) == cbase + 15
