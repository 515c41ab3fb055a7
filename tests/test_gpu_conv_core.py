"""The update operator, the encoders and the ResNet-V2 backbone run one convolution tile (csrc/sgr_conv_mma.h) behind three gathers: on
the same input and weights the three entry points give the same bits."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.mark.parametrize("n,h,w", [(2, 9, 15), (1, 2, 2)])
@pytest.mark.parametrize("cin,cout,k", [(32, 64, 3), (8, 32, 7), (64, 128, 1)])
def test_the_three_entry_points_of_the_convolution_give_the_same_bits(cin, cout, k, n, h, w):
    """135 pixels per image cross the 128-pixel tile once; in the update kernel the two images share a tile, in the other two they
    do not.  The k order of the sums is the tile's, so the fp32 results are equal, not merely close."""
    from splat_slam_amd import encoder, resnetv2, update_op
    g = torch.Generator().manual_seed(100 * cin + 10 * k + n)
    x = torch.randn((n, cin, h, w), generator=g).to(torch.float16).to(DEV)
    wt = torch.randn((cout, cin, k, k), generator=g).to(torch.float16).to(DEV)
    a = update_op.conv2d_f16(x, wt, out_dtype=torch.float32)
    b = encoder.conv2d_f16(x, wt, stride=1, out_dtype=torch.float32)
    c = resnetv2.conv2d_same_f16(x, wt, stride=1, padding=k // 2, out_dtype=torch.float32)
    assert a.dtype == b.dtype == c.dtype == torch.float32 and tuple(a.shape) == (n, cout, h, w)
    assert bool(a.abs().max() > 0)
    assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(b, c)
