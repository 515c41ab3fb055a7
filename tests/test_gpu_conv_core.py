"""The update operator, the encoders, the ResNet-V2 backbone, the DPT decoder and LPIPS run one convolution tile (csrc/sgr_conv_mma.h);
the encoders, the ResNet and LPIPS share its window gather as well.  On the same input and weights the five entry points give the
same bits, each on the cases it takes."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _operands(cin, cout, k, n, h, w):
    g = torch.Generator().manual_seed(100 * cin + 10 * k + n)
    x = torch.randn((n, cin, h, w), generator=g).to(torch.float16).to(DEV)
    wt = torch.randn((cout, cin, k, k), generator=g).to(torch.float16).to(DEV)
    return x, wt


@pytest.mark.parametrize("n,h,w", [(2, 9, 15), (1, 2, 2)])
@pytest.mark.parametrize("cin,cout,k", [(32, 64, 3), (8, 32, 7), (64, 128, 1)])
def test_the_three_entry_points_of_the_convolution_give_the_same_bits(cin, cout, k, n, h, w):
    """(Named when three files shared the tile; it holds all five.)  135 pixels per image cross the 128-pixel tile once; in the update,
    DPT and LPIPS kernels the two images share a tile, in the other two they do not.  The k order of the sums is the tile's, so the
    fp32 results are equal, not merely close.  The DPT convolution takes k 1 or 3, the LPIPS one k 3 with cout a multiple of 64; it
    stores relu(sum + bias) as fp16, so with a zero bias it is the rounded ReLU of the others' fp32 sums."""
    from splat_slam_amd import dpt_decoder, encoder, lpips, resnetv2, update_op
    x, wt = _operands(cin, cout, k, n, h, w)
    a = update_op.conv2d_f16(x, wt, out_dtype=torch.float32)
    b = encoder.conv2d_f16(x, wt, stride=1, out_dtype=torch.float32)
    c = resnetv2.conv2d_same_f16(x, wt, stride=1, padding=k // 2, out_dtype=torch.float32)
    assert a.dtype == b.dtype == c.dtype == torch.float32 and tuple(a.shape) == (n, cout, h, w)
    assert bool(a.abs().max() > 0)
    assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(b, c)
    if k in (1, 3):
        d = dpt_decoder.conv_cl_f16(x.permute(0, 2, 3, 1).contiguous(), wt, out_dtype=torch.float32)
        assert d.dtype == torch.float32 and tuple(d.shape) == (n, h, w, cout)
        assert torch.equal(a, d.permute(0, 3, 1, 2))
    if k == 3 and cout in (64, 128):
        e = lpips.conv_relu_f16(x, wt, torch.zeros(cout, device=DEV), 1, k // 2)
        assert e.dtype == torch.float16 and tuple(e.shape) == (n, cout, h, w)
        assert torch.equal(e, torch.relu(a).to(torch.float16))


def test_the_strided_gather_gives_the_same_bits_in_its_three_kernels():
    """stride 2 with padding 1 on 9 x 15 maps: the shared window gather carries the stride for the encoders, the ResNet and LPIPS, and
    all three have the output size (v - 1) // 2 + 1 = 5 x 8"""
    from splat_slam_amd import encoder, lpips, resnetv2
    (n, h, w), (cin, cout, k) = (2, 9, 15), (32, 64, 3)
    x, wt = _operands(cin, cout, k, n, h, w)
    b = encoder.conv2d_f16(x, wt, stride=2, out_dtype=torch.float32)
    c = resnetv2.conv2d_same_f16(x, wt, stride=2, padding=1, out_dtype=torch.float32)
    e = lpips.conv_relu_f16(x, wt, torch.zeros(cout, device=DEV), 2, 1)
    assert tuple(b.shape) == tuple(c.shape) == tuple(e.shape) == (n, cout, (h - 1) // 2 + 1, (w - 1) // 2 + 1)
    assert bool(b.abs().max() > 0)
    assert torch.equal(b, c)
    assert e.dtype == torch.float16 and torch.equal(e, torch.relu(b).to(torch.float16))
