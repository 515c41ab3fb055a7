"""splat_slam_amd.dpt_decoder on the MI355X: each kernel against fp64 torch on the CPU applied to the fp16-rounded inputs, with bounds
computed from the operands (one fp16 rounding of the result plus the fp32 sums), and MonoDepth(decoder="hip") on a reduced network
against the fp64 statement tests/mono_depth_ref.py by the project's criterion (tests/vit_ref.check_against_oracle)."""
import itertools

import pytest
import torch
import torch.nn.functional as F

import mono_depth_ref as MR
import vit_ref as VR

pytestmark = pytest.mark.gpu

DEV = "cuda"
SEED = 5
U16, U32 = 2.0 ** -11, 2.0 ** -24            # unit roundoffs of fp16 and fp32


def reduced_cfg():
    from splat_slam_amd.mono_depth import MonoDepthConfig
    return MonoDepthConfig(stem_chs=32, stage_chs=(64, 128, 256), stage_layers=(1, 1, 2), gn_groups=8, dim=128, heads=2, depth=4, taps=(2, 3),
                           pos_grid=4, features=32, net_size=(64, 96))


def make_image(B, H, W, seed):
    return (2 * torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(seed)) - 1).half().float().to(DEV)


def uniform(gen, *shape, scale=1.0):
    """U(-scale, scale) rounded to fp16, on the CPU"""
    return ((2 * torch.rand(*shape, generator=gen) - 1) * scale).half()


def channels_last(t):
    """NCHW on the CPU -> [B,h,w,C] on the GPU, a view of a buffer whose row stride is C rounded up to a multiple of 8"""
    p = t.permute(0, 2, 3, 1)
    wide = torch.zeros(*p.shape[:3], (p.shape[3] + 7) // 8 * 8, dtype=torch.float16)
    wide[..., :p.shape[3]] = p
    return wide.to(DEV)[..., :p.shape[3]]


# ---- the convolution ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("B,h,w", [(2, 5, 7), (1, 9, 15), (2, 1, 1)])
def test_conv_against_fp64_with_bounds_from_the_operands(B, h, w, k):
    """70 pixels: one tile of 128 spanning two images; 135: two tiles with a tail; 2: the deepest map of the reduced network.  Every
    cin in {8, 40}, cout in {1 (fp32 plane), 16, 32, 80} (channel tiles of 16 and 32, a tail for 1) and every combination of relu_in,
    the epilogue's ReLU and 0, 1 or 2 residuals.  Per output the bound is 2^-11 |oracle| + K 2^-24 sum |w x| for fp16 (one rounding of
    the result, fp32 accumulation of K = k^2 cin products), the second term alone for fp32; both terms come from the oracle's operands.
    The fp32 bound has no term for the 1 + residuals fp32 roundings of the epilogue (sum + bias, + res0, + res1), each at most 2^-24
    of |bias| + sum |w x| + |res0| + |res1|, so no fp32 result can meet it where sum |w x| is small against the bias and the residuals
    (relu_in zeroes a whole pixel of 8 channels now and then).  The fp32 plane therefore runs every combination with cin = 40; with
    cin = 8 it runs without residuals and, at k = 1 (K = 8), without relu_in; and the test asserts for each fp32 run that those
    roundings stay below half of the accumulation term, so that the data cannot silently stop supporting the bound."""
    from splat_slam_amd.dpt_decoder import conv_cl_f16
    gen = torch.Generator().manual_seed(100 * B + 10 * h + w + k)
    worst = 0.0
    for cin, cout in itertools.product((8, 40), (1, 16, 32, 80)):
        x = uniform(gen, B, cin, h, w)
        wt = uniform(gen, cout, cin, k, k, scale=1.0 / (cin * k * k) ** 0.5)
        b = uniform(gen, cout, scale=0.1)
        res = [uniform(gen, B, cout, h, w), uniform(gen, B, cout, h, w)]
        xg, wg, bg, rg = channels_last(x), wt.to(DEV), b.to(DEV), [channels_last(r) for r in res]
        out_dtype = torch.float32 if cout == 1 else torch.float16
        for relu_in, relu, nres in itertools.product((False, True), (False, True), (0, 1, 2)):
            if cout == 1 and cin == 8 and (nres or (relu_in and k == 1)):
                continue
            got = conv_cl_f16(xg, wg, bg, relu_in=relu_in, relu=relu, res0=rg[0] if nres > 0 else None, res1=rg[1] if nres > 1 else None,
                              out_dtype=out_dtype)
            assert got.dtype == out_dtype and tuple(got.shape) == (B, h, w, cout)
            xin = torch.relu(x.double()) if relu_in else x.double()
            oracle = F.conv2d(xin, wt.double(), b.double(), padding=(k - 1) // 2)
            if relu:
                oracle = torch.relu(oracle)
            for r in res[:nres]:
                oracle = oracle + r.double()
            sums = k * k * cin * U32 * F.conv2d(xin.abs(), wt.double().abs(), None, padding=(k - 1) // 2)
            bound = sums if cout == 1 else U16 * oracle.abs() + sums
            if cout == 1:
                partial = b.double().abs().view(1, -1, 1, 1) + sums / (k * k * cin * U32) + sum(r.double().abs() for r in res[:nres])
                assert bool(((1 + nres) * U32 * partial <= sums / 2).all()), (cin, relu_in, nres)
            err = (got.permute(0, 3, 1, 2).double().cpu() - oracle).abs()
            ratio = float((err / bound.clamp_min(1e-300)).max())
            worst = max(worst, ratio)
            assert bool((err <= bound).all()), (cin, cout, relu_in, relu, nres, float(err.max()), ratio)
    print(f"conv B={B} {h}x{w} k={k}: worst error / bound {worst:.3f}")


def test_conv_reads_a_row_stride_and_gives_an_image_the_bits_it_has_alone():
    from splat_slam_amd.dpt_decoder import conv_cl_f16
    gen = torch.Generator().manual_seed(3)
    wide = uniform(gen, 3, 5, 7, 24).to(DEV)
    x = wide[..., :16]                                          # row stride 24
    wt, b = uniform(gen, 32, 16, 3, 3, scale=0.1).to(DEV), uniform(gen, 32, scale=0.1).to(DEV)
    res = uniform(gen, 3, 5, 7, 40).to(DEV)[..., :32]
    batch = conv_cl_f16(x, wt, b, relu_in=True, res0=res)
    assert torch.equal(batch, conv_cl_f16(x.contiguous(), wt, b, relu_in=True, res0=res.contiguous()))
    for i in range(3):
        assert torch.equal(conv_cl_f16(x[i:i + 1].contiguous(), wt, b, relu_in=True, res0=res[i:i + 1].contiguous())[0], batch[i]), i


def test_conv_rejects_what_it_does_not_compute():
    from splat_slam_amd.dpt_decoder import conv_cl_f16
    x = torch.zeros(1, 4, 4, 8, dtype=torch.float16, device=DEV)
    with pytest.raises(RuntimeError, match="kernel size"):
        conv_cl_f16(x, torch.zeros(16, 8, 5, 5, device=DEV))
    with pytest.raises(RuntimeError, match="channels-last"):
        conv_cl_f16(torch.zeros(1, 4, 4, 12, dtype=torch.float16, device=DEV)[..., :4], torch.zeros(16, 4, 1, 1, device=DEV))
    with pytest.raises(RuntimeError, match="GPU tensor"):
        conv_cl_f16(x.cpu(), torch.zeros(16, 8, 1, 1, device=DEV))


# ---- the resampling ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,stride", [(8, 8), (24, 24), (24, 32)])
@pytest.mark.parametrize("h,w", [(1, 1), (1, 3), (2, 5), (3, 2)])
def test_up2_against_fp64(h, w, C, stride):
    """a side of one pixel copies; bound: one fp16 rounding of the result plus four fp32 roundings on values of at most max |x|"""
    from splat_slam_amd.dpt_decoder import up2_cl_f16
    wide = uniform(torch.Generator().manual_seed(h * 10 + w + C), 2, h, w, stride)
    x = wide[..., :C]
    got = up2_cl_f16(wide.to(DEV)[..., :C])                     # a view with the row stride `stride`
    assert got.dtype == torch.float16 and tuple(got.shape) == (2, 2 * h, 2 * w, C)
    oracle = F.interpolate(x.permute(0, 3, 1, 2).double(), scale_factor=2, mode="bilinear", align_corners=True)
    err = (got.permute(0, 3, 1, 2).double().cpu() - oracle).abs()
    bound = U16 * oracle.abs() + 4 * U32 * float(x.abs().max())
    print(f"up2 {h}x{w} C={C}: worst error / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()), float(err.max())


@pytest.mark.parametrize("H,W", [(48, 80), (37, 130), (480, 640)])
def test_resize_in_against_fp64(H, W):
    """up on both axes; down on one with a support of three taps and up on the other; down by 7.5 and 6.7 with supports of 16 and 14"""
    from splat_slam_amd.dpt_decoder import resize_in
    image = torch.rand(1, 3, H, W, generator=torch.Generator().manual_seed(H + W))
    got = resize_in(image.to(DEV), (64, 96))
    assert got.dtype == torch.float16 and tuple(got.shape) == (1, 3, 64, 96)
    oracle = (F.interpolate(image.double(), size=(64, 96), mode="bilinear", align_corners=False, antialias=True) - 0.5) / 0.5
    err = (got.double().cpu() - oracle).abs()
    bound = U16 * oracle.abs() + 8e-6
    print(f"resize_in {H}x{W}: worst error / bound {float((err / bound).max()):.3f}, max error {float(err.max()):.3e}")
    assert bool((err <= bound).all()), float(err.max())


@pytest.mark.parametrize("H,W", [(48, 80), (37, 130)])
def test_resize_out_against_fp64(H, W):
    from splat_slam_amd.dpt_decoder import resize_out
    depth = 1.4 * torch.rand(64, 96, generator=torch.Generator().manual_seed(H + W)) - 0.2
    assert float(depth.min()) < 0 and float(depth.max()) > 1
    got = resize_out(depth.to(DEV), (H, W))
    assert got.dtype == torch.float32 and tuple(got.shape) == (H, W) and float(got.min()) >= 0 and float(got.max()) <= 1
    oracle = F.interpolate(depth.double().clamp(0, 1)[None, None], size=(H, W), mode="bicubic").clamp(0, 1)[0, 0]
    err = float((got.double().cpu() - oracle).abs().max())
    print(f"resize_out {H}x{W}: max error {err:.3e}")
    assert err <= 32 * U32 * 1.375 ** 2


# ---- the whole network -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def models():
    from splat_slam_amd import mono_depth as M
    cfg = reduced_cfg()
    sd = M.synthetic_state_dict(SEED, cfg)
    prepared = MR.prepare(sd)
    nets = {(b, d): M.MonoDepth.from_state_dict(sd, cfg, DEV, backbone=b, decoder=d) for b, d in (("hip", "hip"), ("torch", "hip"), ("hip", "torch"))}
    return cfg, nets, MR.TorchMonoDepth(prepared, cfg, DEV), prepared


@pytest.fixture(scope="module")
def references(models):
    """(H, W) -> (x, the fp64 oracle, the autocast composition), computed once"""
    cfg, _, torch_model, prepared = models
    out = {}
    for H, W in ((32, 32), (64, 96)):
        x = make_image(2, H, W, H + W)
        out[(H, W)] = (x, MR.mono_depth_ref(prepared, cfg, x), torch_model(x))
    return out


@pytest.mark.parametrize("H,W", [(32, 32), (64, 96)])
def test_forward_on_the_hip_decoder_meets_the_criterion_and_repeats(models, references, H, W):
    """at 32 x 32 the deepest map is one pixel: refinenet4's convolutions see their zero padding only and its up2 copies"""
    from splat_slam_amd.dpt_decoder import DPTDecoder
    model = models[1][("hip", "hip")]
    assert model.decoder_kind == "hip" and isinstance(model.dpt, DPTDecoder) and model.dpt.launches == 35
    x, oracle, torch_out = references[(H, W)]
    got = model.forward(x)
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, H, W) and torch.isfinite(got).all() and (got >= 0).all()
    assert float(oracle.max()) > 0
    VR.check_against_oracle(f"mono-hip-decoder-{H}x{W}", ("depth",), (got,), (torch_out,), (oracle,))
    assert torch.equal(model.forward(x), got)


def test_forward_on_the_torch_backbone_and_the_hip_decoder_meets_the_criterion(models, references):
    """the NCHW stage maps go through the pack launch first"""
    model = models[1][("torch", "hip")]
    x, oracle, torch_out = references[(64, 96)]
    got = model.forward(x)
    VR.check_against_oracle("mono-torch-backbone-hip-decoder-64x96", ("depth",), (got,), (torch_out,), (oracle,))
    assert torch.equal(model.forward(x), got)


def test_the_hip_decoder_gives_an_image_the_bits_it_has_alone(models):
    model = models[1][("hip", "hip")]
    x = make_image(3, 64, 96, 23)
    batch = model.forward(x)
    for i in range(3):
        assert torch.equal(model.forward(x[i:i + 1])[0], batch[i]), i


def test_predict_on_the_hip_decoder_is_forward_between_its_two_resize_launches(models):
    from splat_slam_amd.dpt_decoder import resize_in, resize_out
    model = models[1][("hip", "hip")]
    image = torch.rand(1, 3, 48, 80, generator=torch.Generator().manual_seed(9)).to(DEV)
    got = model.predict(image)
    assert got.dtype == torch.float32 and tuple(got.shape) == (48, 80) and float(got.min()) >= 0 and float(got.max()) <= 1
    by_hand = resize_out(model.forward(resize_in(image, model.cfg.net_size))[0], (48, 80))
    assert torch.equal(got, by_hand) and torch.equal(got, model(3.0, image))


def test_predict_differs_from_the_torch_decoder_by_what_the_forwards_differ(models):
    """the two predicts resize back what their forwards returned, so they differ by no more than those two maps do plus the error
    bound of each bicubic resize (32 * 2^-24 * 1.375^2 against the exact resize, test_resize_out_against_fp64)"""
    from splat_slam_amd.dpt_decoder import resize_in
    hip, ref = models[1][("hip", "hip")], models[1][("hip", "torch")]
    image = torch.rand(1, 3, 48, 80, generator=torch.Generator().manual_seed(9)).to(DEV)
    x_ref = (F.interpolate(image, size=tuple(ref.cfg.net_size), mode="bilinear", align_corners=False, antialias=True) - 0.5) / 0.5
    forwards = float((hip.forward(resize_in(image, hip.cfg.net_size)).clamp(0, 1) - ref.forward(x_ref).clamp(0, 1)).abs().max())
    predicts = float((hip.predict(image) - ref.predict(image)).abs().max())
    print(f"predict hip vs torch decoder: {predicts:.3e}; forwards: {forwards:.3e}")
    assert predicts <= forwards + 2 * 32 * U32 * 1.375 ** 2


def test_the_default_decoder_did_not_move(models):
    """a model built with the default arguments gives bit for bit what decoder="torch" gives, and holds no DPTDecoder"""
    from splat_slam_amd import mono_depth as M
    cfg, nets, _, _ = models
    default = M.MonoDepth.synthetic(SEED, cfg, DEV, backbone="hip")
    assert default.decoder_kind == "torch" and not hasattr(default, "dpt") and M.MonoDepth.synthetic(SEED, cfg, DEV).decoder_kind == "torch"
    x = make_image(2, 64, 96, 31)
    assert torch.equal(default.forward(x), nets[("hip", "torch")].forward(x))
    image = torch.rand(1, 3, 48, 80, generator=torch.Generator().manual_seed(9)).to(DEV)
    assert torch.equal(default.predict(image), MR.predict_by_hand(default, image))
