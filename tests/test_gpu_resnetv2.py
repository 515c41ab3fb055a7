"""splat_slam_amd.resnetv2 on the MI355X: the convolution, the group norm and the pool at their edges against the fp64 statements of
tests/resnetv2_ref.py, the whole backbone and MonoDepth(backbone="hip") on a reduced network.  The tolerance is the project's own
criterion (vit_ref.check_against_oracle): the error against fp64 is measured against that of the torch composition of the same weights.
Bitwise claims are torch.equal."""
import pytest
import torch
import torch.nn.functional as F

import mono_depth_ref as MR
import resnetv2_ref as R
import vit_ref as VR

pytestmark = pytest.mark.gpu

DEV = "cuda"
SEED = 5
TILE = 128                                   # output pixels of one workgroup of the convolution, and of one statistics record


def reduced_cfg(stage_layers=(1, 1, 2)):
    from splat_slam_amd.mono_depth import MonoDepthConfig
    return MonoDepthConfig(stem_chs=32, stage_chs=(64, 128, 256), stage_layers=stage_layers, gn_groups=8, dim=128, heads=2, depth=4, taps=(2, 3),
                           pos_grid=4, features=32, net_size=(64, 96))


def rand(*shape, seed, scale=1.0):
    return ((2 * torch.rand(*shape, generator=torch.Generator().manual_seed(seed)) - 1) * scale).to(DEV)


def two_scales(B, C, h, w, seed):
    """images drawn at different scales (1, 4, 0.25, ...), so that a sum that mixes images shows"""
    x = rand(B, C, h, w, seed=seed)
    return x * torch.tensor([4.0 ** ((i + 1) // 2 * (-1) ** i) for i in range(B)], device=DEV).reshape(B, 1, 1, 1)


def check_conv(name, B, cin, cout, k, stride, h, w, padding="same", bias=False, act="none", seed=0):
    from splat_slam_amd.resnetv2 import conv2d_same_f16
    x = two_scales(B, cin, h, w, seed + 1)
    wt = rand(cout, cin, k, k, seed=seed + 2, scale=(cin * k * k) ** -0.5 * 3 ** 0.5)
    b = rand(cout, seed=seed + 3) if bias else None
    got = conv2d_same_f16(x, wt, stride, padding, b, act)
    oracle = R.conv_ref(x, wt, stride, padding, b, act == "relu")
    assert got.dtype == torch.float16 and got.shape == oracle.shape, (got.shape, oracle.shape)
    VR.check_against_oracle(name, ("conv",), (got,), (R.conv_torch(x, wt, stride, padding, b, act == "relu"),), (oracle,))


# ---- convolution -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("k", [1, 3, 7])
def test_conv_same_padding_on_odd_and_even_maps(k, stride):
    """odd and even sizes take different before / after amounts; on 1 x 1 and 2 x 2 most taps are padding"""
    for h, w in ((1, 1), (2, 2), (7, 8), (8, 7)):
        check_conv(f"conv-k{k}-s{stride}-{h}x{w}", 2, 8, 16, k, stride, h, w, seed=10 * k + stride)


@pytest.mark.parametrize("pixels", [TILE - 1, TILE, TILE + 1])
def test_conv_around_the_pixel_tile(pixels):
    h, w = {127: (1, 127), 128: (8, 16), 129: (3, 43)}[pixels]
    check_conv(f"conv-tile-{pixels}", 2, 8, 16, 3, 1, h, w, seed=pixels)
    check_conv(f"conv-tile-{pixels}-s2", 2, 8, 16, 3, 2, 2 * h, 2 * w, seed=pixels + 1)         # ho * wo = pixels after the stride


@pytest.mark.parametrize("h,w", [(8, 8), (7, 9), (2, 2)])
def test_conv_symmetric_padding_stride_2_with_bias(h, w):
    """the reassemble convolution: 3 x 3, stride 2, padding 1, bias"""
    check_conv(f"conv-sym-{h}x{w}", 2, 16, 32, 3, 2, h, w, padding=1, bias=True, seed=h)
    check_conv(f"conv-sym-relu-{h}x{w}", 2, 16, 32, 3, 2, h, w, padding=1, bias=True, act="relu", seed=h + 1)


@pytest.mark.parametrize("cin,cout,k", [(8, 16, 1), (16, 16, 3), (1024, 16, 1), (8, 48, 3), (16, 1024, 1), (3, 32, 7)])
def test_conv_channel_edges(cin, cout, k):
    """cin 8 pads K from 8 to 32, cin 16 at k = 3 pads 144 to 160, cin 1024 is the widest input; cout 16 and 48 take the 16-wide channel
    tile, 1024 is 16 tiles of 64; 3 image channels pad to 8"""
    check_conv(f"conv-c{cin}-{cout}-k{k}", 2, cin, cout, k, 2 if k == 7 else 1, 5, 6, seed=cin + cout)


def test_conv_gives_an_image_the_same_bits_alone_and_inside_a_batch_of_300():
    """one workgroup alone, 300 (more than the card has compute units) in the batch; K = 9 * 32 = 288 is 9 steps of the k loop"""
    from splat_slam_amd.resnetv2 import conv2d_same_f16
    x = rand(300, 32, 8, 16, seed=41)
    w = rand(16, 32, 3, 3, seed=42, scale=0.1)
    batch = conv2d_same_f16(x, w, 1, "same", out_dtype=torch.float32)
    for i in (0, 7, 299):
        assert torch.equal(conv2d_same_f16(x[i:i + 1], w, 1, "same", out_dtype=torch.float32)[0], batch[i]), i
    VR.check_against_oracle("conv-grid", ("conv",), (batch[:4],), (R.conv_torch(x[:4], w),), (R.conv_ref(x[:4], w),))


def test_conv_asymmetric_padding_reads_the_appended_row_and_column_only():
    """stride 2, k = 3 on an even map pads 0 before and 1 after.  Small integers: fp16 products and fp32 sums are exact, so the output
    equals the fp64 statement.  A weight in the last tap row and column reads the appended zeros at the last output row and column; a
    weight in the first tap row and column never reads padding."""
    from splat_slam_amd.resnetv2 import conv2d_same_f16
    g = torch.Generator().manual_seed(3)
    x = torch.randint(-4, 5, (2, 8, 6, 8), generator=g).float().to(DEV)
    for corner in (0, 2):
        w = torch.zeros(16, 8, 3, 3)
        w[:, :, corner, :] = torch.randint(-3, 4, (16, 8, 3), generator=g).float()
        w[:, :, :, corner] = torch.randint(-3, 4, (16, 8, 3), generator=g).float()
        w = w.to(DEV)
        got = conv2d_same_f16(x, w, 2, "same", out_dtype=torch.float32)
        oracle = R.conv_ref(x, w, 2, "same")
        assert tuple(got.shape) == (2, 16, 3, 4) and torch.equal(got.double(), oracle)
        by_hand = F.conv2d(F.pad(x.double(), (0, 1, 0, 1)), w.double(), stride=2)                # the amounts written out: 0 before, 1 after
        assert torch.equal(oracle, by_hand)
        shifted = F.conv2d(F.pad(x.double(), (1, 0, 1, 0)), w.double(), stride=2)                # what padding in front would give
        assert not torch.equal(got.double(), shifted)


def test_conv_rejects_an_output_size_that_does_not_follow_from_the_padding():
    import ctypes as C
    from splat_slam_amd import _native as nat
    xs = torch.zeros(64, 8, dtype=torch.float16, device=DEV)
    wp = torch.zeros(16, 96, dtype=torch.float16, device=DEV)
    out = torch.zeros(16 * 64, dtype=torch.float16, device=DEV)
    c = nat.SgrResnetConv()
    c.src, c.src_stride, c.cin, c.ksize, c.stride, c.n, c.h, c.w = xs.data_ptr(), 8, 8, 3, 2, 1, 8, 8
    c.weight, c.weight_elems, c.cout, c.out, c.out_kind = wp.data_ptr(), wp.numel(), 16, out.data_ptr(), nat.SGR_UPDATE_OUT_NCHW_F16
    for pt, pl, ho, wo, ok in ((0, 0, 4, 4, True), (1, 1, 4, 4, True), (0, 0, 5, 4, False), (0, 0, 4, 3, True), (0, 0, 4, 2, False), (3, 0, 4, 4, False),
                               (1, 1, 5, 5, True), (1, 1, 6, 5, False)):
        c.pad_top, c.pad_left, c.ho, c.wo = pt, pl, ho, wo
        rc = nat.lib().sgr_resnet_conv(C.byref(c), torch.cuda.current_stream().cuda_stream)
        assert (rc == 0) == ok, (pt, pl, ho, wo, rc, nat.last_error())
    torch.cuda.synchronize()


# ---- group norm ------------------------------------------------------------------------------------------------------------------------
def gn_inputs(B, C, h, w, seed, offset=0.0, spread=1.0):
    """different statistics per image: image i is offset + (i + 1) * spread * u, shifted by i"""
    x = rand(B, C, h, w, seed=seed) * spread * torch.arange(1, B + 1, device=DEV).reshape(B, 1, 1, 1).float()
    x = x + offset + torch.arange(B, device=DEV).reshape(B, 1, 1, 1).float()
    return x, 1 + 0.5 * rand(C, seed=seed + 1), rand(C, seed=seed + 2)


def check_gn(name, x, groups, gamma, beta, relu, residual):
    from splat_slam_amd.resnetv2 import group_norm_f16
    got = group_norm_f16(x, groups, gamma, beta, relu, residual)
    oracle = R.group_norm_ref(x, groups, gamma, beta, relu, residual)
    assert got.dtype == torch.float16 and got.shape == oracle.shape
    VR.check_against_oracle(name, ("gn",), (got,), (R.group_norm_torch(x, groups, gamma, beta, relu, residual),), (oracle,))
    return got, oracle


@pytest.mark.parametrize("C,groups", [(16, 8), (32, 4), (64, 2)])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("with_residual", [False, True])
def test_group_norm_channels_per_group_relu_and_residual(C, groups, relu, with_residual):
    """2, 8 and 32 channels per group; B = 3 with different statistics per image; a 20 x 20 map spans four tiles.  Half of the residual
    is -10, which makes the value in front of the ReLU negative: a ReLU applied before the add would leave -10 in the output."""
    for h, w in ((5, 7), (20, 20)):
        x, gamma, beta = gn_inputs(3, C, h, w, seed=C + h)
        residual = None
        if with_residual:
            residual = rand(3, C, h, w, seed=C + h + 5)
            residual[:, :, :, ::2] = -10.0
        got, oracle = check_gn(f"gn-{C}/{groups}-{h}x{w}-relu{int(relu)}-res{int(with_residual)}", x, groups, gamma, beta, relu, residual)
        if relu:
            assert float(got.min()) >= 0
            if with_residual:
                assert float(got[:, :, :, ::2].abs().max()) == 0.0 and float(oracle[:, :, :, ::2].abs().max()) == 0.0
        elif with_residual:
            assert float(got[:, :, :, ::2].max()) < -4


def test_group_norm_smallest_group_and_unsupported_sizes():
    """a 1 x 1 map with 2 channels per group normalises two numbers; one element per group is an error"""
    from splat_slam_amd.resnetv2 import group_norm_f16
    x, gamma, beta = gn_inputs(3, 16, 1, 1, seed=1)
    check_gn("gn-1x1", x, 8, gamma, beta, False, None)
    with pytest.raises(RuntimeError, match="at least 2 elements"):
        group_norm_f16(x, 16, gamma, beta)
    with pytest.raises(RuntimeError, match="unsupported groups"):
        group_norm_f16(rand(1, 48, 2, 2, seed=2), 4, rand(48, seed=3), rand(48, seed=4))         # 12 channels per group


def test_group_norm_of_a_constant_group_is_beta_exactly():
    from splat_slam_amd.resnetv2 import group_norm_f16
    x, gamma, beta = gn_inputs(2, 32, 13, 11, seed=7)                                           # 143 pixels: a second, partial tile
    x[:, 8:16] = 3.7                                                                            # group 1 of 4
    x[1, 24:32] = -1e-3
    got = group_norm_f16(x, 4, gamma, beta)
    want = beta.to(torch.float16).reshape(1, 32, 1, 1).expand(2, 32, 13, 11)
    assert torch.equal(got[:, 8:16], want[:, 8:16]) and torch.equal(got[1, 24:32], want[1, 24:32])
    assert not torch.equal(got[:, :8], want[:, :8])


def test_group_norm_of_a_large_mean_keeps_the_shifted_sums_precision():
    """values 64 + u, u of spread 0.25: E[x^2] - E[x]^2 in fp32 loses the variance (x^2 ~ 4096 carries an error of 2.4e-4 against a
    variance of 0.02: about 1 % of it, i.e. 0.02 at |y| = 3), the shifted sums do not.  Beyond the criterion, the error stays below
    one fp16 ulp of the largest output (|y| < 8: 2^-8): half of it is the rounding of the result, the other half a margin that the fp32
    arithmetic (an ulp of 64 against a deviation of 0.14: 1e-4 of y) does not come near."""
    x, gamma, beta = gn_inputs(3, 32, 20, 20, seed=11, offset=64.0, spread=0.25)
    got, oracle = check_gn("gn-64+u", x, 4, gamma, beta, False, None)
    assert float(oracle.abs().max()) < 8
    assert VR.err(got, oracle)[0] <= 2.0 ** -8


# ---- pool ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(1, 1), (2, 2), (7, 8), (16, 16)])
def test_max_pool_pads_with_minus_infinity(h, w):
    """all values negative: a zero fill would win every window that touches the padding"""
    from splat_slam_amd.resnetv2 import max_pool_same_f16
    x = (-0.01 - torch.rand(2, 16, h, w, generator=torch.Generator().manual_seed(h * w))).to(torch.float16).to(DEV)
    got = max_pool_same_f16(x)
    want = R.pool_ref(x)
    assert tuple(got.shape) == (2, 16, (h + 1) // 2, (w + 1) // 2) and float(got.max()) < 0
    assert torch.equal(got, want)


# ---- the whole backbone ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nets():
    from splat_slam_amd import mono_depth as M
    from splat_slam_amd.resnetv2 import ResNetV2
    out = {}
    for layers in ((1, 1, 2), (2, 1, 1)):
        cfg = reduced_cfg(layers)
        sd = M.synthetic_state_dict(SEED, cfg)
        out[layers] = (cfg, ResNetV2.synthetic(SEED, cfg, DEV), R.prepare(sd), sd)
    return out


def make_image(B, H, W, seed):
    return (2 * torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(seed)) - 1).half().float().to(DEV)


@pytest.mark.parametrize("layers,H,W", [((1, 1, 2), 32, 32), ((1, 1, 2), 64, 96), ((2, 1, 1), 64, 96)])
def test_backbone_is_as_close_to_the_fp64_oracle_as_the_autocast_composition(nets, layers, H, W):
    """at 32 x 32 the deepest map is 2 x 2.  blocks (2, 1, 1) runs a stride-1 block without a downsample in stage 0 and, in the strided
    stages, a first block with a downsample that is also the last"""
    cfg, net, prepared, _ = nets[layers]
    x = make_image(2, H, W, H + W)
    got = net(x)
    for s, (t, c) in enumerate(zip(got, cfg.stage_chs)):
        assert t.dtype == torch.float16 and tuple(t.shape) == (2, c, H >> (s + 2), W >> (s + 2)) and torch.isfinite(t).all()
    VR.check_against_oracle(f"backbone-{layers}-{H}x{W}", ("l1", "l2", "l3"), got, R.backbone_torch(prepared, cfg, x), R.backbone_ref(prepared, cfg, x))
    again = net(x)
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    cl = net.channels_last(x)
    for t, u in zip(got, cl):
        assert u.is_contiguous() and tuple(u.shape) == (2, t.shape[2] * t.shape[3], t.shape[1])
        assert torch.equal(t.permute(0, 2, 3, 1).reshape(u.shape), u)


def test_backbone_gives_an_image_the_bits_it_has_alone(nets):
    cfg, net, _, _ = nets[(1, 1, 2)]
    x = make_image(3, 64, 96, 17) * torch.tensor([1.0, 0.25, 2.0], device=DEV).reshape(3, 1, 1, 1)
    batch = net(x)
    for i in range(3):
        alone = net(x[i:i + 1])
        assert all(torch.equal(a[0], b[i]) for a, b in zip(alone, batch)), i


def test_backbone_rejects_bad_sizes_and_cpu_tensors(nets):
    net = nets[(1, 1, 2)][1]
    with pytest.raises(ValueError, match="multiples of 32"):
        net(make_image(1, 40, 64, 1))
    with pytest.raises(ValueError, match="multiples of 32"):
        net(make_image(1, 32, 0, 1))
    with pytest.raises(RuntimeError, match="GPU tensor"):
        net(torch.zeros(1, 3, 32, 32))
    assert net.launches == 34


# ---- MonoDepth with backbone="hip" -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def models(nets):
    from splat_slam_amd import mono_depth as M
    cfg, _, _, sd = nets[(1, 1, 2)]
    prepared = MR.prepare(sd)
    return cfg, M.MonoDepth.from_state_dict(sd, cfg, DEV, backbone="hip"), MR.TorchMonoDepth(prepared, cfg, DEV), prepared, sd


@pytest.mark.parametrize("H,W", [(32, 32), (64, 96)])
def test_mono_depth_on_the_hip_backbone_meets_the_criterion_and_repeats(models, H, W):
    from splat_slam_amd.resnetv2 import ResNetV2
    cfg, model, torch_model, prepared, _ = models
    assert isinstance(model.backbone, ResNetV2) and model.backbone_kind == "hip"
    x = make_image(2, H, W, H + W)
    got = model.forward(x)
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, H, W) and torch.isfinite(got).all() and (got >= 0).all()
    oracle = MR.mono_depth_ref(prepared, cfg, x)
    assert float(oracle.max()) > 0
    VR.check_against_oracle(f"mono-hip-{H}x{W}", ("depth",), (got,), (torch_model(x),), (oracle,))
    assert torch.equal(model.forward(x), got)


def test_mono_depth_on_the_hip_backbone_gives_an_image_the_bits_it_has_alone(models):
    model = models[1]
    x = make_image(3, 64, 96, 23)
    batch = model.forward(x)
    for i in range(3):
        assert torch.equal(model.forward(x[i:i + 1])[0], batch[i]), i


def test_predict_on_the_hip_backbone_is_forward_between_the_stated_resizes(models):
    model = models[1]
    image = torch.rand(1, 3, 48, 80, generator=torch.Generator().manual_seed(9)).to(DEV)
    got = model.predict(image)
    assert got.dtype == torch.float32 and tuple(got.shape) == (48, 80) and float(got.min()) >= 0 and float(got.max()) <= 1
    assert torch.equal(got, MR.predict_by_hand(model, image)) and torch.equal(got, model(3.0, image))


def test_the_default_backbone_did_not_move(models):
    """a model built with the default arguments gives bit for bit what backbone="torch" gives, and holds no ResNetV2"""
    from splat_slam_amd import mono_depth as M
    cfg, _, _, _, sd = models
    default, named = M.MonoDepth.from_state_dict(sd, cfg, DEV), M.MonoDepth(sd, cfg, DEV, backbone="torch")
    assert default.backbone_kind == "torch" and M.MonoDepth.synthetic(SEED, cfg, DEV).backbone_kind == "torch"
    assert callable(default.backbone) and default.backbone.__func__ is M.MonoDepth.backbone
    x = make_image(2, 64, 96, 31)
    assert torch.equal(default.forward(x), named.forward(x))
    a, b = default.backbone(x.half()), named.backbone(x.half())
    assert all(torch.equal(s, t) for s, t in zip(a, b))


def test_the_prior_on_the_hip_backbone_is_slams_mono_depth_callable(models):
    import numpy as np
    import test_gpu_slam as S
    import tracker_cases as T
    from splat_slam_amd.droid_net import DroidNet
    from splat_slam_amd.fused import FusedMappingLoop
    from splat_slam_amd.mono_depth import MonoDepth
    from splat_slam_amd.slam import Slam
    cfg = S.make_cfg()
    torch.manual_seed(43)
    np.random.seed(43)
    prior = MonoDepth.synthetic(SEED, reduced_cfg(), DEV, backbone="hip")
    slam = Slam(cfg, DroidNet.synthetic(7, device=DEV), T.SyntheticStream(2), FusedMappingLoop(cfg, device=DEV), prior)
    timestamp, image, _, _ = slam.stream[0]
    mono = slam._mono(timestamp, image)
    assert tuple(mono.shape) == (T.HT, T.WD) and mono.dtype == torch.float32 and torch.isfinite(mono).all()
    assert torch.equal(mono, prior.predict(image)) and torch.equal(mono, models[1].predict(image))
