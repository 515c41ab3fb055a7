"""splat_slam_amd.encoder on the MI355X: the strided MFMA convolution bit for bit on exact data, the instance norm against fp64
statistics, batch independence, and the whole encoders against the fp64 statement tests/encoder_ref.py, their error measured against that
of the torch autocast composition of the same weights.

Measured on an MI355X: see DESIGN.md section 3, "Encoders", and profiles/encoder_times.json."""
import copy
import os

import numpy as np
import pytest
import torch

import encoder_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
SEED = 7
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_encoders.npz")
WHICH = ("fnet", "cnet")


@pytest.fixture(scope="module")
def nets():
    from splat_slam_amd import encoder as E
    out = {}
    for which in WHICH:
        sd = E.synthetic_encoder_state_dict(which, SEED)
        out[which] = (E.Encoder.synthetic(which, SEED, DEV), R.TorchEncoder(sd, E.NORM[which], DEV), R.round_fp16(sd), E.NORM[which])
    return out


def eighths(g, shape):
    return torch.randint(-8, 9, shape, generator=g).float() / 8.0


# ---- 1. exact convolution ---------------------------------------------------------------------------------------------------------
CONVS = [(3, 32, 7, 2), (32, 32, 3, 1), (32, 64, 3, 2), (32, 64, 1, 2), (64, 64, 3, 1), (64, 128, 3, 2), (64, 128, 1, 2), (128, 128, 3, 1),
         (128, 128, 1, 1), (128, 256, 1, 1)]
SIZES = [(1, 2, 2), (3, 5, 7), (2, 20, 28), (2, 13, 19)]


def exact_case(cin, cout, k, stride, n, h, w):
    g = torch.Generator().manual_seed(100000 * stride + 1000 * cin + 10 * cout + k + h)
    return eighths(g, (n, cin, h, w)), eighths(g, (cout, cin, k, k)), eighths(g, (cout,)), g


@pytest.mark.parametrize("n,h,w", SIZES)
@pytest.mark.parametrize("cin,cout,k,stride", CONVS)
def test_convolution_of_exact_data_equals_the_fp64_oracle_bit_for_bit(cin, cout, k, stride, n, h, w):
    """inputs, weights and bias are multiples of 1/8 in [-1, 1], drawn independently: every product is a multiple of 1/64 and every
    partial sum stays below 2^24 / 64, so fp32 accumulation in any order is exact"""
    from splat_slam_amd.encoder import conv2d_f16
    x, wt, b, _ = exact_case(cin, cout, k, stride, n, h, w)
    got = conv2d_f16(x.to(DEV), wt.to(DEV), b.to(DEV), stride=stride, out_dtype=torch.float32)
    ref = R.conv2d_ref(x, wt, b, stride)
    assert got.dtype == torch.float32 and tuple(got.shape) == (n, cout, (h - 1) // stride + 1, (w - 1) // stride + 1) == tuple(ref.shape)
    assert got.is_contiguous() and torch.equal(got.cpu().double(), ref)
    half = conv2d_f16(x.to(DEV), wt.to(DEV), b.to(DEV), stride=stride)
    assert half.dtype == torch.float16 and torch.equal(half, got.half())


@pytest.mark.parametrize("n,h,w", SIZES)
@pytest.mark.parametrize("cin,cout,k,stride", [(32, 32, 3, 1), (64, 64, 3, 1), (128, 128, 3, 1), (32, 64, 3, 2)])
def test_residual_tail_of_an_exact_sum_is_exact(cin, cout, k, stride, n, h, w):
    """relu(x + relu(v)) of exact v and x is exact: the no-norm block tail"""
    from splat_slam_amd.encoder import conv2d_f16
    x, wt, b, g = exact_case(cin, cout, k, stride, n, h, w)
    res = eighths(g, (n, cout, (h - 1) // stride + 1, (w - 1) // stride + 1)) * 4
    got = conv2d_f16(x.to(DEV), wt.to(DEV), b.to(DEV), stride=stride, act="relu", residual=res.to(DEV), out_dtype=torch.float32)
    ref = R.conv2d_ref(x, wt, b, stride, None, "relu", res)
    assert torch.equal(got.cpu().double(), ref) and (ref == 0).any()
    plain = conv2d_f16(x.to(DEV), wt.to(DEV), b.to(DEV), stride=stride, act="relu", out_dtype=torch.float32)
    assert torch.equal(plain.cpu().double(), R.conv2d_ref(x, wt, b, stride, None, "relu"))


@pytest.mark.parametrize("n,h,w", SIZES)
def test_tanh_relu_split_of_an_exact_sum(n, h, w):
    """the context split: relu is exact, tanh is held to 4 fp32 ulp of the fp64 tanh of the exact sum before its rounding to fp16, that
    is to half an fp16 ulp plus 4 fp32 ulp"""
    from splat_slam_amd.encoder import conv2d_f16
    x, wt, b, _ = exact_case(128, 256, 1, 1, n, h, w)
    wt = wt / 8                                                   # sums of order 1, so that tanh does not saturate everywhere
    net, inp = conv2d_f16(x.to(DEV), wt.to(DEV), b.to(DEV), act="split")
    ref_net, ref_inp = R.conv2d_ref(x, wt, b, 1, None, "split")
    assert net.dtype == inp.dtype == torch.float16 and tuple(net.shape) == tuple(inp.shape) == (n, 128, h, w)
    assert net.is_contiguous() and inp.is_contiguous()
    assert torch.equal(inp.cpu(), ref_inp.half()) and (ref_inp > 0).any() and (ref_inp == 0).any()
    t = ref_net.numpy()
    ulp32 = np.spacing(np.abs(t).astype(np.float32)).astype(np.float64)
    ulp16 = np.spacing(np.abs(t).astype(np.float16)).astype(np.float64)
    err = np.abs(net.cpu().double().numpy() - t)
    print("tanh: max error over (ulp16 / 2 + 4 ulp32):", float((err / (ulp16 / 2 + 4 * ulp32)).max()))
    assert (err <= ulp16 / 2 + 4 * ulp32).all() and np.abs(t).max() > 0.9 and np.abs(t).min() < 0.1


# ---- 2. instance norm -------------------------------------------------------------------------------------------------------------
def norm_bound_ratio(got, ref, stats):
    """max over the elements of |got - ref| / (16 * 2^-24 * (1 + |mu| / sigma) * (1 + |y|)); sigma is the sqrt(var + eps) of the
    normalisation itself, so that a constant map (sigma^2 = eps) has a finite bound"""
    mu, sigma = stats
    bound = 16 * 2.0 ** -24 * (1 + mu.abs() / sigma) * (1 + ref.abs())
    return float(((got.cpu().double() - ref).abs() / bound).max())


@pytest.mark.parametrize("n,h,w", SIZES)
@pytest.mark.parametrize("cin,cout,k,stride", [c for c in CONVS if c[1] <= 128])
def test_instance_norm_of_exact_sums(cin, cout, k, stride, n, h, w):
    """The sums are exact, so the error is that of the statistics and of the apply step: mu rounded once to fp32 costs 2^-24 |mu| / sigma,
    the subtraction, the rsqrt and the product a few ulp of y, the fp64 merge of shifted tile sums under 4: held to 16."""
    from splat_slam_amd.encoder import conv2d_f16
    x, wt, b, _ = exact_case(cin, cout, k, stride, n, h, w)
    got = conv2d_f16(x.to(DEV), wt.to(DEV), b.to(DEV), stride=stride, norm="instance", out_dtype=torch.float32)
    ref, stats = R.conv2d_ref(x, wt, b, stride, "instance", return_stats=True)
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(ref.shape) and got.is_contiguous()
    ratio = norm_bound_ratio(got, ref, stats)
    print(f"instance norm {(cin, cout, k, stride)} at {(n, h, w)}: max err / bound = {ratio:.4f}")
    assert ratio <= 1.0
    relu = conv2d_f16(x.to(DEV), wt.to(DEV), b.to(DEV), stride=stride, norm="instance", act="relu", out_dtype=torch.float32)
    assert torch.equal(relu, got.clamp_min(0))
    half = conv2d_f16(x.to(DEV), wt.to(DEV), b.to(DEV), stride=stride, norm="instance")
    assert half.dtype == torch.float16 and torch.equal(half, got.half())


@pytest.mark.parametrize("stride", [1, 2])
def test_instance_norm_of_a_map_far_from_zero(stride):
    """channel 0 constant 124, channel 1 drawn from +-1/8, both weights 1: |mu| / sigma is about 1000.  A one-pass fp32 sum of squares
    minus N mu^2 loses 2^-24 * 124^2 of a variance of 1/64, a relative 6e-2 of y, and misses this bound by more than 10x."""
    from splat_slam_amd.encoder import conv2d_f16
    g = torch.Generator().manual_seed(stride)
    x = torch.empty(2, 2, 20, 28)
    x[:, 0] = 124.0
    x[:, 1] = (torch.randint(0, 2, (2, 20, 28), generator=g).float() * 2 - 1) / 8
    wt = torch.ones(32, 2, 1, 1)
    got = conv2d_f16(x.to(DEV), wt.to(DEV), None, stride=stride, norm="instance", out_dtype=torch.float32)
    ref, stats = R.conv2d_ref(x, wt, None, stride, "instance", return_stats=True)
    assert float((stats[0].abs() / stats[1]).min()) > 900 and float(ref.abs().max()) > 0.9
    ratio = norm_bound_ratio(got, ref, stats)
    print(f"offset map, stride {stride}: max err / bound = {ratio:.4f}, max |err| = {float((got.cpu().double() - ref).abs().max()):.3e}")
    assert ratio <= 1.0


def test_bias_of_a_normalised_convolution_cancels_bitwise():
    from splat_slam_amd.encoder import conv2d_f16
    g = torch.Generator().manual_seed(9)
    x, wt, b = torch.randn(2, 32, 13, 19, generator=g).to(DEV), torch.randn(64, 32, 3, 3, generator=g).to(DEV), torch.randn(64, generator=g).to(DEV)
    res = torch.randn(2, 64, 7, 10, generator=g).to(DEV)
    for kw in ({}, {"act": "relu", "residual": res}):
        a = conv2d_f16(x, wt, 3 * b, stride=2, norm="instance", **kw)
        c = conv2d_f16(x, wt, None, stride=2, norm="instance", **kw)
        assert torch.equal(a, c) and torch.isfinite(a).all() and float(a.float().abs().max()) > 1


# ---- 3. isolation and batch independence ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", WHICH)
def test_an_image_gives_the_same_bits_alone_and_in_any_batch(nets, which):
    enc = nets[which][0]
    x = R.make_images(1, 3, 16, 24, seed=41, device=DEV, dtype=torch.float16)
    a = enc(x)
    y = x.clone()
    y[:, 1] = R.make_images(1, 1, 16, 24, seed=42, device=DEV, dtype=torch.float16)[:, 0]
    b = enc(y)
    assert torch.equal(a[:, 0], b[:, 0]) and torch.equal(a[:, 2], b[:, 2]) and not torch.equal(a[:, 1], b[:, 1])
    for i in range(3):
        assert torch.equal(enc(x[:, i:i + 1])[:, 0], a[:, i])
    assert torch.equal(enc(x.reshape(3, 1, 3, 16, 24)).reshape(a.shape), a)           # b and n are one batch axis
    if which == "cnet":
        net, inp = enc.context(x)
        one = enc.context(x[:, 1:2])
        assert torch.equal(one[0][:, 0], net[:, 1]) and torch.equal(one[1][:, 0], inp[:, 1])


# ---- 4. the whole encoders --------------------------------------------------------------------------------------------------------
def err(got, ref):
    d = (got.detach().double().cpu() - ref).abs()
    return float(d.max()), float(d.pow(2).mean().sqrt())


def check_against_oracle(name, hip, torch_out, oracle):
    """the rule of tests/test_gpu_update_op.py: max |hip - oracle| <= 2 max |torch - oracle| and rms <= 1.5 rms"""
    (e_hip, r_hip), (e_ref, r_ref) = err(hip, oracle), err(torch_out, oracle)
    print(f"{name}: max {e_hip:.3e} (torch {e_ref:.3e})  rms {r_hip:.3e} (torch {r_ref:.3e})")
    assert e_hip <= 2 * e_ref and r_hip <= 1.5 * r_ref, (name, e_hip, e_ref, r_hip, r_ref)


def check_output(out, b, n, dim, H, W):
    assert tuple(out.shape) == (b, n, dim, (H + 7) // 8, (W + 7) // 8) and out.dtype == torch.float16
    assert out.is_contiguous() and torch.isfinite(out).all()


CASES = {"2x40x56-f16": (2, 40, 56, torch.float16, False), "2x40x56-f32-strided": (2, 40, 56, torch.float32, True),
         "1x13x19-f32": (1, 13, 19, torch.float32, False), "1x13x19-f16-strided": (1, 13, 19, torch.float16, True)}


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("which", WHICH)
def test_encoder_is_as_close_to_the_fp64_oracle_as_the_autocast_composition(nets, which, case):
    enc, torch_enc, sd16, norm = nets[which]
    n, H, W, dtype, strided = CASES[case]
    x = R.make_images(1, n, H, W, seed=50 + H, device=DEV, dtype=dtype)
    if strided:
        big = torch.zeros(1, 2 * n, 3, H + 1, 2 * W, dtype=dtype, device=DEV)
        big[:, ::2, :, :H, ::2] = x
        x = big[:, ::2, :, :H, ::2]
        assert not x.is_contiguous()
    keep = x.clone()
    hip = enc(x)
    check_output(hip, 1, n, enc.out_dim, H, W)
    oracle = R.encoder_ref(sd16, norm, x)
    check_against_oracle(f"{which} {case}", hip, torch_enc(x), oracle)
    assert torch.equal(x, keep)
    if which == "cnet":
        net, inp = enc.context(x)
        check_output(net, 1, n, 128, H, W)
        check_output(inp, 1, n, 128, H, W)
        t_net, t_inp = torch_enc.context(x)
        check_against_oracle(f"context net {case}", net, t_net, torch.tanh(oracle[:, :, :128]))
        check_against_oracle(f"context inp {case}", inp, t_inp, torch.relu(oracle[:, :, 128:]))
        # against the plain output: relu commutes with the rounding; tanh of the rounded value is within half an fp16 ulp of |tanh| of
        # the fp32 tanh (v tanh'(v) <= tanh(v)), which is rounded once more: one fp16 ulp in all
        assert torch.equal(inp, hip[:, :, 128:].relu())
        t = torch.tanh(hip[:, :, :128].float())
        assert ((net.float() - t).abs() <= 2.0 ** -10 * t.abs() + 2.0 ** -24).all()


@pytest.mark.parametrize("which", WHICH)
def test_encoder_on_the_reference_fixture(nets, which):
    """the recorded outputs of the reference's own module in float64 (unrounded weights), held to the bound of the test above"""
    enc, torch_enc, _, _ = nets[which]
    g = np.load(GOLDEN)
    assert int(g["seed"]) == SEED
    x = torch.from_numpy(g["in_images"]).to(DEV)
    check_against_oracle("fixture " + which, enc(x), torch_enc(x), torch.from_numpy(g["out_" + which]))


@pytest.mark.parametrize("which", WHICH)
def test_fused_mean_and_std_equal_normalising_first(nets, which):
    enc, torch_enc, sd16, norm = nets[which]
    g = torch.Generator().manual_seed(60)
    x = torch.rand(1, 2, 3, 40, 56, generator=g).to(DEV)
    first = (x - torch.tensor(R.MEAN, device=DEV)[:, None, None]) / torch.tensor(R.STD, device=DEV)[:, None, None]
    hip = enc(x, R.MEAN, R.STD)
    check_against_oracle(which + " fused mean/std", hip, torch_enc(x, R.MEAN, R.STD), R.encoder_ref(sd16, norm, first.half()))
    print("bitwise equal to normalising first:", bool(torch.equal(hip, enc(first))))
    assert torch.equal(enc(x, torch.tensor(R.MEAN), torch.tensor(R.STD)), hip)                 # tensors or sequences


# ---- 5. reproducibility and hygiene -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", WHICH)
def test_calls_repeat_bit_for_bit_on_any_stream_and_leave_the_images_alone(nets, which):
    enc = nets[which][0]
    x = R.make_images(2, 2, 24, 40, seed=70, device=DEV, dtype=torch.float32)
    keep = x.clone()
    run = (lambda: enc.context(x, R.MEAN, R.STD) + (enc(x),)) if which == "cnet" else (lambda: (enc(x, R.MEAN, R.STD), enc(x)))
    a, b = run(), run()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c = run()
    side.synchronize()
    assert torch.equal(x, keep)
    for p, q, r in zip(a, b, c):
        assert torch.equal(p, q) and torch.equal(p, r) and p.is_contiguous() and torch.isfinite(p).all()
        assert tuple(p.shape[:2]) == (2, 2) and tuple(p.shape[3:]) == (3, 5)


# ---- 6. errors --------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_raise_before_any_launch(nets):
    from splat_slam_amd.encoder import conv2d_f16
    fnet, cnet = nets["fnet"][0], nets["cnet"][0]
    x = R.make_images(1, 2, 16, 24, seed=80, device=DEV)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        fnet(x.cpu())
    with pytest.raises(RuntimeError, match=r"\[b,n,3,H,W\]"):
        fnet(torch.zeros(1, 2, 4, 16, 24, device=DEV))
    with pytest.raises(RuntimeError, match=r"\[b,n,3,H,W\]"):
        cnet(x[0])
    with pytest.raises(RuntimeError, match="empty"):
        cnet(x[:, :0])
    with pytest.raises(RuntimeError, match="more than one element"):
        fnet(torch.zeros(1, 1, 3, 8, 8, device=DEV))
    assert tuple(cnet(torch.zeros(1, 1, 3, 8, 8, device=DEV)).shape) == (1, 1, 256, 1, 1)      # no norm, no such limit
    with pytest.raises(RuntimeError, match="fp16 or fp32"):
        fnet(x.double())
    with pytest.raises(RuntimeError, match="together"):
        fnet(x, mean=R.MEAN)
    with pytest.raises(RuntimeError, match="context"):
        fnet.context(x)
    elsewhere = copy.copy(fnet)
    elsewhere.device = torch.device("cuda", torch.cuda.current_device() + 1)
    with pytest.raises(RuntimeError, match="the encoder on cuda:"):
        elsewhere(x)
    if torch.cuda.device_count() > 1:
        with pytest.raises(RuntimeError, match="the encoder on cuda:0"):
            fnet(x.to("cuda:1"))
    with pytest.raises(RuntimeError, match="cout"):
        conv2d_f16(torch.zeros(1, 32, 8, 8, device=DEV), torch.zeros(48, 32, 3, 3, device=DEV))
    with pytest.raises(RuntimeError, match="stride"):
        conv2d_f16(torch.zeros(1, 32, 8, 8, device=DEV), torch.zeros(32, 32, 3, 3, device=DEV), stride=3)
    with pytest.raises(RuntimeError, match="cout <= 128"):
        conv2d_f16(torch.zeros(1, 32, 8, 8, device=DEV), torch.zeros(256, 32, 1, 1, device=DEV), norm="instance")


# ---- 7. DroidNet ------------------------------------------------------------------------------------------------------------------
def test_droid_net_builds_the_three_parts_from_one_dict(nets):
    import update_ref
    from splat_slam_amd.droid_net import DroidNet, synthetic_state_dict
    from splat_slam_amd.update_op import UpdateOperator
    sd = {"module." + k: v for k, v in synthetic_state_dict(SEED).items()}
    net = DroidNet.from_state_dict(sd, DEV)
    x = R.make_images(1, 2, 16, 24, seed=90, device=DEV)
    assert torch.equal(net.fnet(x), nets["fnet"][0](x)) and torch.equal(net.cnet(x), nets["cnet"][0](x))
    ins = update_ref.make_inputs(2, 5, 7, seed=91, device=DEV, dtype=torch.float16)
    ii = torch.tensor([1, 0], device=DEV)
    a, b = net.update(*ins, ii), UpdateOperator.synthetic(SEED, DEV)(*ins, ii)
    assert len(a) == 5 and all(torch.equal(p, q) for p, q in zip(a, b))
    same = DroidNet.synthetic(SEED, DEV)
    assert torch.equal(same.fnet(x), net.fnet(x))
