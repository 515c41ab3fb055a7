"""splat_slam_amd.vit on the MI355X: the GEMM bit for bit on exact data, layer norm and attention against fp64 to bounds that follow
from the number formats, and the whole transformer against the fp64 statement tests/vit_ref.py, its error measured against that of the
torch autocast composition of the same weights.

Measured on an MI355X: see DESIGN.md section 3, "Vision transformer", and profiles/mono_depth_times.json."""
import numpy as np
import pytest
import torch

import vit_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
SEED = 11


def eighths(g, shape):
    return torch.randint(-8, 9, shape, generator=g).float() / 8.0


def fp16_ulp(ref):
    """the spacing of fp16 at |ref| (that of the subnormals below 2^-14)"""
    return np.spacing(np.abs(ref.cpu().numpy()).astype(np.float16)).astype(np.float64)


# ---- 1. exact GEMM ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", [(192, 64), (2304, 768), (768, 3072), (768, 1536)])
@pytest.mark.parametrize("M", [1, 5, 63, 64, 65, 129])
def test_gemm_of_exact_data(M, N, K):
    """inputs, weights and bias are multiples of 1/8 in [-1, 1], drawn independently (an asymmetric w): every product is a multiple of
    1/64 and every partial sum stays below 2^24 / 64 at K <= 3072, so fp32 accumulation in any order is exact.  The store epilogues
    equal the fp64 product bit for bit, the residual epilogue equals the fp32 sum stream + v, and the GELU epilogue is within 1 fp16
    ulp of the fp64 GELU of the exact sum."""
    from splat_slam_amd import vit as V
    g = torch.Generator().manual_seed(100000 * M + N + K)
    a, w, b = eighths(g, (M, K)), eighths(g, (N, K)), eighths(g, (N,))
    ref = a.double() @ w.double().T + b.double()
    a16, w16, bd = a.half().to(DEV), w.half().to(DEV), b.to(DEV)
    got = V.gemm(a16, w16, bd)
    assert got.dtype == torch.float16 and tuple(got.shape) == (M, N)
    assert torch.equal(got.cpu().double(), ref.half().double())
    assert torch.equal(V.gemm(a16, w16, bd, "store_f32").cpu().double(), ref)
    assert torch.equal(V.gemm(a16, w16, None, "store_f32").cpu().double(), ref - b.double())
    stream = torch.randn(M, N, generator=g)
    out, tap = V.gemm(a16, w16, bd, "residual", out=stream.to(DEV), tap=True)
    want = stream + ref.float()
    assert torch.equal(out.cpu(), want) and torch.equal(tap.cpu(), want.half())
    gl = V.gemm(a16, w16, bd, "gelu_f16")
    gref = R.gelu_ref(ref)
    e = np.abs(gl.cpu().double().numpy() - gref.numpy()) / fp16_ulp(gref)
    print("gelu max error in fp16 ulp:", float(e.max()))
    assert (e <= 1.0).all()


def test_gemm_with_an_identity_operand_returns_the_other_transposed():
    """a = I and an asymmetric w: out[m][n] = w[n][m], which a swapped lane map of either operand or of the result would not give"""
    from splat_slam_amd import vit as V
    g = torch.Generator().manual_seed(3)
    for K in (64, 128):
        w = eighths(g, (192, K))
        w[5, 3], w[3, 5] = 1.0, -1.0
        out = V.gemm(torch.eye(K).half().to(DEV), w.half().to(DEV), None, "store_f32")
        assert torch.equal(out.cpu(), w.T.contiguous())


def test_gemm_token_maps_of_the_readout_and_embedding_epilogues():
    from splat_slam_amd import vit as V
    g = torch.Generator().manual_seed(4)
    B, T, N, K = 3, 23, 128, 64                                      # 69 rows: two row tiles, the second ragged
    a, w, b = eighths(g, (B * T, K)), eighths(g, (N, K)), eighths(g, (N,))
    aux = eighths(g, (B, N))
    got = V.gemm(a.half().to(DEV), w.half().to(DEV), None, "readout", aux=aux.to(DEV), T=T)
    ref = R.gelu_ref((a.double() @ w.double().T).reshape(B, T, N) + aux.double()[:, None])[:, 1:].transpose(1, 2)
    assert tuple(got.shape) == (B, N, T - 1)
    assert (np.abs(got.cpu().double().numpy() - ref.numpy()) <= fp16_ulp(ref)).all()
    table = eighths(g, (T, N))
    a = eighths(g, (B * (T - 1), K))
    got = V.gemm(a.half().to(DEV), w.half().to(DEV), b.to(DEV), "embed", aux=table.to(DEV), T=T).cpu().reshape(B, T, N)
    ref = (a.double() @ w.double().T + b.double()).reshape(B, T - 1, N) + table.double()[None, 1:]
    assert torch.equal(got[:, 1:].double(), ref) and (got[:, 0] == 0).all()


# ---- 2. layer norm ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [64, 768])
def test_layernorm_rows(D):
    """random rows, a constant row (beta exactly) and rows of mean 10^3 with unit spread, within 1 fp16 ulp of the fp64 result: one
    rounding to fp16 plus the fp32 error, about 2e-7 of |beta| where the result cancels against beta; with |beta| <= 0.1 that is below
    half the smallest fp16 spacing."""
    from splat_slam_amd import vit as V
    g = torch.Generator().manual_seed(D)
    x = torch.randn(7, D, generator=g)
    x[2] = 3.7
    x[3] = 1000.0 + torch.randn(D, generator=g)
    x[5] = -1000.0 + torch.randn(D, generator=g)
    gamma, beta = 1 + 0.1 * torch.randn(D, generator=g), 0.1 * (2 * torch.rand(D, generator=g) - 1)
    got = V.layernorm(x.to(DEV), gamma.to(DEV), beta.to(DEV)).cpu()
    ref = R.layernorm_ref(x, gamma, beta)
    assert got.dtype == torch.float16 and torch.equal(got[2], beta.half())
    e = np.abs(got.double().numpy() - ref.numpy()) / fp16_ulp(ref)
    print("layernorm max error in fp16 ulp:", float(e.max()))
    assert (e <= 1.0).all()


# ---- 3. attention -----------------------------------------------------------------------------------------------------------------
def attention_bound(qkv):
    """4 * 2^-11 * max |v| over the keys of each (image, head): the fp16 rounding of P against sum p = 1, the same rounding in the
    normaliser, the rounding of the output, and one more for fp32 noise; [B,1,heads * 64]"""
    B, T, _, H, d = qkv.shape
    vmax = qkv[:, :, 2].double().abs().amax(dim=(1, 3))              # [B,H]
    return (4 * 2.0 ** -11 * vmax)[:, None, :, None].expand(B, 1, H, d).reshape(B, 1, H * d)


def make_qkv(B, T, heads, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, T, 3, heads, 64, generator=g).half().to(DEV)


@pytest.mark.parametrize("heads", [1, 12])
@pytest.mark.parametrize("T", [2, 5, 64, 65, 129, 1025])
def test_attention_against_fp64(T, heads):
    from splat_slam_amd import vit as V
    qkv = make_qkv(2, T, heads, 1000 * T + heads)
    got = V.attention(qkv)
    assert got.dtype == torch.float16 and tuple(got.shape) == (2, T, heads * 64)
    ratio = ((got.double() - R.attention_ref(qkv)).abs() / attention_bound(qkv)).max().item()
    print(f"attention T={T} heads={heads}: max error / bound = {ratio:.3f}")
    assert ratio <= 1.0
    assert torch.equal(V.attention(qkv), got)                         # two runs, the same bits
    assert torch.equal(V.attention(qkv[:1].contiguous())[0], got[0])  # image 0 alone
    perm = torch.randperm(T, generator=torch.Generator().manual_seed(T)).to(DEV)
    moved = qkv.clone()
    moved[:, :, 1:] = qkv[:, perm, 1:]                                # keys together with their values
    assert ((V.attention(moved).double() - got.double()).abs() <= attention_bound(qkv)).all()


def test_attention_with_logits_of_plus_and_minus_sixty():
    """q . k / 8 = +-60 (64 c^2 / 8 = 60): exp(-120) underflows, nothing overflows, and the running maximum moves from -60 to +60
    between two key tiles"""
    from splat_slam_amd import vit as V
    T, c = 130, (60 * 8 / 64) ** 0.5
    g = torch.Generator().manual_seed(60)
    qkv = torch.randn(1, T, 3, 1, 64, generator=g)
    qkv[:, :, 0] = c
    qkv[:, :, 1] = -c
    qkv[:, 70:75, 1] = c                                              # the second key tile holds the maxima
    qkv[:, 1::2, 0] = -c                                              # for the odd queries the maxima are everywhere else
    qkv = qkv.half().to(DEV)
    got = V.attention(qkv)
    assert torch.isfinite(got).all()
    ratio = ((got.double() - R.attention_ref(qkv)).abs() / attention_bound(qkv)).max().item()
    print(f"attention +-60: max error / bound = {ratio:.3f}")
    assert ratio <= 1.0


# ---- 4. the whole transformer -----------------------------------------------------------------------------------------------------
def small_cfg():
    from splat_slam_amd.vit import VitConfig
    return VitConfig(dim=128, heads=2, depth=4, taps=(2, 3), pos_grid=4, cin=64)


def wide_cfg():
    from splat_slam_amd.vit import VitConfig
    return VitConfig(dim=768, heads=12, depth=2, taps=(0, 1), pos_grid=4, cin=64)


@pytest.fixture(scope="module")
def models():
    from splat_slam_amd import vit as V
    out = {}
    for name, cfg in (("small", small_cfg()), ("wide", wide_cfg())):
        sd = V.synthetic_state_dict(SEED, cfg)
        out[name] = (cfg, V.VisionTransformer.from_state_dict(sd, cfg, DEV), R.TorchVit(R.round_fp16(sd), cfg, DEV), R.round_fp16(sd))
    return out


GRIDS = [("small", 1, 1), ("small", 2, 2), ("small", 4, 6), ("small", 8, 8), ("small", 7, 9), ("wide", 2, 2), ("wide", 32, 32)]


@pytest.mark.parametrize("which,gh,gw", GRIDS)
def test_transformer_is_as_close_to_the_fp64_oracle_as_the_autocast_composition(models, which, gh, gw):
    cfg, vit, torch_vit, sd16 = models[which]
    g = torch.Generator().manual_seed(100 * gh + gw)
    x = torch.relu(torch.randn(2, cfg.cin, gh, gw, generator=g)).half().to(DEV)
    hip = vit(x)
    for t in hip:
        assert t.dtype == torch.float16 and tuple(t.shape) == (2, cfg.dim, gh, gw) and t.is_contiguous() and torch.isfinite(t).all()
    R.check_against_oracle(f"{which}-{gh}x{gw}", ("tap_a", "tap_b"), hip, torch_vit(x), R.vit_ref(sd16, cfg, x))
    alone = vit(x[:1])
    assert torch.equal(alone[0][0], hip[0][0]) and torch.equal(alone[1][0], hip[1][0])
    again = vit(x)
    assert torch.equal(again[0], hip[0]) and torch.equal(again[1], hip[1])


def test_a_sub_range_of_launches_repeats_on_the_buffers_of_a_whole_call(models):
    cfg, vit, _, _ = models["small"]
    x = torch.randn(1, cfg.cin, 4, 6, generator=torch.Generator().manual_seed(1)).half().to(DEV)
    call, outs, keep = vit._prepare(x)
    vit._run(call)
    want = [o.clone() for o in outs]
    outs[1].zero_()
    call.first_launch = call.last_launch = vit.launches - 1           # the last readout alone
    vit._run(call)
    assert torch.equal(outs[0], want[0]) and torch.equal(outs[1], want[1])


def test_bad_arguments_raise_before_any_launch(models):
    cfg, vit, _, _ = models["small"]
    with pytest.raises(RuntimeError, match="GPU tensor"):
        vit(torch.zeros(1, cfg.cin, 2, 2))
    with pytest.raises(RuntimeError, match="cin|64"):
        vit(torch.zeros(1, cfg.cin + 64, 2, 2, device=DEV))
    from splat_slam_amd import vit as V
    with pytest.raises(RuntimeError, match="multiples of 64"):
        V.gemm(torch.zeros(4, 32, dtype=torch.half, device=DEV), torch.zeros(64, 32, dtype=torch.half, device=DEV))
