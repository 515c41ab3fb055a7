"""CPU checks of the correlation restatement (tests/corr_ref.py) against an independent formulation (grid_sample over the planes and
torch autograd through it), of the droid_backends argument checks of the four correlation functions, and of their ABI.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import corr_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("corr_index_forward", "corr_index_backward", "altcorr_forward", "altcorr_backward")
ENTRY = ("sgr_corr_index_forward", "sgr_corr_index_backward", "sgr_corr_alt_forward", "sgr_corr_alt_backward")


# ---- 1. exports and argument checks (every error is raised before the device is touched)
def test_package_exports_the_four_correlation_functions():
    import droid_backends as db
    for name in NAMES:
        assert callable(getattr(db, name)) and name in db.__all__ and name in db.__doc__


def _index(**kw):
    a = dict(volume=torch.zeros(2, 4, 5, 3, 6), coords=torch.zeros(2, 2, 4, 5), radius=1)
    a.update(kw)
    return a


def _alt(**kw):
    a = dict(fmap1=torch.zeros(2, 4, 5, 8), fmap2=torch.zeros(2, 2, 3, 8), coords=torch.zeros(2, 3, 4, 5, 2), radius=1)
    a.update(kw)
    return a


def _call(name, a):
    import droid_backends as db
    if name == "corr_index_forward":
        return db.corr_index_forward(a["volume"], a["coords"], a["radius"])
    if name == "corr_index_backward":
        rd = 2 * max(int(a["radius"]), 0) + 1
        v = a["volume"]
        ok = isinstance(v, torch.Tensor) and v.dim() == 5
        grad = a.get("corr_grad", torch.zeros((v.shape[0], rd, rd) + tuple(v.shape[1:3]), dtype=v.dtype) if ok else torch.zeros(1))
        return db.corr_index_backward(v, a["coords"], grad, a["radius"])
    if name == "altcorr_forward":
        return db.altcorr_forward(a["fmap1"], a["fmap2"], a["coords"], a["radius"])
    rd = 2 * max(int(a["radius"]), 0) + 1
    c = a["coords"]
    grad = a.get("corr_grad", torch.zeros((c.shape[0], c.shape[1], rd * rd) + tuple(c.shape[2:4])) if c.dim() == 5 else torch.zeros(1))
    return db.altcorr_backward(a["fmap1"], a["fmap2"], c, grad, a["radius"])


@pytest.mark.parametrize("name", NAMES)
def test_correlation_functions_reject_cpu_tensors(name):
    with pytest.raises(RuntimeError, match="GPU tensor"):
        _call(name, _index() if name.startswith("corr_index") else _alt())
    with pytest.raises(RuntimeError, match="GPU tensor"):      # an empty batch is checked like any other
        _call(name, _index(volume=torch.zeros(0, 4, 5, 3, 6), coords=torch.zeros(0, 2, 4, 5)) if name.startswith("corr_index")
              else _alt(fmap1=torch.zeros(0, 4, 5, 8), fmap2=torch.zeros(0, 2, 3, 8), coords=torch.zeros(0, 3, 4, 5, 2)))


@pytest.mark.parametrize("name", NAMES[:2])
@pytest.mark.parametrize("kw,err,msg", [
    (dict(volume=torch.zeros(2, 4, 5, 3, 6, dtype=torch.float64)), TypeError, "volume must be torch.float16 or torch.float32"),
    (dict(volume=torch.zeros(2, 4, 5, 3, 6, dtype=torch.bfloat16)), TypeError, "volume must be torch.float16 or torch.float32"),
    (dict(coords=torch.zeros(2, 2, 4, 5, dtype=torch.float16)), TypeError, "coords must be torch.float32"),
    (dict(volume=torch.zeros(2, 4, 5, 18)), ValueError, "volume must have 5 dimensions"),
    (dict(coords=torch.zeros(2, 2, 20)), ValueError, "coords must have 4 dimensions"),
    (dict(coords=torch.zeros(2, 2, 5, 4)), ValueError, r"coords must be \[B,2,h1,w1\]"),
    (dict(coords=torch.zeros(2, 4, 5, 2)), ValueError, r"coords must be \[B,2,h1,w1\]"),
    (dict(volume=torch.zeros(2, 4, 5, 6, 3).transpose(3, 4)), ValueError, "volume must be contiguous"),
    (dict(coords=torch.zeros(2, 4, 5, 2).permute(0, 3, 1, 2)), ValueError, "coords must be contiguous"),
    (dict(radius=-1), ValueError, "radius must be >= 0"),
    (dict(volume=[1.0]), TypeError, "volume must be a torch.Tensor"),
])
def test_corr_index_rejects_bad_arguments(name, kw, err, msg):
    with pytest.raises(err, match=msg):
        _call(name, _index(**kw))


@pytest.mark.parametrize("kw,err,msg", [
    (dict(corr_grad=torch.zeros(2, 3, 3, 4, 5, dtype=torch.float16)), TypeError, "corr_grad must be torch.float32"),
    (dict(corr_grad=torch.zeros(2, 9, 4, 5)), ValueError, "corr_grad must have 5 dimensions"),
    (dict(corr_grad=torch.zeros(2, 5, 5, 4, 5)), ValueError, r"corr_grad must be \[B,rd,rd,h1,w1\]"),
    (dict(corr_grad=torch.zeros(2, 3, 3, 5, 4).transpose(3, 4)), ValueError, "corr_grad must be contiguous"),
])
def test_corr_index_backward_rejects_a_bad_gradient(kw, err, msg):
    with pytest.raises(err, match=msg):
        _call("corr_index_backward", _index(**kw))


@pytest.mark.parametrize("name", NAMES[2:])
@pytest.mark.parametrize("kw,err,msg", [
    (dict(fmap1=torch.zeros(2, 4, 5, 8, dtype=torch.float16), fmap2=torch.zeros(2, 2, 3, 8, dtype=torch.float16)), TypeError,
     "fmap1 must be torch.float32"),
    (dict(fmap2=torch.zeros(2, 2, 3, 8, dtype=torch.float16)), TypeError, "fmap2 must be torch.float32"),
    (dict(fmap1=torch.zeros(2, 4, 5, 8, dtype=torch.float64)), TypeError, "fmap1 must be torch.float32"),
    (dict(coords=torch.zeros(2, 3, 4, 5, 2, dtype=torch.float64)), TypeError, "coords must be torch.float32"),
    (dict(fmap1=torch.zeros(2, 20, 8)), ValueError, "fmap1 must have 4 dimensions"),
    (dict(coords=torch.zeros(2, 4, 5, 2)), ValueError, "coords must have 5 dimensions"),
    (dict(fmap2=torch.zeros(3, 2, 3, 8)), ValueError, r"fmap2 must be \[B,H2,W2,C\]"),
    (dict(fmap2=torch.zeros(2, 2, 3, 12)), ValueError, r"fmap2 must be \[B,H2,W2,C\]"),
    (dict(coords=torch.zeros(2, 3, 5, 4, 2)), ValueError, r"coords must be \[B,N,H1,W1,2\]"),
    (dict(coords=torch.zeros(2, 3, 2, 4, 5)), ValueError, r"coords must be \[B,N,H1,W1,2\]"),
    (dict(fmap1=torch.zeros(2, 4, 5, 6), fmap2=torch.zeros(2, 2, 3, 6)), ValueError, "positive multiple of 4"),
    (dict(fmap1=torch.zeros(2, 4, 5, 0), fmap2=torch.zeros(2, 2, 3, 0)), ValueError, "positive multiple of 4"),
    (dict(fmap1=torch.zeros(2, 8, 4, 5).permute(0, 2, 3, 1)), ValueError, "fmap1 must be contiguous"),
    (dict(radius=-2), ValueError, "radius must be >= 0"),
])
def test_altcorr_rejects_bad_arguments(name, kw, err, msg):
    with pytest.raises(err, match=msg):
        _call(name, _alt(**kw))


@pytest.mark.parametrize("kw,err,msg", [
    (dict(corr_grad=torch.zeros(2, 3, 9, 4, 5, dtype=torch.float16)), TypeError, "corr_grad must be torch.float32"),
    (dict(corr_grad=torch.zeros(2, 3, 3, 3, 4, 5)), ValueError, "corr_grad must have 5 dimensions"),
    (dict(corr_grad=torch.zeros(2, 3, 25, 4, 5)), ValueError, r"corr_grad must be \[B,N,rd\*rd,H1,W1\]"),
])
def test_altcorr_backward_rejects_a_bad_gradient(kw, err, msg):
    with pytest.raises(err, match=msg):
        _call("altcorr_backward", _alt(**kw))


# ---- 2. the restatement against a second, independent formulation
def sample_planes(planes, x0, y0, r):
    """planes [P,h2,w2] (torch fp64), x0, y0 [P] -> [P,rd(x offset),rd(y offset)]: grid_sample, align_corners, zero padding"""
    P, h2, w2 = planes.shape
    rd = 2 * r + 1
    off = torch.arange(rd, dtype=torch.float64) - r
    gx = (x0[:, None, None] + off[None, None, :]).expand(P, rd, rd)        # grid_sample's output is [y index, x index]
    gy = (y0[:, None, None] + off[None, :, None]).expand(P, rd, rd)
    grid = torch.stack([2 * gx / (w2 - 1) - 1, 2 * gy / (h2 - 1) - 1], -1)
    out = F.grid_sample(planes[:, None], grid, mode="bilinear", padding_mode="zeros", align_corners=True)[:, 0]
    return out.transpose(1, 2)


def coords_mix(rng, n, h2, w2, r):
    """fractional interior points, exact integers, points around every border and points wholly outside"""
    x = rng.uniform(-(r + 3), w2 + r + 2, n)
    y = rng.uniform(-(r + 3), h2 + r + 2, n)
    k = rng.integers(0, 4, n)
    x = np.where(k == 0, rng.uniform(0, w2 - 1, n), x)
    y = np.where(k == 0, rng.uniform(0, h2 - 1, n), y)
    x = np.where(k == 1, np.round(x), x)
    y = np.where(k == 1, np.round(y), y)
    return x, y


@pytest.mark.parametrize("r", [0, 1, 3])
@pytest.mark.parametrize("shape", [(2, 3, 4, 5, 6), (1, 5, 3, 2, 7)])
def test_corr_index_restatement_equals_grid_sample_and_its_autograd(r, shape):
    rng = np.random.default_rng(10 * r + shape[0])
    B, h1, w1, h2, w2 = shape
    P, rd = B * h1 * w1, 2 * r + 1
    vol = rng.normal(0, 1, shape)
    x, y = coords_mix(rng, P, h2, w2, r)
    coords = np.stack([x.reshape(B, h1, w1), y.reshape(B, h1, w1)], 1)
    val, mag, cnt = R.corr_index_forward(vol, coords, r)
    tv = torch.tensor(vol).reshape(P, h2, w2).requires_grad_(True)
    out = sample_planes(tv, torch.tensor(x), torch.tensor(y), r)                     # [P, a, b]
    want = out.detach().numpy().reshape(B, h1, w1, rd, rd).transpose(0, 3, 4, 1, 2)
    np.testing.assert_allclose(val, want, rtol=0, atol=1e-12)
    assert np.all(mag >= np.abs(val) - 1e-12) and cnt.max() <= 4 and cnt.min() == 0 and cnt.max() == 4
    cg = rng.normal(0, 1, val.shape)
    out.backward(torch.tensor(cg.transpose(0, 3, 4, 1, 2).reshape(P, rd, rd).copy()))
    gval, gmag, gcnt = R.corr_index_backward(shape, coords, cg, r)
    np.testing.assert_allclose(gval, tv.grad.numpy().reshape(shape), rtol=0, atol=1e-12)
    assert np.all(gmag >= np.abs(gval) - 1e-12) and gcnt.max() <= 4
    assert np.all((gcnt == 0) == (gmag == 0))


def test_corr_index_output_is_x_offset_major():
    """a volume that is a ramp in w2 only varies along output axis 1 (x offset) and not along axis 2 (y offset)"""
    B, h1, w1, h2, w2, r = 1, 2, 3, 9, 11, 2
    vol = np.broadcast_to(np.arange(w2, dtype=np.float64), (B, h1, w1, h2, w2))
    coords = np.stack([np.full((B, h1, w1), 5.25), np.full((B, h1, w1), 4.5)], 1)
    val, _, _ = R.corr_index_forward(vol, coords, r)
    np.testing.assert_allclose(val[0, :, :, 0, 0], np.broadcast_to((5.25 - r + np.arange(5))[:, None], (5, 5)), atol=1e-12)


@pytest.mark.parametrize("r,N,half", [(0, 1, False), (1, 3, False), (2, 2, True)])
def test_altcorr_restatement_equals_sampling_the_all_pairs_volume(r, N, half):
    rng = np.random.default_rng(7 + r)
    B, H1, W1, C = 2, 4, 6, 8
    H2, W2 = (H1 // 2, W1 // 2) if half else (H1, W1)
    rd = 2 * r + 1
    f1, f2 = rng.normal(0, 1, (B, H1, W1, C)), rng.normal(0, 1, (B, H2, W2, C))
    x, y = coords_mix(rng, B * N * H1 * W1, H2, W2, r)
    coords = np.stack([x, y], -1).reshape(B, N, H1, W1, 2)
    val, mag, cnt = R.altcorr_forward(f1, f2, coords, r)
    t1, t2 = torch.tensor(f1).requires_grad_(True), torch.tensor(f2).requires_grad_(True)
    vol = torch.einsum("bhwc,bklc->bhwkl", t1, t2)                                   # [B,H1,W1,H2,W2]
    planes = vol[:, None].expand(B, N, H1, W1, H2, W2).reshape(-1, H2, W2)
    out = sample_planes(planes, torch.tensor(x), torch.tensor(y), r)                 # [B*N*H1*W1, ax, ay]
    out = out.reshape(B, N, H1, W1, rd * rd).permute(0, 1, 4, 2, 3)                  # index ax * rd + ay
    np.testing.assert_allclose(val, out.detach().numpy(), rtol=0, atol=1e-11)
    assert np.all(mag >= np.abs(val) - 1e-11) and cnt.max() == 4 * C and np.all(cnt % C == 0)
    cg = rng.normal(0, 1, val.shape)
    out.backward(torch.tensor(cg))
    (g1, m1, k1), (g2, m2, k2) = R.altcorr_backward(f1, f2, coords, cg, r)
    np.testing.assert_allclose(g1, t1.grad.numpy(), rtol=0, atol=1e-11)
    np.testing.assert_allclose(g2, t2.grad.numpy(), rtol=0, atol=1e-11)
    assert np.all(m1 >= np.abs(g1) - 1e-11) and np.all(m2 >= np.abs(g2) - 1e-11)
    assert k1.max() <= 4 * N * (rd + 1) ** 2 and k2.sum() == k1.sum()


def test_restatement_treats_unusable_coordinates_as_dead_pixels():
    vol = np.ones((1, 1, 6, 4, 5))
    x = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 2.0])
    coords = np.stack([x.reshape(1, 1, 6), np.full((1, 1, 6), 1.5)], 1)
    for c in (coords, coords[:, ::-1].copy()):
        val, mag, cnt = R.corr_index_forward(vol, c, 1)
        assert np.all(val[..., :5] == 0) and np.all(mag[..., :5] == 0) and np.all(cnt[..., :5] == 0) and np.all(val[..., 5] > 0)


# ---- 3. ABI
def test_header_declares_and_native_binds_the_correlation_entry_points():
    from splat_slam_amd import _native as nat
    txt = open(os.path.join(ROOT, "include", "splat_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ENTRY:
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert name in nat.SIGNATURES
        m = re.search(name + r"\s*\((.*?)\)\s*;", code, flags=re.S)
        assert len(m.group(1).split(",")) == len(nat.SIGNATURES[name][1]), name
    assert "sgr_corr_*" in txt[:txt.index("#ifndef SPLAT_HIP_H_")]          # the entry-point map at the top
    assert os.path.exists(os.path.join(ROOT, "splat_slam_amd", "csrc", "sgr_corr.hip"))
