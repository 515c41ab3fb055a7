"""The parts of splat_slam_amd.update_op that need no GPU: the fp64 oracle tests/update_ref.py against the recorded outputs of the
reference's module and against known answers, the state-dict handling, and the build of the kernels for gfx950."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import update_ref as R
from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_update_op.npz")
OUTS = ("net", "delta", "weight", "eta", "upmask")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_oracle_equals_the_recorded_outputs_of_the_reference_module():
    """both sides are fp64 sums of at most 4032 terms of order 1: 1e-12 of rounding, held to 1e-9"""
    from splat_slam_amd import update_op as U
    g = np.load(GOLDEN)
    assert tuple(g["in_net"].shape) == (1, 3, 128, 5, 7) and g["ii"].tolist() == [2, 0, 2]
    sd = U.synthetic_state_dict(int(g["seed"]))
    ins = [torch.from_numpy(g["in_" + n].astype(np.float32)) for n in ("net", "inp", "corr", "flow")]
    outs = R.update_ref(sd, *ins, torch.from_numpy(g["ii"]))
    for n, o in zip(OUTS, outs):
        ref = g["out_" + n]
        assert ref.dtype == np.float64 and tuple(o.shape) == ref.shape, n
        assert np.abs(o.numpy() - ref).max() <= 1e-9, n
    assert np.abs(g["out_net"]).max() > 0.5 and np.abs(g["out_upmask"]).max() > 0.05     # (not a comparison of zeros)


def test_fixture_lists_exactly_the_keys_the_operator_requires():
    from splat_slam_amd import update_op as U
    g = np.load(GOLDEN)
    recorded = {k: tuple(int(s) for s in sh.split(",")) for k, sh in zip(g["keys"].tolist(), g["shapes"].tolist())}
    assert recorded == U.LAYER_SHAPES
    assert os.path.getsize(GOLDEN) <= 661363


def test_synthetic_weights_follow_their_closed_form_rule():
    from splat_slam_amd import update_op as U
    a, b, c = U.synthetic_state_dict(7), U.synthetic_state_dict(7), U.synthetic_state_dict(8)
    assert set(a) == set(U.LAYER_SHAPES)
    for k, shape in U.LAYER_SHAPES.items():
        assert a[k].dtype == torch.float32 and tuple(a[k].shape) == shape and torch.equal(a[k], b[k]) and not torch.equal(a[k], c[k])
    w = a["gru.convz.weight"]
    bound = 1 / np.sqrt(448 * 9)
    assert float(w.abs().max()) <= bound and float(w.abs().max()) > 0.99 * bound and abs(float(w.mean())) < 0.01 * bound
    assert abs(float(w.std()) - bound / np.sqrt(3)) < 0.01 * bound
    assert not torch.equal(a["gru.convz.weight"], a["gru.convr.weight"])
    # one element by hand: the murmur3 finaliser of (index * 0x9E3779B1 + FNV-1a(name) + seed * 0x85EBCA77)
    name, idx = "delta.2.bias", 1
    h = 2166136261
    for ch in name.encode():
        h = ((h ^ ch) * 16777619) & 0xFFFFFFFF
    x = (idx * 0x9E3779B1 + h + 7 * 0x85EBCA77) & 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & 0xFFFFFFFF
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & 0xFFFFFFFF
    x ^= x >> 16
    assert float(a[name][idx]) == np.float32((x / 2.0 ** 31 - 1.0) / np.sqrt(128 * 9))


def _case(E=2, h=4, w=5, seed=1):
    from splat_slam_amd import update_op as U
    return U.synthetic_state_dict(3), R.make_inputs(E, h, w, seed)


def test_oracle_update_gate_closed_leaves_net_unchanged():
    sd, (net, inp, corr, flow) = _case()
    sd["gru.convz.bias"] = torch.full((128,), -40.0)
    out = R.update_ref(sd, net, inp, corr, flow)
    assert len(out) == 3 and (out[0] - net.double()).abs().max() < 1e-12


def test_oracle_update_gate_open_with_zero_convq_gives_tanh_of_the_bias_and_global_term():
    sd, (net, inp, corr, flow) = _case()
    sd["gru.convz.bias"] = torch.full((128,), 40.0)
    sd["gru.convq.weight"] = torch.zeros_like(sd["gru.convq.weight"])
    out = R.update_ref(sd, net, inp, corr, flow)[0]
    n = net[0].double()
    gate = torch.sigmoid(torch.einsum("oc,echw->eohw", sd["gru.w.weight"][:, :, 0, 0].double(), n) + sd["gru.w.bias"].double()[None, :, None, None])
    glo = (gate * n).mean(dim=(2, 3))
    glo_q = glo @ sd["gru.convq_glo.weight"][:, :, 0, 0].double().T + sd["gru.convq_glo.bias"].double()
    want = torch.tanh(sd["gru.convq.bias"].double()[None] + glo_q)[:, :, None, None].expand_as(n)
    assert (out[0] - want).abs().max() < 1e-12


def test_oracle_segmented_mean_equals_a_loop():
    x = torch.randn(5, 3, 2, dtype=torch.float64)
    ii = [2, 0, 2, 5, 0]
    got = R.segmented_mean(x, ii)
    assert tuple(got.shape) == (3, 3, 2)
    for k, g in enumerate([0, 2, 5]):
        acc, cnt = torch.zeros(3, 2, dtype=torch.float64), 0
        for e in range(5):
            if ii[e] == g:
                acc, cnt = acc + x[e], cnt + 1
        assert torch.allclose(got[k], acc / cnt, rtol=0, atol=1e-15)


def test_oracle_flow_none_is_zero_flow():
    sd, (net, inp, corr, flow) = _case()
    ii = torch.tensor([1, 1])
    a, b = R.update_ref(sd, net, inp, corr, None, ii), R.update_ref(sd, net, inp, corr, torch.zeros_like(flow), ii)
    assert len(a) == 5 and all(torch.equal(x, y) for x, y in zip(a, b))


def test_state_dict_prefixes_slicing_and_errors():
    from splat_slam_amd import update_op as U
    sd = U.synthetic_state_dict(1)
    for prefix in ("", "update.", "module.update.", "module."):
        ck = {prefix + k: v for k, v in sd.items()}
        ck["module.fnet.conv1.weight" if prefix.startswith("module.") else "cnet.conv1.weight"] = torch.zeros(3)
        out = U.normalize_state_dict(ck)
        assert set(out) == set(U.LAYER_SHAPES) and all(torch.equal(out[k], sd[k]) for k in sd)
    ck = {"module.update." + k: v for k, v in sd.items()}
    for name in ("weight.2", "delta.2"):
        ck[f"module.update.{name}.weight"] = torch.cat([sd[name + ".weight"], torch.ones(1, 128, 3, 3)])
        ck[f"module.update.{name}.bias"] = torch.cat([sd[name + ".bias"], torch.ones(1)])
    out = U.normalize_state_dict(ck)
    assert all(torch.equal(out[k], sd[k]) for k in sd)
    # errors come from the validation, before the device is looked at: these run on a machine without a GPU
    missing = {k: v for k, v in sd.items() if k != "gru.w.bias"}
    with pytest.raises(ValueError, match="gru.w.bias"):
        U.UpdateOperator.from_state_dict(missing)
    with pytest.raises(ValueError, match="unexpected key 'gru.convx.weight'"):
        U.UpdateOperator.from_state_dict({**sd, "gru.convx.weight": torch.zeros(1)})
    with pytest.raises(ValueError, match="shape"):
        U.UpdateOperator.from_state_dict({**sd, "agg.eta.0.weight": torch.zeros(3, 128, 3, 3)})   # only weight.2 / delta.2 are sliced
    with pytest.raises(ValueError, match="shape"):
        U.UpdateOperator.from_state_dict({**sd, "corr_encoder.0.weight": torch.zeros(128, 195, 1, 1)})


CONV_KERNELS = re.compile(r"conv_kernelILi[137]ELi(16|64)E")


def test_update_kernels_compile_for_gfx950_without_scratch(tmp_path):
    """the convolution kernels keep their accumulators in registers: no private segment, no spills (VGPR counts: DESIGN.md section 3)"""
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("hipcc not available")
    out = str(tmp_path / "update.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-S", "--cuda-device-only", "-o", out,
                    os.path.join(ROOT, "splat_slam_amd", "csrc", "sgr_update.hip")], check=True, capture_output=True)
    text = open(out).read()
    assert "v_mfma_f32_16x16x32_f16" in text
    seen = 0
    for block in text.split("\n  - ")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if not name or not CONV_KERNELS.search(name.group(1)):
            continue
        seen += 1
        vgpr = int(re.search(r"\.vgpr_count:\s+(\d+)", block).group(1))
        spill = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", block).group(1))
        scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1))
        print(name.group(1), "vgpr", vgpr)
        ceiling = {"16": 60, "64": 108}[CONV_KERNELS.search(name.group(1)).group(1)]       # BN -> the count when it was written
        assert scratch == 0 and spill == 0 and vgpr <= ceiling, (name.group(1), vgpr, spill, scratch)
    assert seen == 6
    from splat_slam_amd import _native as nat
    lib = nat.lib()
    assert lib.sgr_update_scratch_bytes(0, 0, 6, 8) == 0 and lib.sgr_update_scratch_bytes(3, 4, 6, 8) == 0
    small, big = lib.sgr_update_scratch_bytes(3, 2, 5, 7), lib.sgr_update_scratch_bytes(80, 12, 48, 64)
    assert small >= 3 * 35 * 2 * (448 + 200 + 8 + 128 + 256 + 128) and big > small and small % 16 == 0
