#!/usr/bin/env python3
"""Generates tests/golden/reference_update_op.npz by INSTANTIATING the reference's UpdateModule
(thirdparty/glorie_slam/modules/droid_net/droid_net.py:83-153 of the reference checkout, ConvGRU of gru.py, GraphAgg of :48-80) on the CPU in
float64 with the weights of splat_slam_amd.update_op.synthetic_state_dict(SEED).  Development machine only; the output is data: the inputs
(fp16-representable, stored as fp16), the five outputs (float64) and the names and shapes of the module's state dict.  Weights are not
recorded: the closed-form rule reproduces them.  torch_scatter is not installed: scatter_mean is supplied here.

    python tests/golden/make_golden_update.py
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

REF = os.environ.get("SPLAT_SLAM_REFERENCE", "/root/reference")
PKG = "thirdparty.glorie_slam.modules.droid_net"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
SEED = 7


def scatter_mean(src, index, dim):
    n = int(index.max()) + 1
    shape = list(src.shape)
    shape[dim] = n
    total = torch.zeros(shape, dtype=src.dtype).index_add_(dim, index, src)
    count = torch.zeros(n, dtype=src.dtype).index_add_(0, index, torch.ones(index.shape[0], dtype=src.dtype))
    view = [1] * src.dim()
    view[dim] = n
    return total / count.view(view)


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


# the package's __init__ pulls in the correlation extension and the encoders: only the three files the update module needs are loaded
scatter = types.ModuleType("torch_scatter")
scatter.scatter_mean = scatter_mean
sys.modules["torch_scatter"] = scatter
src = os.path.join(REF, *PKG.split("."))
pkg = types.ModuleType(PKG)
pkg.__path__ = [src]
sys.modules[PKG] = pkg
pkg.GradientClip = _load(PKG + ".clipping", os.path.join(src, "clipping.py")).GradientClip
pkg.ConvGRU = _load(PKG + ".gru", os.path.join(src, "gru.py")).ConvGRU
pkg.BasicEncoder = type("BasicEncoder", (), {})
UpdateModule = _load(PKG + ".droid_net", os.path.join(src, "droid_net.py")).UpdateModule

from splat_slam_amd.update_op import synthetic_state_dict  # noqa: E402
from update_ref import make_inputs  # noqa: E402

torch.manual_seed(0)
module = UpdateModule().double().eval()
module.load_state_dict({k: v.double() for k, v in synthetic_state_dict(SEED).items()})
E, h, w = 3, 5, 7
ii = torch.tensor([2, 0, 2])
net, inp, corr, flow = make_inputs(E, h, w, seed=11)
with torch.no_grad():
    outs = module(net.double(), inp.double(), corr.double(), flow.double(), ii, None)
out = {"seed": np.array(SEED), "ii": ii.numpy()}
for name, t in zip(("net", "inp", "corr", "flow"), (net, inp, corr, flow)):
    out["in_" + name] = t.to(torch.float16).numpy()
for name, t in zip(("net", "delta", "weight", "eta", "upmask"), outs):
    out["out_" + name] = t.numpy()
sd = module.state_dict()
out["keys"] = np.array(sorted(sd))
out["shapes"] = np.array([",".join(str(s) for s in sd[k].shape) for k in sorted(sd)])
path = os.path.join(HERE, "reference_update_op.npz")
np.savez_compressed(path, **out)
print({k: v.shape for k, v in out.items()}, os.path.getsize(path), "bytes")
