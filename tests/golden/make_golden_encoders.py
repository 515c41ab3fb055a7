#!/usr/bin/env python3
"""Generates tests/golden/reference_encoders.npz by INSTANTIATING the reference's BasicEncoder
(thirdparty/glorie_slam/modules/droid_net/extractor.py of the reference checkout) on the CPU in float64, as fnet (out_dim 128,
norm_fn "instance") and cnet (out_dim 256, norm_fn "none"), with the weights of splat_slam_amd.encoder.synthetic_encoder_state_dict(., SEED).
Development machine only; the output is data: one input (fp16-representable, stored as fp16), the two outputs (float64) and the names and
shapes of each module's state dict.  Weights are not recorded: the closed-form rule reproduces them.  extractor.py imports only torch.nn,
so it loads by path.

    python tests/golden/make_golden_encoders.py
"""
import importlib.util
import os
import sys

import numpy as np
import torch

REF = os.environ.get("SPLAT_SLAM_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
SEED = 7

spec = importlib.util.spec_from_file_location("reference_extractor",
                                              os.path.join(REF, "thirdparty", "glorie_slam", "modules", "droid_net", "extractor.py"))
extractor = importlib.util.module_from_spec(spec)
spec.loader.exec_module(extractor)

from splat_slam_amd.encoder import NORM, OUT_DIM, synthetic_encoder_state_dict  # noqa: E402
from encoder_ref import make_images  # noqa: E402

torch.manual_seed(0)
images = make_images(1, 2, 40, 56, seed=11)
out = {"seed": np.array(SEED), "in_images": images.to(torch.float16).numpy()}
for which in ("fnet", "cnet"):
    module = extractor.BasicEncoder(out_dim=OUT_DIM[which], norm_fn=NORM[which]).double().eval()
    module.load_state_dict({k: v.double() for k, v in synthetic_encoder_state_dict(which, SEED).items()})
    with torch.no_grad():
        out["out_" + which] = module(images.double()).numpy()
    sd = module.state_dict()
    out["keys_" + which] = np.array(sorted(sd))
    out["shapes_" + which] = np.array([",".join(str(s) for s in sd[k].shape) for k in sorted(sd)])
path = os.path.join(HERE, "reference_encoders.npz")
np.savez_compressed(path, **out)
print({k: v.shape for k, v in out.items()}, os.path.getsize(path), "bytes")
for which in ("fnet", "cnet"):
    o = out["out_" + which]
    print(which, "rms", float(np.sqrt((o ** 2).mean())), "max", float(np.abs(o).max()))
