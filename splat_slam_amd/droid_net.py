"""The three networks of the tracker (DroidNet of the reference's thirdparty/glorie_slam/modules/droid_net/droid_net.py) behind one object,
filled from one checkpoint dict: `fnet` and `cnet` (splat_slam_amd.encoder.Encoder) and `update` (splat_slam_amd.update_op.UpdateOperator).

    DroidNet.from_state_dict(sd, device="cuda")      keys "fnet.*", "cnet.*" and "update.*", each optionally behind "module."
    DroidNet.synthetic(seed, device="cuda")          weights of synthetic_state_dict(seed)
    synthetic_state_dict(seed)                       the three synthetic dicts under their prefixes
"""
from splat_slam_amd import update_op
from splat_slam_amd.encoder import Encoder, normalize_encoder_state_dict, synthetic_encoder_state_dict

__all__ = ["DroidNet", "synthetic_state_dict"]


def synthetic_state_dict(seed):
    sd = {"update." + k: v for k, v in update_op.synthetic_state_dict(seed).items()}
    for which in ("fnet", "cnet"):
        sd.update({which + "." + k: v for k, v in synthetic_encoder_state_dict(which, seed).items()})
    return sd


class DroidNet:
    def __init__(self, sd, device="cuda"):
        def part(prefix):
            out = {}
            for key, v in sd.items():
                k = key[len("module."):] if key.startswith("module.") else key
                if k.startswith(prefix):
                    out[k] = v
            return out
        unknown = [k for k in sd if not (k[len("module."):] if k.startswith("module.") else k).startswith(("fnet.", "cnet.", "update."))]
        if unknown:
            raise ValueError(f"droid_net: keys outside fnet.*, cnet.* and update.*: {unknown}")
        # all three are validated before anything is built, so that a bad checkpoint raises without touching a device
        fnet, cnet = (normalize_encoder_state_dict(part(which + "."), which) for which in ("fnet", "cnet"))
        update = update_op.normalize_state_dict(part("update."))
        self.fnet, self.cnet = Encoder(fnet, "fnet", device), Encoder(cnet, "cnet", device)
        self.update = update_op.UpdateOperator(update, device)
        self.device = self.update.device

    @classmethod
    def from_state_dict(cls, sd, device="cuda"):
        return cls(sd, device)

    @classmethod
    def synthetic(cls, seed, device="cuda"):
        return cls(synthetic_state_dict(seed), device)
