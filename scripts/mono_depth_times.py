"""GPU box: times of the mono-depth prior (splat_slam_amd.mono_depth, splat_slam_amd.vit, csrc/sgr_vit.hip) next to the torch composition
of the same weights in fp16 (tests/vit_ref.TorchVit and tests/mono_depth_ref.TorchMonoDepth: F.linear and F.conv2d under torch.autocast,
i.e. the vendor libraries, and F.scaled_dot_product_attention): the whole transformer at dim 768, depth 12, 1025 tokens, one image, whole
and launch by launch, and a whole predict of a 480 x 640 image through the default network.  HIP-event medians after a warm-up, the
two sides alternating in this one process on the same card.  A single launch is timed on the buffers a whole call has left in scratch.
Then MonoDepth's two backbones, "torch" (the default) and "hip" (splat_slam_amd.resnetv2, csrc/sgr_resnet.hip): the backbone alone and a
whole predict, the two variants alternating, with the spread of the repeats, the difference of the two predict outputs, and the HIP
backbone launch by launch with the bytes and operations its shapes imply.
Then MonoDepth's two decoders, "torch" (the default) and "hip" (splat_slam_amd.dpt_decoder, csrc/sgr_dpt.hip), both on backbone="hip": a
whole predict, the decoder alone on the same taps and stage maps, and each resize of predict, the two variants alternating with the same
spread rule; then the 35 launches of the HIP decoder one by one with bytes, operations and workgroups from the shapes (key
decoder_torch_vs_hip; --only decoder measures this leg alone and keeps the other keys of the output file as they are).
Writes one JSON file (rewritten after every section, so a run that is cut short leaves what it measured).

    timeout 900 python scripts/mono_depth_times.py [--out profiles/mono_depth_times.json] [--reps 10] [--only decoder]"""
import argparse
import datetime
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
DEV = "cuda:0"
SEED = 7
PEAK_F16_TFLOPS = 2500.0         # MI355X dense fp16 matrix peak
PEAK_HBM_TBS = 8.0               # MI355X HBM3E peak bandwidth (spec)


def one_time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def summary(times):
    return {"ms_median": round(float(np.median(times)), 4), "ms_min": round(float(np.min(times)), 4), "reps": len(times)}


def alternating(hip, ref, reps):
    """warm both, then hip, torch, hip, torch, ...: a drift of the card's clock falls on both sides alike"""
    hip(), ref(), hip(), ref()
    th, tr = [], []
    for _ in range(reps):
        th.append(one_time(hip))
        tr.append(one_time(ref))
    r = {"hip": summary(th), "torch": summary(tr)}
    r["ratio_hip_over_torch"] = round(r["hip"]["ms_median"] / r["torch"]["ms_median"], 4)
    r["hip_not_slower"] = r["hip"]["ms_median"] <= r["torch"]["ms_median"]
    return r


def two_variants(torch_fn, hip_fn, reps):
    """warm both, then torch, hip, torch, hip, ...; the spread of a variant is the distance between the quartiles of its repeats, and
    the hip variant counts as faster only when the medians differ by more than the larger spread"""
    torch_fn(), hip_fn(), torch_fn(), hip_fn()
    tt, th = [], []
    for _ in range(reps):
        tt.append(one_time(torch_fn))
        th.append(one_time(hip_fn))
    iqr = lambda t: float(np.percentile(t, 75) - np.percentile(t, 25))
    r = {"torch": summary(tt), "hip": summary(th), "spread_ms": round(max(iqr(tt), iqr(th)), 4)}
    r["torch"]["ms_max"], r["hip"]["ms_max"] = round(float(np.max(tt)), 4), round(float(np.max(th)), 4)
    r["ratio_hip_over_torch"] = round(r["hip"]["ms_median"] / r["torch"]["ms_median"], 4)
    r["hip_faster_beyond_the_spread"] = r["torch"]["ms_median"] - r["hip"]["ms_median"] > r["spread_ms"]
    return r


def backbone_launch_model(cfg, B, H, W):
    """launch name -> (bytes, GFLOP) of sgr_resnet_forward from the shapes alone: every map read once and written once (taps re-read
    through the caches are not counted), the packed weights once, the statistics once"""
    from splat_slam_amd import resnetv2 as RN
    out, tile = {}, 128
    groups = cfg.gn_groups

    def conv(name, norm, cin, cout, k, h, w, stride, residual=False):
        ho, wo = -(-h // stride), -(-w // stride)
        k_pad = -(-k * k * cin // 32) * 32
        stats = B * -(-ho * wo // tile) * groups * 16
        out[name] = (B * h * w * cin * 2 + cout * k_pad * 2 + B * ho * wo * cout * 4 + stats, 2.0 * B * ho * wo * cout * k * k * cin / 1e9)
        out[norm] = (B * ho * wo * cout * (4 + 2 + (2 if residual else 0)) + stats + cout * 8, 0.0)
        return ho, wo

    out["pack"] = (B * H * W * (3 * 2 + 8 * 2), 0.0)
    h, w = conv("stem.conv", "stem.norm", 8, cfg.stem_chs, 7, H, W, 2)
    out["pool"] = (B * h * w * cfg.stem_chs * 2 + B * (h // 2) * (w // 2) * cfg.stem_chs * 2, 0.0)
    h, w, cin = h // 2, w // 2, cfg.stem_chs
    for s, (cout, n) in enumerate(zip(cfg.stage_chs, cfg.stage_layers)):
        for blk in range(n):
            p, stride, mid = f"stages.{s}.blocks.{blk}.", 2 if s > 0 and blk == 0 else 1, cout // 4
            conv(p + "conv1", p + "norm1", cin, mid, 1, h, w, 1)
            if blk == 0:
                conv(p + "downsample.conv", p + "downsample.norm", cin, cout, 1, h, w, stride)
            ho, wo = conv(p + "conv2", p + "norm2", mid, mid, 3, h, w, stride)
            conv(p + "conv3", p + "norm3", mid, cout, 1, ho, wo, 1, True)
            h, w, cin = ho, wo, cout
    assert tuple(out) == RN.LAUNCH_NAMES(cfg)
    return out


def decoder_launch_model(cfg, B, H, W):
    """launch name -> (bytes, GFLOP, workgroups) of sgr_dpt_forward from the shapes alone: every map read once and written once (taps
    re-read through the caches are not counted), residuals read once, the packed weights once"""
    from splat_slam_amd import dpt_decoder as DD
    D, f, out = cfg.dim, cfg.features, {}
    gh, gw = H // 16, W // 16

    def conv(name, cin, cout, k, h, w, nres=0, stride=1, out_bytes=2):
        ho, wo = h // stride, w // stride
        k_pad = -(-k * k * cin // 32) * 32
        bn = 64 if cout % 64 == 0 else 32 if cout % 32 == 0 else 16
        tiles = B * -(-ho * wo // 128) if stride == 2 else -(-B * ho * wo // 128)
        out[name] = (B * h * w * cin * 2 + -(-cout // 64) * 64 * k_pad * 2 + B * ho * wo * cout * (out_bytes + 2 * nres),
                     2.0 * B * ho * wo * cout * k * k * cin / 1e9, tiles * -(-cout // bn))

    def up2(name, h, w, C):
        out[name] = (B * h * w * C * 2 * 5, 0.0, -(-B * h * w * 4 * (C // 8) // 256))

    out["pack3"] = (B * gh * gw * D * 4, 0.0, 0)
    conv("act_postprocess3.3", D, D, 1, gh, gw)
    out["pack4"] = (B * gh * gw * D * 4, 0.0, 0)
    conv("act_postprocess4.3", D, D, 1, gh, gw)
    conv("act_postprocess4.4", D, D, 3, gh, gw, stride=2)
    for i, cin in enumerate((cfg.stage_chs[0], cfg.stage_chs[1], D, D)):
        conv(f"layer{i + 1}_rn", cin, f, 3, H >> (2 + i), W >> (2 + i))
    for i in (4, 3, 2, 1):
        h, w, p = H >> (1 + i), W >> (1 + i), f"refinenet{i}."
        if i < 4:
            conv(p + "resConfUnit1.conv1", f, f, 3, h, w)
            conv(p + "resConfUnit1.conv2", f, f, 3, h, w, 2)
        conv(p + "resConfUnit2.conv1", f, f, 3, h, w)
        conv(p + "resConfUnit2.conv2", f, f, 3, h, w, 1)
        up2(p + "up2", h, w, f)
        conv(p + "out_conv", f, f, 1, 2 * h, 2 * w)
    conv("output_conv.0", f, f // 2, 3, H // 2, W // 2)
    up2("head.up2", H // 2, W // 2, f // 2)
    conv("output_conv.2", f // 2, 32, 3, H, W)
    conv("output_conv.4", 32, 1, 1, H, W, out_bytes=4)
    assert tuple(out) == DD.LAUNCH_NAMES(cfg)
    return out


def torch_decoder(m, tap3, tap4, l1, l2, B, H, W):
    """the decoder of MonoDepth.forward with decoder="torch", backbone="hip", on given taps and stage maps: the same calls in the same
    order"""
    from splat_slam_amd.mono_depth import _up2
    c = m._c
    r4 = m._down(c["pretrained.act_postprocess4.3"](tap4))
    skip2 = c["scratch.layer2_rn"].packed(l2, B, H // 8, W // 8)
    skip1 = c["scratch.layer1_rn"].packed(l1, B, H // 4, W // 4)
    r3 = c["pretrained.act_postprocess3.3"](tap3)
    path = m._fusion(4, c["scratch.layer4_rn"](r4))
    path = m._fusion(3, path, c["scratch.layer3_rn"](r3))
    path = m._fusion(2, path, skip2)
    path = m._fusion(1, path, skip1)
    y = c["scratch.output_conv.2"](_up2(c["scratch.output_conv.0"](path)), "relu")
    return c["scratch.output_conv.4"](y, "relu", torch.float32)[:, 0]


def decoder_leg(res, save, reps):
    """decoder="torch" against decoder="hip", both on backbone="hip": whole predict and the decoder alone, alternating; then the 35
    launches and the two resizes one by one on the buffers of a whole call"""
    import torch.nn.functional as F
    from splat_slam_amd import dpt_decoder as DD
    from splat_slam_amd import mono_depth as MD
    mcfg = MD.MonoDepthConfig()
    sd = MD.synthetic_state_dict(SEED, mcfg)
    ref = MD.MonoDepth.from_state_dict(sd, mcfg, DEV, backbone="hip", decoder="torch")
    hip = MD.MonoDepth.from_state_dict(sd, mcfg, DEV, backbone="hip", decoder="hip")
    del sd
    image = torch.rand(1, 3, 480, 640, generator=torch.Generator().manual_seed(2)).to(DEV)
    H, W = mcfg.net_size
    d = {"net_size": [H, W], "image": [480, 640], "backbone": "hip"}
    d["predict"] = two_variants(lambda: ref.predict(image), lambda: hip.predict(image), reps)
    d["max_abs_difference_of_the_two_predicts"] = float((ref.predict(image) - hip.predict(image)).abs().max())
    x = DD.resize_in(image, (H, W))
    l1, l2, l3 = hip.backbone.channels_last(x)
    tap3, tap4 = hip.vit.tokens(l3, H // 16, W // 16)
    d["decoder"] = two_variants(lambda: torch_decoder(ref, tap3, tap4, l1, l2, 1, H, W), lambda: hip.dpt(tap3, tap4, l1, l2, H, W), reps)
    d["max_abs_difference_of_the_two_decoders"] = float((torch_decoder(ref, tap3, tap4, l1, l2, 1, H, W) - hip.dpt(tap3, tap4, l1, l2, H, W)).abs().max())
    depth = hip.dpt(tap3, tap4, l1, l2, H, W)[0]
    torch_in = lambda: ((F.interpolate(image, size=(H, W), mode="bilinear", align_corners=False, antialias=True) - 0.5) / 0.5).to(torch.float16)
    torch_out = lambda: F.interpolate(depth.clamp(0, 1)[None, None], size=(480, 640), mode="bicubic").clamp(0, 1)[0, 0]
    d["resize_in"] = two_variants(torch_in, lambda: DD.resize_in(image, (H, W)), reps)
    d["resize_out"] = two_variants(torch_out, lambda: DD.resize_out(depth, (480, 640)), reps)
    res["decoder_torch_vs_hip"] = d
    save()
    print("predict torch", d["predict"]["torch"]["ms_median"], "hip", d["predict"]["hip"]["ms_median"], "spread", d["predict"]["spread_ms"],
          "; decoder torch", d["decoder"]["torch"]["ms_median"], "hip", d["decoder"]["hip"]["ms_median"], "spread", d["decoder"]["spread_ms"], flush=True)
    call, _ = hip.dpt._prepare(tap3, tap4, l1, l2, H, W)
    hip.dpt._run(call)
    model_of = decoder_launch_model(mcfg, 1, H, W)
    launches = {}
    for i, name in enumerate(DD.LAUNCH_NAMES(mcfg)):
        call.first_launch = call.last_launch = i
        hip.dpt._run(call)
        t = summary([one_time(lambda: hip.dpt._run(call)) for _ in range(reps)])
        nbytes, gflop, groups = model_of[name]
        t_bytes, t_flop = nbytes / (PEAK_HBM_TBS * 1e12) * 1e3, gflop / PEAK_F16_TFLOPS
        t.update({"mbytes": round(nbytes / 1e6, 3), "gflop": round(gflop, 4), "workgroups": groups, "bound": "bytes" if t_bytes >= t_flop else "mfma",
                  "ms_at_the_bound": round(max(t_bytes, t_flop), 5), "share_of_the_bound": round(max(t_bytes, t_flop) / t["ms_median"], 4)})
        launches[name] = t
    d["hip_launches"] = launches
    d["hip_sum_of_launches_ms"] = round(sum(t["ms_median"] for t in launches.values()), 4)
    d["hip_gflop"], d["hip_mbytes"] = round(sum(v[1] for v in model_of.values()), 2), round(sum(v[0] for v in model_of.values()) / 1e6, 1)
    d["peak_hbm_tbs"] = PEAK_HBM_TBS
    save()
    print("decoder launches", {k: v["ms_median"] for k, v in launches.items()}, flush=True)


def hold_fp16(params):
    """the torch side keeps its matrices and kernels in fp16, so that autocast casts no weight inside the timed call"""
    for k, v in params.items():
        if v.dim() >= 2 and not k.endswith(("cls_token", "pos_embed")):
            params[k] = v.to(torch.float16)


def launch_gflop(name, B, T, D, cin):
    """the matrix work of one launch of sgr_vit_forward"""
    M, kind = B * T, name.rsplit(".", 1)[-1]
    if name == "embed":
        return 2.0 * B * (T - 1) * D * cin / 1e9
    if kind in ("qkv", "fc1", "fc2", "proj"):
        return 2.0 * M * D * D * {"qkv": 3, "fc1": 4, "fc2": 4, "proj": 1}[kind] / 1e9
    if kind == "attention":
        return 4.0 * B * T * T * D / 1e9
    if name.startswith("readout"):
        return 2.0 * (B if kind == "cls" else M) * D * D / 1e9
    return 0.0


def main():
    import mono_depth_ref as MR
    import vit_ref as VR
    from splat_slam_amd import mono_depth as MD
    from splat_slam_amd import vit as V
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mono_depth_times.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", choices=("all", "decoder"), default="all",
                    help="decoder: keep what the output file holds and (re)write its key decoder_torch_vs_hip alone")
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "date": datetime.date.today().isoformat(), "peak_f16_tflops": PEAK_F16_TFLOPS}

    def save():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)

    if a.only == "decoder":
        if os.path.exists(a.out):
            with open(a.out) as fh:
                res = json.load(fh)
        decoder_leg(res, save, a.reps)
        res["decoder_torch_vs_hip"]["device"], res["decoder_torch_vs_hip"]["date"] = torch.cuda.get_device_name(0), datetime.date.today().isoformat()
        save()
        return

    # ---- the whole transformer ----
    cfg = V.VitConfig()
    sd = V.synthetic_state_dict(SEED, cfg)
    vit, torch_vit = V.VisionTransformer.from_state_dict(sd, cfg, DEV), VR.TorchVit(VR.round_fp16(sd), cfg, DEV)
    hold_fp16(torch_vit.p)
    B, gh, gw = 1, 32, 32
    T = 1 + gh * gw
    x = torch.relu(torch.randn(B, cfg.cin, gh, gw, generator=torch.Generator().manual_seed(1))).half().to(DEV)
    r = {"B": B, "T": T, "dim": cfg.dim, "depth": cfg.depth, "heads": cfg.heads}
    r.update(alternating(lambda: vit(x), lambda: torch_vit(x), a.reps))
    print("vit", r["hip"]["ms_median"], "ms; torch", r["torch"]["ms_median"], "ms; ratio", r["ratio_hip_over_torch"], flush=True)
    res["vit_768x12_T1025_B1"] = r
    save()
    call, outs, keep = vit._prepare(x)
    vit._run(call)
    launches, by_kind, total = {}, {}, 0.0
    for i, name in enumerate(V.launch_names(cfg.depth)):
        call.first_launch = call.last_launch = i
        vit._run(call)
        t = summary([one_time(lambda: vit._run(call)) for _ in range(a.reps)])
        gf = launch_gflop(name, B, T, cfg.dim, cfg.cin)
        if gf:
            t["gflop"], t["tflops"] = round(gf, 3), round(gf / t["ms_median"], 1)
            t["fraction_of_f16_peak"] = round(t["tflops"] / PEAK_F16_TFLOPS, 4)
        total += gf
        launches[name] = t
        kind = name.rsplit(".", 1)[-1] if name.startswith("blocks.") else name
        by_kind[kind] = round(by_kind.get(kind, 0.0) + t["ms_median"], 4)
    r["launches"], r["ms_by_kind_of_launch"] = launches, by_kind
    r["gflop"], r["sum_of_launches_ms"] = round(total, 1), round(sum(t["ms_median"] for t in launches.values()), 4)
    r["hip_tflops"] = round(total / r["hip"]["ms_median"], 1)
    save()
    print("by kind", by_kind, flush=True)
    del vit, torch_vit, call, outs, keep, sd
    torch.cuda.empty_cache()

    # ---- a whole predict ----
    mcfg = MD.MonoDepthConfig()
    sd = MD.synthetic_state_dict(SEED, mcfg)
    model, torch_model = MD.MonoDepth.from_state_dict(sd, mcfg, DEV), MR.TorchMonoDepth(MR.prepare(sd), mcfg, DEV)
    hold_fp16(torch_model.p), hold_fp16(torch_model.vit.p)
    image = torch.rand(1, 3, 480, 640, generator=torch.Generator().manual_seed(2)).to(DEV)
    p = {"image": [480, 640], "net_size": list(mcfg.net_size)}
    p.update(alternating(lambda: model.predict(image), lambda: MR.predict_by_hand(torch_model, image), a.reps))
    xn = torch.rand(1, 3, *mcfg.net_size, generator=torch.Generator().manual_seed(3)).half().to(DEV)
    p["backbone_torch_fp16"] = summary([one_time(lambda: model.backbone(xn)) for _ in range(a.reps + 1)][1:])
    d = (model.predict(image) - MR.predict_by_hand(torch_model, image)).abs()
    p["max_abs_difference_hip_torch"] = float(d.max())
    res["predict_480x640"] = p
    save()
    print("predict", p["hip"]["ms_median"], "ms; torch", p["torch"]["ms_median"], "ms; ratio", p["ratio_hip_over_torch"], flush=True)

    # ---- the two backbones of MonoDepth: "torch" (the default) and "hip" (csrc/sgr_resnet.hip), alternating in this process ----
    from splat_slam_amd import resnetv2 as RN
    hip_model = MD.MonoDepth.from_state_dict(sd, mcfg, DEV, backbone="hip")
    del sd
    b = {"net_size": list(mcfg.net_size), "image": [480, 640]}
    b["backbone"] = two_variants(lambda: model.backbone(xn), lambda: hip_model.backbone(xn), a.reps)
    b["predict"] = two_variants(lambda: model.predict(image), lambda: hip_model.predict(image), a.reps)
    b["max_abs_difference_of_the_two_predicts"] = float((model.predict(image) - hip_model.predict(image)).abs().max())
    res["backbone_torch_vs_hip"] = b
    p["backbone_hip"] = b["backbone"]["hip"]
    save()
    print("backbone torch", b["backbone"]["torch"]["ms_median"], "hip", b["backbone"]["hip"]["ms_median"], "spread", b["backbone"]["spread_ms"],
          "; predict torch", b["predict"]["torch"]["ms_median"], "hip", b["predict"]["hip"]["ms_median"], "spread", b["predict"]["spread_ms"], flush=True)
    net = hip_model.backbone
    call, outs = net._prepare(xn)
    net._run(call)
    model_of = backbone_launch_model(mcfg, 1, *mcfg.net_size)
    launches, by_kind = {}, {}
    for i, name in enumerate(RN.LAUNCH_NAMES(mcfg)):
        call.first_launch = call.last_launch = i
        net._run(call)
        t = summary([one_time(lambda: net._run(call)) for _ in range(a.reps)])
        nbytes, gflop = model_of[name]
        t_bytes, t_flop = nbytes / (PEAK_HBM_TBS * 1e12) * 1e3, gflop / PEAK_F16_TFLOPS
        t.update({"mbytes": round(nbytes / 1e6, 3), "gflop": round(gflop, 4), "bound": "bytes" if t_bytes >= t_flop else "mfma",
                  "ms_at_the_bound": round(max(t_bytes, t_flop), 5), "share_of_the_bound": round(max(t_bytes, t_flop) / t["ms_median"], 4)})
        launches[name] = t
        kind = name.rsplit(".", 1)[-1] if name.startswith("stages.") else name
        k = by_kind.setdefault(kind, {"ms": 0.0, "mbytes": 0.0, "gflop": 0.0, "launches": 0})
        k["ms"], k["mbytes"], k["gflop"], k["launches"] = round(k["ms"] + t["ms_median"], 4), round(k["mbytes"] + t["mbytes"], 3), \
            round(k["gflop"] + gflop, 4), k["launches"] + 1
    b["hip_launches"], b["hip_by_kind_of_launch"] = launches, by_kind
    b["hip_sum_of_launches_ms"] = round(sum(t["ms_median"] for t in launches.values()), 4)
    b["hip_gflop"], b["hip_mbytes"] = round(sum(v[1] for v in model_of.values()), 2), round(sum(v[0] for v in model_of.values()) / 1e6, 1)
    b["peak_hbm_tbs"] = PEAK_HBM_TBS
    save()
    print("backbone by kind", by_kind, flush=True)
    del model, torch_model, hip_model, net, call, outs
    torch.cuda.empty_cache()
    decoder_leg(res, save, a.reps)
    print(json.dumps({k: v.get("ratio_hip_over_torch") for k, v in res.items() if isinstance(v, dict)}))


if __name__ == "__main__":
    main()
