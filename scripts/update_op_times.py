"""GPU box: times of the update operator (splat_slam_amd.update_op, csrc/sgr_update.hip), whole and launch by launch, next to the torch
composition of the same weights (tests/update_ref.TorchUpdate: F.conv2d under torch.autocast, i.e. the vendor convolution library), at a
frontend window (80 edges of 12 source frames, 48 x 64) and at one update_lowmem chunk (40 edges of 8 source frames, 48 x 64); and the
errors of both against the fp64 oracle tests/update_ref.update_ref on the small cases of tests/test_gpu_update_op.py.  HIP-event medians
after a warm-up, everything in this one process.  A single launch is timed on the buffers a whole call has left in scratch.  Writes one
JSON file (rewritten after every section, so a run that is cut short leaves what it measured).

    timeout 900 python scripts/update_op_times.py [--out profiles/update_op_times.json] [--reps 10]"""
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
PEAK_HBM_GB_S = 8000.0

# launch -> (cout, cin, kernel size, runs on the K groups instead of the E edges); None: no matrix work
LAUNCH_CONVS = {"corr_encoder.0": (128, 196, 1, 0), "corr_encoder.2": (128, 128, 3, 0), "flow_encoder.0": (128, 4, 7, 0),
                "flow_encoder.2": (64, 128, 3, 0), "gru.w+gate": (128, 128, 1, 0), "gru.convz|convr": (256, 448, 3, 0),
                "gru.convq+blend": (128, 448, 3, 0), "delta.0|weight.0": (256, 128, 3, 0), "delta.2": (2, 128, 3, 0),
                "weight.2": (2, 128, 3, 0), "agg.conv1": (128, 128, 3, 0), "agg.conv2": (128, 128, 3, 1), "agg.eta": (1, 128, 3, 1),
                "agg.upmask": (576, 128, 1, 1)}


def event_times(fn, reps):
    fn()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return {"ms_median": round(float(np.median(times)), 4), "ms_min": round(float(np.min(times)), 4), "reps": reps}


def errors(op, torch_op, sd16):
    import update_ref as R
    out = {}
    for name, (E, h, w, ii, dtype) in {"3x5x7_f16": (3, 5, 7, [2, 0, 2], torch.float16),
                                       "7x6x8_f32": (7, 6, 8, [4, 1, 4, 1, 9, 4, 0], torch.float32)}.items():
        net, inp, corr, flow = R.make_inputs(E, h, w, seed=100 + E, device=DEV, dtype=dtype)
        ii_t = torch.tensor(ii, device=DEV)
        hip, ref = op(net, inp, corr, flow, ii_t), torch_op(net, inp, corr, flow, ii_t)
        oracle = R.update_ref(sd16, net, inp, corr, flow, torch.tensor(ii))
        out[name] = {}
        for n, a, b, o in zip(("net", "delta", "weight", "eta", "upmask"), hip, ref, oracle):
            da, db = (a.double().cpu() - o).abs(), (b.double().cpu() - o).abs()
            out[name][n] = {"max_hip": float(da.max()), "max_torch": float(db.max()), "rms_hip": float(da.pow(2).mean().sqrt()),
                            "rms_torch": float(db.pow(2).mean().sqrt())}
    return out


def main():
    import update_ref as R
    from splat_slam_amd import update_op as U
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "update_op_times.json"))
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "date": datetime.date.today().isoformat(), "peak_f16_tflops": PEAK_F16_TFLOPS,
           "peak_hbm_gb_per_s": PEAK_HBM_GB_S, "shapes": {}}

    def save():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)

    sd = U.synthetic_state_dict(SEED)
    op, torch_op = U.UpdateOperator.synthetic(SEED, DEV), R.TorchUpdate(sd, DEV)
    res["errors_against_fp64_oracle"] = errors(op, torch_op, R.round_fp16(sd))
    save()
    print("errors recorded", flush=True)
    for name, (E, frames, h, w) in {"frontend_80_edges_48x64": (80, 12, 48, 64), "lowmem_chunk_40_edges_48x64": (40, 8, 48, 64)}.items():
        net, inp, corr, flow = R.make_inputs(E, h, w, seed=E, device=DEV, dtype=torch.float16)
        ii = torch.arange(E, device=DEV) % frames
        r = {"E": E, "K": frames, "h": h, "w": w, "hip": event_times(lambda: op(net, inp, corr, flow, ii), a.reps)}
        print(name, "hip", r["hip"]["ms_median"], "ms", flush=True)
        call, outs, keep = op._prepare(net, inp, corr, flow, ii)
        op._run(call)
        launches, flops_total = {}, 0
        for i, lname in enumerate(U.LAUNCH_NAMES):
            call.first_launch = call.last_launch = i
            t = event_times(lambda: op._run(call), a.reps)
            if lname in LAUNCH_CONVS:
                cout, cin, k, grouped = LAUNCH_CONVS[lname]
                M = (frames if grouped else E) * h * w
                t["gflop"] = round(2.0 * M * cout * cin * k * k / 1e9, 3)
                t["tflops"] = round(t["gflop"] / t["ms_median"], 1)
                t["fraction_of_f16_peak"] = round(t["tflops"] / PEAK_F16_TFLOPS, 4)
                flops_total += t["gflop"]
            launches[lname] = t
        r["launches"] = launches
        r["gflop"] = round(flops_total, 1)
        r["sum_of_launches_ms"] = round(sum(t["ms_median"] for t in launches.values()), 4)
        r["hip_tflops"] = round(flops_total / r["hip"]["ms_median"], 1)
        res["shapes"][name] = r
        save()
        r["torch"] = event_times(lambda: torch_op(net, inp, corr, flow, ii), a.reps)
        r["ratio_hip_over_torch"] = round(r["hip"]["ms_median"] / r["torch"]["ms_median"], 4)
        r["hip_not_slower"] = r["hip"]["ms_median"] <= r["torch"]["ms_median"]
        print(name, "torch", r["torch"]["ms_median"], "ms; ratio", r["ratio_hip_over_torch"], flush=True)
        save()
        del net, inp, corr, flow, call, outs, keep
        torch.cuda.empty_cache()
    print(json.dumps({k: v.get("ratio_hip_over_torch") for k, v in res["shapes"].items()}))


if __name__ == "__main__":
    main()
