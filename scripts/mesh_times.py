"""GPU box: HIP-event times of the TSDF mesh (csrc/sgr_mesh.hip) on the 40-frame synthetic room session at 640x480
(voxel 5/512 m, sdf_trunc 0.04, as eval_rendering(mesh=True)): integration per frame (touch + the chunk's one host read +
integrate, in chunks of 16), extraction (sort, count, scan, emit) and cleaning (components, compaction); for scale, the fp64
numpy restatement of tests/mesh_ref.py integrating the first frames on the host.  Writes one JSON file.

    python scripts/mesh_times.py [--out profiles/mesh_times.json] [--reps 5]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
DEV = "cuda:0"


def session_frames(n):
    """renders of the opaque synthetic room from n orbit cameras: frame dicts as TSDFVolume.integrate_frames takes them"""
    from splat_slam_amd import synthetic as syn
    from splat_slam_amd.camera import getWorld2View2
    from splat_slam_amd.mapper import PipelineParams
    from splat_slam_amd.renderer import render
    intr = syn.INTRINSICS["metric"]
    world = syn.room_parameters(60000, seed=43, device=DEV)
    world["scaling"] = world["scaling"] * 0 + world["scaling"].mean(dim=1, keepdim=True) + 1.6
    world["opacity"] = torch.full_like(world["opacity"], 4.0)
    gm = syn.model_from_parameters(world, device=DEV, knn_fn=lambda p: torch.ones(p.shape[0], device=p.device))
    cams = syn.make_views(world, n, intr, DEV, seed=5, perturb=False)
    bg = torch.zeros(3, device=DEV)
    frames = []
    with torch.no_grad():
        for k, cam in enumerate(cams):
            pkg = render(cam, gm, PipelineParams(), bg)
            frames.append(dict(render=pkg["render"].contiguous(), depth=pkg["depth"].contiguous(), gt_depth=cam.depth.contiguous(),
                               w2c=getWorld2View2(cam.R, cam.T).double().cpu(), fx=cam.fx, fy=cam.fy, cx=cam.cx, cy=cam.cy,
                               exposure_a=torch.full((1,), 0.02 * (k % 3), device=DEV) if k else None,
                               exposure_b=torch.full((1,), 0.01, device=DEV) if k else None))
    return frames


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_times.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--host-frames", type=int, default=2)
    args = ap.parse_args()
    from splat_slam_amd.mesh import TSDFVolume, clean_mesh
    frames = session_frames(args.frames)
    runs = []
    for rep in range(args.reps + 1):              # the first run warms up (and sizes the hash and pool from their defaults)
        vol = TSDFVolume(device=DEV)
        t_int, _ = event_ms(lambda: vol.integrate_frames(frames))
        t_ext, mesh = event_ms(vol.extract_triangle_mesh)
        t_cln, clean = event_ms(lambda: clean_mesh(mesh))
        if rep:
            runs.append(dict(integrate_ms=t_int, integrate_per_frame_ms=t_int / len(frames), extract_ms=t_ext, clean_ms=t_cln,
                             units=vol.num_units, vertices=len(mesh), triangles=int(mesh.triangles.shape[0]),
                             clean_vertices=len(clean), clean_triangles=int(clean.triangles.shape[0])))
    med = {k: float(np.median([r[k] for r in runs])) for k in runs[0]}
    import mesh_ref as ref
    host = []
    rv = ref.RefVolume(5.0 / 512.0, 0.04)
    for fr in frames[:args.host_frames]:
        h = {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in fr.items()}
        t0 = time.perf_counter()
        rv.integrate(h)
        host.append((time.perf_counter() - t0) * 1e3)
    out = dict(workload=f"{len(frames)} frames of the synthetic room at 640x480, voxel 5/512 m, sdf_trunc 0.04",
               device=torch.cuda.get_device_name(0), median=med, runs=runs,
               host_numpy_integrate_per_frame_ms=float(np.median(host)), host_frames=len(host))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(dict(median=med, host_numpy_integrate_per_frame_ms=out["host_numpy_integrate_per_frame_ms"])))


if __name__ == "__main__":
    main()
