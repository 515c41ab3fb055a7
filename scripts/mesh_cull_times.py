"""GPU box: HIP-event times of the mesh culling (csrc/sgr_mesh_cull.hip, splat_slam_amd.mesh_cull) for 16 frames at 680 x 1200: each
entry point on the box room of tests/mesh_eval_ref.py at three tessellations (large, medium and several hundred thousand small
triangles), a torch composition of projection plus frustum test next to sgr_cull_project + sgr_cull_visibility, and a whole
evaluate_mesh of the synthetic room session's TSDF mesh against its box walls with and without culling.  Writes one JSON file.

    python scripts/mesh_cull_times.py [--out profiles/mesh_cull_times.json] [--reps 5]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
DEV = "cuda:0"
H, W = 680, 1200
INTR = (600.0, 600.0, 599.5, 339.5)
FRAMES = 16


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def median_ms(fn, reps):
    fn()                                            # warm-up
    return float(np.median([event_ms(fn)[0] for _ in range(reps)]))


def room_mesh_gpu(n):
    import mesh_eval_ref as ref
    from splat_slam_amd.mesh import TriangleMesh
    v, t = ref.room_mesh(n)
    v = torch.from_numpy(v.astype(np.float32)).to(DEV)
    return TriangleMesh(v, torch.from_numpy(t.astype(np.int32)).to(DEV), torch.full_like(v, 0.5))


def torch_frustum(vertices, w2c, intr, near=0.01):
    """the torch composition: fp64 projection of every vertex into every frame and the frustum test, counts per vertex"""
    p = vertices.double()
    cam = torch.einsum("nij,vj->nvi", w2c[:, :, :3], p) + w2c[:, None, :, 3]
    z = cam[..., 2]
    u = intr[:, None, 0] * cam[..., 0] / z + intr[:, None, 2]
    v = intr[:, None, 1] * cam[..., 1] / z + intr[:, None, 3]
    j, i = torch.floor(u + 0.5), torch.floor(v + 0.5)
    ok = (z >= near) & (j >= 0) & (j < W) & (i >= 0) & (i < H)
    return ok.sum(0).to(torch.int32)


def entry_points(mesh, reps):
    import mesh_cull_ref as cref
    from splat_slam_amd import mesh_cull as mc
    c2w = cref.room_cameras(FRAMES)
    w2c, intr = mc.invert_poses(c2w), np.tile(np.asarray(INTR), (FRAMES, 1))
    v, t = mesh.vertices, mesh.triangles
    out = dict(vertices=len(mesh), triangles=int(t.shape[0]))
    out["project_ms"] = median_ms(lambda: mc.project(v, w2c, intr), reps)
    xy, z = mc.project(v, w2c, intr)
    out["raster_ms"] = median_ms(lambda: mc.rasterize(xy, z, t, H, W), reps)
    depth, skipped = mc.rasterize(xy, z, t, H, W)
    out["pixels_hit_fraction"] = float(torch.isfinite(depth).float().mean())
    out["unrasterized_triangles_max"] = int(skipped.max())
    seen = torch.zeros(len(mesh), dtype=torch.int32, device=DEV)
    out["visibility_frustum_ms"] = median_ms(lambda: mc.count_visible(xy, z, None, H, W, seen), reps)
    out["visibility_depth_ms"] = median_ms(lambda: mc.count_visible(xy, z, depth, H, W, seen), reps)
    seen.zero_()
    mc.count_visible(xy, z, depth, H, W, seen)
    out["select_compact_ms"] = median_ms(lambda: mc.select(mesh, seen), reps)
    out["cull_mesh_ms"] = median_ms(lambda: mc.cull_mesh(mesh, c2w, INTR, H, W), reps)
    culled = mc.cull_mesh(mesh, c2w, INTR, H, W)
    out["culled_vertices"], out["culled_triangles"] = len(culled), int(culled.triangles.shape[0])
    # projection + frustum test: the two kernels next to the torch composition (same counts)
    w2c_t, intr_t = torch.from_numpy(w2c).to(DEV), torch.from_numpy(intr).to(DEV)

    def hip():
        a, b = mc.project(v, w2c, intr)
        return mc.count_visible(a, b, None, H, W, torch.zeros(len(mesh), dtype=torch.int32, device=DEV))

    out["project_plus_frustum_ms"] = median_ms(hip, reps)
    out["torch_project_plus_frustum_ms"] = median_ms(lambda: torch_frustum(v, w2c_t, intr_t), reps)
    out["torch_counts_differ"] = int((hip() != torch_frustum(v, w2c_t, intr_t)).sum())
    return out


def session_scores(reps):
    """the room session's TSDF mesh against its box walls (tests/test_gpu_mesh_eval.py), scored whole and culled to its six views"""
    import mesh_eval_ref as ref
    from splat_slam_amd import mesh_cull as mc
    from splat_slam_amd import synthetic as syn
    from splat_slam_amd.eval import _w2c
    from splat_slam_amd.mesh import TriangleMesh
    from splat_slam_amd.mesh_eval import evaluate_mesh
    from test_gpu_mesh_eval import _room_session
    sess = _room_session()
    frames = [sess.loop.viewpoints[k] for k in sorted(sess.loop.viewpoints)]
    pred = sess.evaluate(mesh=True)["mesh"]
    half = np.array(syn.ROOM) / 2
    v, t = ref.box_mesh(-half, half, 64)
    vv = torch.from_numpy(v.astype(np.float32)).to(DEV)
    walls = TriangleMesh(vv, torch.from_numpy(t.astype(np.int32)).to(DEV), torch.full_like(vv, 0.5))
    c2w = [torch.linalg.inv(p) for p in _w2c(frames)]
    intr = [[float(f.fx), float(f.fy), float(f.cx), float(f.cy)] for f in frames]
    h, w = frames[0].original_image.shape[1:]
    keys = ("accuracy", "completion", "precision", "completion_ratio", "fscore", "chamfer_l1")
    out = dict(frames=len(frames), image=[int(h), int(w)], pred_triangles=int(pred.triangles.shape[0]), gt_triangles=int(t.shape[0]))
    res = {}
    out["evaluate_whole_ms"] = median_ms(lambda: res.update(evaluate_mesh(pred, walls)), reps)
    out["metrics_whole"] = {k: res[k] for k in keys}
    out["cull_pred_ms"] = median_ms(lambda: mc.cull_mesh(pred, c2w, intr, h, w), reps)
    out["cull_gt_ms"] = median_ms(lambda: mc.cull_mesh(walls, c2w, intr, h, w), reps)
    pc, pi = mc.cull_mesh(pred, c2w, intr, h, w, return_info=True)
    gc, gi = mc.cull_mesh(walls, c2w, intr, h, w, return_info=True)
    out["pred_triangles_culled"], out["gt_triangles_culled"] = pi["faces_after"], gi["faces_after"]
    out["evaluate_culled_ms"] = median_ms(lambda: res.update(evaluate_mesh(pc, gc)), reps)
    out["metrics_culled"] = {k: res[k] for k in keys}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_cull_times.json"))
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    out = dict(device=torch.cuda.get_device_name(0), frames=FRAMES, image=[H, W], intrinsics=list(INTR))
    # room_mesh(8): 1 152 triangles of up to half a metre, every one a wave's; (64): 73 728; (160): 460 800, most of them a thread's
    out["meshes"] = {f"room_mesh_{n}": entry_points(room_mesh_gpu(n), args.reps) for n in (8, 64, 160)}
    out["room_session"] = session_scores(args.reps)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
