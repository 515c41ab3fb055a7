"""numpy restatement of the mesh culling of splat_slam_amd.mesh_cull ("Mesh culling"): the projection in fp64
with the kernel's order of operations, the exact integer rasteriser (int64 edge functions, fp64 depth), the visibility rule in
single fp32 operations, and the selection.  Tests only."""
import numpy as np

SUB = 256                       # snapped units per pixel (SGR_CULL_SUBPIXEL_BITS = 8)
GUARD = 16384.0                 # SGR_CULL_GUARD_PIXELS


def invert(c2w):
    """world -> camera rows [n,3,4] fp64 of camera -> world poses [n,4,4], as mesh_cull inverts them"""
    c2w = np.asarray(c2w, np.float64).reshape(-1, 4, 4)
    return np.stack([np.linalg.inv(m)[:3] for m in c2w])


def project_raw(vertices, w2c, intr):
    """(256 u, 256 v, p.z) in fp64 [n,V] each, in the kernel's order of operations (no fused multiply-add)"""
    p = np.asarray(vertices, np.float32).astype(np.float64).reshape(-1, 3)
    w = np.asarray(w2c, np.float64).reshape(-1, 3, 4)
    k = np.broadcast_to(np.asarray(intr, np.float64).reshape(-1, 4), (len(w), 4))
    X, Y, Z = p[None, :, 0], p[None, :, 1], p[None, :, 2]
    with np.errstate(all="ignore"):
        row = lambda r: ((w[:, r, 0, None] * X + w[:, r, 1, None] * Y) + w[:, r, 2, None] * Z) + w[:, r, 3, None]
        px, py, pz = row(0), row(1), row(2)
        u = k[:, 0, None] * px / pz + k[:, 2, None]
        v = k[:, 1, None] * py / pz + k[:, 3, None]
        return u * SUB, v * SUB, pz


def project(vertices, w2c, intr, near=0.01):
    """xy int64 [n,V,2] and z fp32 [n,V]; an invalid vertex gets zeros"""
    us, vs, pz = project_raw(vertices, w2c, intr)
    with np.errstate(all="ignore"):
        zf = pz.astype(np.float32)
        ok = (pz >= near) & (np.abs(us / SUB) <= GUARD) & (np.abs(vs / SUB) <= GUARD) & (zf > 0) & np.isfinite(zf)
        x = np.where(ok, np.rint(np.where(ok, us, 0.0)), 0.0).astype(np.int64)
        y = np.where(ok, np.rint(np.where(ok, vs, 0.0)), 0.0).astype(np.int64)
    return np.stack([x, y], -1), np.where(ok, zf, np.float32(0.0)).astype(np.float32)


def raster(xy, z, triangles, H, W):
    """one frame: the z-buffer fp64 [H,W] (inf where nothing is hit) of the triangles from snapped xy int [V,2] and z fp32 [V], and the
    number of triangles with an invalid vertex.  Coverage in exact integers, depth A / (E0/z0 + E1/z1 + E2/z2) in fp64."""
    xy = np.asarray(xy, np.int64)
    zz = np.asarray(z, np.float32).astype(np.float64)
    depth = np.full((H, W), np.inf)
    skipped = 0
    g = int(GUARD) * SUB
    for tri in np.asarray(triangles, np.int64).reshape(-1, 3):
        zs = zz[tri]
        if not (np.all(zs > 0) and np.all(np.isfinite(zs))) or np.abs(xy[tri]).max() > g:
            skipped += 1
            continue
        (x0, y0), (x1, y1), (x2, y2) = (tuple(int(c) for c in xy[i]) for i in tri)
        z0, z1, z2 = zs
        A = (x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0)
        if A == 0:
            continue
        if A < 0:
            x1, y1, z1, x2, y2, z2, A = x2, y2, z2, x1, y1, z1, -A
        j0, j1 = max(0, -(-min(x0, x1, x2) // SUB)), min(W - 1, max(x0, x1, x2) // SUB)
        i0, i1 = max(0, -(-min(y0, y1, y2) // SUB)), min(H - 1, max(y0, y1, y2) // SUB)
        if j0 > j1 or i0 > i1:
            continue
        py, px = np.meshgrid(np.arange(i0, i1 + 1, dtype=np.int64) * SUB, np.arange(j0, j1 + 1, dtype=np.int64) * SUB, indexing="ij")
        edge = lambda xp, yp, xq, yq: (xq - xp) * (py - yp) - (yq - yp) * (px - xp)
        e0, e1, e2 = edge(x1, y1, x2, y2), edge(x2, y2, x0, y0), edge(x0, y0, x1, y1)
        assert np.all(e0 + e1 + e2 == A)
        inside = (e0 >= 0) & (e1 >= 0) & (e2 >= 0)
        with np.errstate(all="ignore"):
            d = np.where(inside, A / (e0 / z0 + e1 / z1 + e2 / z2), np.inf)
        box = depth[i0:i1 + 1, j0:j1 + 1]
        np.minimum(box, d, out=box)
    return depth, skipped


def visibility(xy, z, depth, H, W, edge=0, far=np.inf, eps=0.03):
    """seen int64 [V]: the number of frames that see each vertex; xy [n,V,2], z fp32 [n,V], depth fp32 [n,H,W] or None"""
    xy = np.asarray(xy, np.int64)
    z = np.asarray(z, np.float32)
    j, i = (xy[..., 0] + SUB // 2) >> 8, (xy[..., 1] + SUB // 2) >> 8
    ok = (z > 0) & (z <= np.float32(far)) & (j >= edge) & (j < W - edge) & (i >= edge) & (i < H - edge)
    if depth is not None:
        depth = np.asarray(depth, np.float32)
        f = np.broadcast_to(np.arange(xy.shape[0])[:, None], j.shape)
        d = depth[f, np.clip(i, 0, H - 1), np.clip(j, 0, W - 1)]
        with np.errstate(all="ignore"):
            diff = (z - d).astype(np.float32)                   # one fp32 subtraction
            ok &= ~(d > 0) | (diff <= np.float32(eps))
    return ok.sum(0).astype(np.int64)


def select(V, triangles, seen, min_views=1, rule="all"):
    """(kept vertex indices, kept face indices, reindexed faces, vertex_map) in the original order"""
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    s = np.asarray(seen)[t] >= min_views
    keep = s.all(1) if rule == "all" else s.any(1)
    used = np.zeros(V, bool)
    used[t[keep].ravel()] = True
    vmap = np.where(used, np.cumsum(used) - 1, -1)
    return np.nonzero(used)[0], np.nonzero(keep)[0], vmap[t[keep]], vmap


def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """camera -> world 4x4 of a camera at eye looking at target (x right, y down, z forward)"""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    f = target - eye
    f /= np.linalg.norm(f)
    r = np.cross(f, np.asarray(up, np.float64))
    r /= np.linalg.norm(r)
    d = np.cross(f, r)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = r, d, f, eye
    return m


# ---- the inputs the GPU tests use (shared with the CPU condition check)
INTR = (61.3, 59.7, 31.6, 23.4)          # fx, fy, cx, cy of a 48 x 64 image
ROOM_EYES = [((0.13, -0.21, 1.27), (1.9, 0.4, 1.0)), ((-0.37, 0.11, 1.31), (-1.9, -0.6, 0.9)), ((0.21, 0.33, 0.93), (0.3, 1.4, 0.5)),
             ((-0.11, -0.43, 1.53), (-0.4, -1.4, 0.7)), ((0.47, 0.19, 1.11), (1.1, -0.9, 0.3)), ((-0.53, -0.17, 0.87), (-1.3, 0.8, 1.2))]


def room_cameras(n=6):
    """n camera -> world poses inside the room of mesh_eval_ref.room_mesh, at least 0.5 m from every surface, cycling over six
    stations with a small per-round offset"""
    out = []
    for k in range(n):
        eye, tgt = ROOM_EYES[k % 6]
        s = 0.017 * (k // 6)
        out.append(look_at((eye[0] + s, eye[1] - s, eye[2] + 0.5 * s), tgt))
    return np.stack(out)


def room_intrinsics(n, shared=False):
    if shared:
        return np.asarray([INTR], np.float64)
    return np.asarray([[INTR[0] + 0.37 * k, INTR[1] - 0.29 * k, INTR[2] + 0.11 * k, INTR[3] - 0.07 * k] for k in range(n)], np.float64)


def scaled_intrinsics(n, s, shared=False):
    """room_intrinsics for an image s times as large (pixel centres at integers)"""
    k = room_intrinsics(n, shared).copy()
    k[:, :2] *= s
    k[:, 2:] = (k[:, 2:] + 0.5) * s - 0.5
    return k


def special_vertices(c2w, intr, near=0.01):
    """hand-placed world points for camera 0: behind it, just under and over near, just inside and outside the guard, NaN and inf"""
    m = np.asarray(c2w, np.float64).reshape(-1, 4, 4)[0]
    fx, fy, cx, cy = np.asarray(intr, np.float64).reshape(-1, 4)[0]
    cam = lambda x, y, z: m[:3, :3] @ np.array([x, y, z]) + m[:3, 3]
    at_pixel = lambda u, v, z: cam((u - cx) * z / fx, (v - cy) * z / fy, z)
    pts = [cam(0.1, 0.2, -1.0), cam(0.0, 0.0, near * 0.97), cam(0.0, 0.0, near * 1.03), at_pixel(GUARD - 3.3, 10.2, 0.5),
           at_pixel(GUARD + 3.3, 10.2, 0.5), at_pixel(7.4, -(GUARD - 2.7), 0.5), at_pixel(7.4, -(GUARD + 2.7), 0.5)]
    pts = np.asarray(pts, np.float64)
    bad = np.array([[np.nan, 0.0, 1.0], [0.3, np.inf, 1.0], [0.1, 0.2, -np.inf], [np.inf, np.inf, np.inf]])
    return np.concatenate([pts, bad]).astype(np.float32)


AXES = [((1, 0, 0), (0, 1, 0)), ((-1, 0, 0), (0, 0, 1)), ((0, 1, 0), (0, 0, 1)), ((0, -1, 0), (1, 0, 0)), ((0, 0, 1), (1, 0, 0))]


def axis_cameras(n):
    """n camera -> world poses that look along +-x, +-y or +z from the plane through the origin across that axis, shifted sideways:
    p.z is then a vertex coordinate itself, exactly an fp32 number, half an ulp from every fp32 rounding boundary"""
    out = []
    for k in range(n):
        f, r = (np.asarray(a, np.float64) for a in AXES[k % len(AXES)])
        eye = (0.137 + 0.0213 * k) * r + (0.291 - 0.0171 * k) * np.cross(f, r)
        m = np.eye(4)
        m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = r, np.cross(f, r), f, eye
        out.append(m)
    return np.stack(out)


def project_inputs():
    """every (vertices, c2w, intrinsics) case of the GPU projection test, by name.  The room under axis-aligned cameras (1, 16 and
    17 of them, own and shared intrinsics) with the hand-placed vertices, and a few vertices under freely rotated cameras."""
    import mesh_eval_ref as er
    room = er.room_mesh(8)[0].astype(np.float32)
    cases = {}
    for n in (1, 16, 17):
        for shared in (False, True):
            c2w, intr = axis_cameras(n), room_intrinsics(n, shared)
            cases[f"n{n}_{'shared' if shared else 'own'}"] = (np.concatenate([room, special_vertices(c2w, intr)]), c2w, intr)
    cases["rotated"] = (room[7::41], room_cameras(3), room_intrinsics(3))       # (a subset that meets the CPU condition check)
    return cases


def assert_hidden_box_sides_are_gone(v, t, kept_faces, eyes, n):
    """mesh_eval_ref.room_mesh(n) culled to kept_faces: the sides of the two inner boxes that face away from every camera position
    in `eyes` must be gone.  Each side has its own vertices; those on its rim coincide with the neighbouring side's and are seen
    with them, so a face is judged when it has a vertex inside the rim.  Returns the number of sides checked."""
    kept = np.zeros(len(t), bool)
    kept[kept_faces] = True
    f0, per = 12 * n * n, 12 * (n // 2) ** 2                    # faces of the outer box, of each inner box
    checked = 0
    for b, (lo, hi) in enumerate((((0.6, -1.2, 0.0), (1.5, -0.4, 0.9)), ((-1.6, 0.3, 0.0), (-1.1, 1.2, 1.6)))):
        lo, hi = np.asarray(lo), np.asarray(hi)
        faces = np.arange(f0 + b * per, f0 + (b + 1) * per)
        p = v[t[faces]]                                         # [faces, 3 vertices, xyz]
        for axis in range(3):
            others = [a for a in range(3) if a != axis]
            for side, plane in ((-1.0, lo[axis]), (1.0, hi[axis])):
                if np.any(side * (eyes[:, axis] - plane) > 0):
                    continue                                    # some camera is in front of this side
                on = np.all(np.abs(p[:, :, axis] - plane) < 1e-9, axis=1)
                rim = np.any((np.abs(p[:, :, others] - lo[others]) < 1e-9) | (np.abs(p[:, :, others] - hi[others]) < 1e-9), axis=2)
                inner = on & ~np.all(rim, axis=1)
                assert inner.sum() > 0 and not kept[faces[inner]].any(), (b, axis, side, int(kept[faces[inner]].sum()))
                checked += 1
    return checked


# ---- hand-written snapped coordinates for the rasteriser
def raster_cases(H, W):
    """name -> (xy int64 [V,2] in 1/256 pixel, z fp32 [V], triangles int64 [F,3]) for an H x W image"""
    S = SUB
    cases = {}

    def case(name, pts_px, z, tris):
        xy = np.rint(np.asarray(pts_px, np.float64) * S).astype(np.int64).reshape(-1, 2)
        cases[name] = (xy, np.asarray(z, np.float32), np.asarray(tris, np.int64).reshape(-1, 3))

    case("whole_image", [(-10, -10), (3 * W, -10), (-10, 3 * H)], [1.0, 2.0, 3.0], [(0, 1, 2)])
    case("slivers", [(2.3, 5.1), (W - 3.2, 5.4), (2.3, 5.35), (2.3, 8.9), (W - 3.2, 9.2), (2.3, 9.15)], [1.5, 2.5, 1.5, 2.0, 1.0, 2.0],
         [(0, 1, 2), (3, 4, 5)])
    # bounding boxes of exactly 8 x 8 (the thread's loop), 8 x 9 and 9 x 8 pixels (a wave's), and the same boxes not pixel aligned
    case("box_8x8_8x9_9x8", [(10, 10), (17, 10), (10, 17), (20, 10), (27, 10), (20, 18), (30, 10), (38, 10), (30, 17),
                             (9.5, 20.5), (17.5, 20.5), (9.5, 28.5), (19.5, 20.5), (27.5, 20.5), (19.5, 29.5), (29.5, 20.5), (38.5, 20.5),
                             (29.5, 28.5)],
         [1.0, 1.5, 2.0] * 6, [(0, 1, 2), (3, 4, 5), (6, 7, 8), (9, 10, 11), (12, 13, 14), (15, 16, 17)])
    off = [(-6.5, 5.2), (4.5, 9.1), (-3.2, 14.7),                        # partly off each side
           (W - 4.5, 6.3), (W + 7.2, 11.4), (W - 2.1, 15.8),
           (8.3, -5.5), (19.7, 4.2), (12.1, -2.2),
           (9.4, H - 3.6), (21.3, H + 6.5), (14.2, H - 1.5),
           (-30.5, 5.0), (-20.5, 9.0), (-25.0, 16.0),                    # wholly off each side
           (W + 5.5, 5.0), (W + 20.5, 9.0), (W + 12.0, 16.0),
           (8.0, -25.5), (19.0, -12.5), (12.0, -4.5),
           (8.0, H + 2.5), (19.0, H + 12.5), (12.0, H + 20.5),
           (-8.0, -8.0), (W + 8.0, -4.0), (W / 2, 3.5)]                  # over the two upper corners
    case("off_screen", off, [1.0 + 0.1 * k for k in range(len(off))], [(3 * k, 3 * k + 1, 3 * k + 2) for k in range(len(off) // 3)])
    # a vertex on a pixel centre and an edge (the hypotenuse, and the two legs) through pixel centres; the image corner pixel itself
    case("through_centres", [(5, 5), (15, 5), (5, 15), (0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W - 1, H - 4), (W - 4, H - 1)],
         [1.0, 2.0, 4.0, 2.0, 2.5, 3.0, 1.0, 1.0, 1.0], [(0, 1, 2), (3, 4, 5), (6, 7, 8)])
    case("zero_area", [(3, 3), (9, 9), (20, 20), (7, 4), (7, 4), (12, 9), (5, 20), (25, 20), (15, 20)], [1.0] * 9,
         [(0, 1, 2), (3, 4, 5), (6, 7, 8), (0, 0, 0)])
    case("both_windings", [(4.2, 3.1), (18.6, 5.3), (9.7, 17.9), (24.2, 3.1), (38.6, 5.3), (29.7, 17.9)], [1.0, 1.2, 1.4, 1.0, 1.2, 1.4],
         [(0, 1, 2), (3, 5, 4)])
    case("invalid_vertex", [(4.2, 3.1), (18.6, 5.3), (9.7, 17.9), (0, 0), (30.0, 20.0), (12.0, 25.0)], [1.0, 1.2, 1.4, 0.0, 2.0, 0.0],
         [(0, 1, 2), (0, 1, 3), (3, 4, 5), (4, 1, 2), (5, 3, 0)])
    case("crossing", [(3.3, 4.1), (40.7, 6.2), (20.1, 30.4), (5.2, 3.6), (39.1, 8.8), (18.4, 31.9)], [1.0, 1.0, 3.0, 3.0, 3.0, 1.0],
         [(0, 1, 2), (3, 4, 5)])
    # a tessellated plane whose vertices sit on pixel centres: cells of 2 x 3 pixels, tilted depth
    gx, gy = (W - 5) // 2, (H - 5) // 3
    pts, zz, tris = [], [], []
    for a in range(gy + 1):
        for b in range(gx + 1):
            pts.append((2 + 2 * b, 2 + 3 * a))
            zz.append(1.0 + 0.05 * a + 0.02 * b)
    for a in range(gy):
        for b in range(gx):
            p = a * (gx + 1) + b
            tris += [(p, p + 1, p + gx + 2), (p, p + gx + 2, p + gx + 1)]
    case("tessellated_plane", pts, zz, tris)
    return cases


def plane_interior(H, W):
    """the pixel box that raster_cases' tessellated plane covers: rows, columns (inclusive)"""
    gx, gy = (W - 5) // 2, (H - 5) // 3
    return (2, 2 + 3 * gy), (2, 2 + 2 * gx)
