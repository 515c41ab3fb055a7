"""fp64 numpy restatement of the TSDF fusion, marching cubes and cleaning of csrc/sgr_mesh.hip (conventions 1-5 of DESIGN.md
section 3), for the tests only.  Voxel v of a unit is x + 16 y + 256 z; arrays shaped [n, 16(z), 16(y), 16(x)] flatten in that
order."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = 16


def load_generator():
    spec = importlib.util.spec_from_file_location("gen_mc_table", os.path.join(ROOT, "scripts", "gen_mc_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_GEN = load_generator()
TABLE = _GEN.table()
CORNERS, EDGES = _GEN.CORNERS, _GEN.EDGES


# ---- frames
def frame_arrays(fr, depth_trunc=30.0):
    """(depth fp64 [H,W] as the volume sees it, colour bytes int [3,H,W], colour knife edge [3,H,W] bool) of a frame dict with
    numpy / torch fp32 inputs"""
    g = lambda t: None if t is None else np.asarray(t.detach().cpu().numpy() if hasattr(t, "detach") else t)
    render = g(fr["render"]).astype(np.float32)
    H, W = render.shape[1:]
    depth = g(fr["depth"]).astype(np.float32).reshape(H, W)
    d = (np.float32(fr.get("global_scale", 1.0)) * depth).astype(np.float64)
    gt = g(fr.get("gt_depth"))
    if gt is not None:
        d[gt.reshape(H, W) == 0] = 0.0
    d[d > depth_trunc] = 0.0
    a, b = g(fr.get("exposure_a")), g(fr.get("exposure_b"))
    ea = np.float32(np.exp(np.float64(a.reshape(-1)[0]))) if a is not None else np.float32(1.0)
    eb = np.float32(b.reshape(-1)[0]) if b is not None else np.float32(0.0)
    img = np.clip((ea * render).astype(np.float32) + eb, np.float32(0), np.float32(1)).astype(np.float32)
    prod = (img * np.float32(255.0)).astype(np.float32)
    frac = prod - np.floor(prod)
    knife = (np.minimum(frac, 1 - frac) < 3e-5 * np.maximum(prod, 1.0)) & (prod > 0) & (prod < 255)
    return d, prod.astype(np.int64).astype(np.float64), knife


def w2c_of(fr):
    m = fr["w2c"]
    return np.asarray(m.detach().cpu().numpy() if hasattr(m, "detach") else m, dtype=np.float64).reshape(4, 4)


def touched_units(fr, voxel_length, sdf_trunc, depth_trunc=30.0):
    """(set of unit keys, smallest distance of a sampled point +- sdf_trunc to a unit boundary)"""
    d, _, _ = frame_arrays(fr, depth_trunc)
    H, W = d.shape
    L = R * voxel_length
    v, u = np.mgrid[0:H:4, 0:W:4]
    dd = d[v, u]
    ok = dd > 0
    u, v, dd = u[ok].astype(np.float64), v[ok].astype(np.float64), dd[ok]
    pc = np.stack([(u - fr["cx"]) * dd / fr["fx"], (v - fr["cy"]) * dd / fr["fy"], dd, np.ones_like(dd)], 0)
    p = (np.linalg.inv(w2c_of(fr)) @ pc)[:3].T
    keys, margin = set(), np.inf
    for s in (-sdf_trunc, sdf_trunc):
        q = (p + s) / L
        margin = min(margin, float(np.min(np.abs(q - np.round(q)))) * L if len(q) else np.inf)
    lo = np.floor((p - sdf_trunc) / L).astype(np.int64)
    hi = np.floor((p + sdf_trunc) / L).astype(np.int64)
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                k = np.stack([np.where(dx, hi[:, 0], lo[:, 0]), np.where(dy, hi[:, 1], lo[:, 1]), np.where(dz, hi[:, 2], lo[:, 2])], 1)
                keys.update(map(tuple, k.tolist()))
    return keys, margin


class RefVolume:
    """dict unit key -> arrays tsdf, weight [16,16,16], color [3,16,16,16]; `ambiguous` marks voxels an fp32 evaluation may
    decide differently (pixel, truncation or colour-byte knife edges)"""

    def __init__(self, voxel_length, sdf_trunc, depth_trunc=30.0):
        self.vl, self.trunc, self.depth_trunc = voxel_length, sdf_trunc, depth_trunc
        self.units = {}

    def _unit(self, k):
        if k not in self.units:
            self.units[k] = dict(tsdf=np.zeros((R, R, R)), weight=np.zeros((R, R, R)), color=np.zeros((3, R, R, R)),
                                 ambiguous=np.zeros((R, R, R), bool))
        return self.units[k]

    def integrate(self, fr):
        keys, _ = touched_units(fr, self.vl, self.trunc, self.depth_trunc)
        d, col, knife = frame_arrays(fr, self.depth_trunc)
        H, W = d.shape
        w2c = w2c_of(fr)
        fx, fy, cx, cy = (float(fr[k]) for k in ("fx", "fy", "cx", "cy"))
        z_, y_, x_ = np.mgrid[0:R, 0:R, 0:R]
        for k in sorted(keys):
            U = self._unit(k)
            pw = np.stack([((k[0] * R + x_) + 0.5) * self.vl, ((k[1] * R + y_) + 0.5) * self.vl, ((k[2] * R + z_) + 0.5) * self.vl], 0)
            pc = np.einsum("ij,jzyx->izyx", w2c[:3, :3], pw) + w2c[:3, 3][:, None, None, None]
            x, y, z = pc
            with np.errstate(divide="ignore", invalid="ignore"):
                uf = x * fx / z + cx + 0.5
                vf = y * fy / z + cy + 0.5
            ok = (z > 0) & (uf >= 1e-4) & (uf < W) & (vf >= 1e-4) & (vf < H)
            amb = np.zeros_like(ok)
            edge = lambda a: np.abs(a - np.round(a)) < 1e-3
            amb |= (z > 0) & (edge(uf) | edge(vf) | (np.abs(uf - 1e-4) < 1e-3) | (np.abs(vf - 1e-4) < 1e-3))
            ui = np.where(ok, uf, 0).astype(np.int64)
            vi = np.where(ok, vf, 0).astype(np.int64)
            dd = np.where(ok, d[vi, ui], 0.0)
            ok &= dd > 0
            mult = np.sqrt(((ui - cx) / fx) ** 2 + ((vi - cy) / fy) ** 2 + 1)
            sdf = (dd - z) * mult
            amb |= ok & (np.abs(sdf + self.trunc) < 1e-5)
            ok &= sdf > -self.trunc
            amb |= ok & knife[:, vi, ui].any(0)
            tsdf = np.minimum(1.0, sdf / self.trunc)
            w = U["weight"]
            U["tsdf"] = np.where(ok, (U["tsdf"] * w + tsdf) / (w + 1), U["tsdf"])
            for c in range(3):
                U["color"][c] = np.where(ok, (U["color"][c] * w + col[c][vi, ui]) / (w + 1), U["color"][c])
            U["weight"] = np.where(ok, w + 1, w)
            U["ambiguous"] |= amb

    def arrays(self):
        """ascending keys: keys [n,3], tsdf / weight [n,4096], color [n,4096,3], ambiguous [n,4096]"""
        ks = sorted(self.units)
        f = lambda name: np.stack([self.units[k][name].reshape(-1) for k in ks]) if ks else np.zeros((0, R ** 3))
        col = np.stack([self.units[k]["color"].reshape(3, -1).T for k in ks]) if ks else np.zeros((0, R ** 3, 3))
        return dict(keys=np.array(ks, dtype=np.int64).reshape(-1, 3), tsdf=f("tsdf"), weight=f("weight"), color=col,
                    ambiguous=f("ambiguous").astype(bool))


# ---- marching cubes
def _padded(arr, keys, fill):
    """arr [n,16,16,16,...] -> [n,18,18,18,...] with each unit's 3x3x3 neighbours' border voxels (fill where none)"""
    n = len(keys)
    index = {tuple(k): i for i, k in enumerate(keys.tolist())}
    out = np.full((n, R + 2, R + 2, R + 2) + arr.shape[4:], fill, dtype=arr.dtype)
    sl = {-1: (slice(0, 1), slice(R - 1, R)), 0: (slice(1, R + 1), slice(0, R)), 1: (slice(R + 1, R + 2), slice(0, 1))}
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                nb = np.array([index.get((k[0] + dx, k[1] + dy, k[2] + dz), -1) for k in keys.tolist()], dtype=np.int64)
                has = nb >= 0
                if not has.any():
                    continue
                out[has, sl[dz][0], sl[dy][0], sl[dx][0]] = arr[nb[has]][:, sl[dz][1], sl[dy][1], sl[dx][1]]
    return out


def extract(vox, voxel_length):
    """marching cubes of a volume read back through TSDFVolume.voxels() (or RefVolume.arrays()): (vertices fp64 [V,3],
    triangles int64 [F,3], colours fp64 [V,3] on 0..1), in the kernels' order"""
    keys = np.asarray(vox["keys"], dtype=np.int64).reshape(-1, 3)
    n = len(keys)
    if n == 0:
        return np.zeros((0, 3)), np.zeros((0, 3), np.int64), np.zeros((0, 3))
    T = np.asarray(vox["tsdf"], dtype=np.float64).reshape(n, R, R, R)
    Wt = np.asarray(vox["weight"], dtype=np.float64).reshape(n, R, R, R)
    Cc = np.asarray(vox["color"], dtype=np.float64).reshape(n, R, R, R, 3)
    PT, PW, PC = _padded(T, keys, 0.0), _padded(Wt, keys, 0.0), _padded(Cc, keys, 0.0)
    # cubes with base at padded index 0..16 (voxel -1..15)
    valid = np.ones((n, R + 1, R + 1, R + 1), bool)
    case = np.zeros((n, R + 1, R + 1, R + 1), np.int64)
    for c, (ox, oy, oz) in enumerate(CORNERS):
        w = PW[:, oz:oz + R + 1, oy:oy + R + 1, ox:ox + R + 1]
        t = PT[:, oz:oz + R + 1, oy:oy + R + 1, ox:ox + R + 1]
        valid &= w > 0
        case |= (t < 0).astype(np.int64) << c
    cube = lambda dz, dy, dx: valid[:, 1 + dz:R + 1 + dz, 1 + dy:R + 1 + dy, 1 + dx:R + 1 + dx]
    t0, w0 = PT[:, 1:R + 1, 1:R + 1, 1:R + 1], PW[:, 1:R + 1, 1:R + 1, 1:R + 1]
    masks = np.zeros((n, R, R, R, 3), bool)
    for d in range(3):
        s = [1, 1, 1]
        s[2 - d] += 1                                # padded arrays are [z, y, x]
        t1 = PT[:, s[0]:s[0] + R, s[1]:s[1] + R, s[2]:s[2] + R]
        w1 = PW[:, s[0]:s[0] + R, s[1]:s[1] + R, s[2]:s[2] + R]
        a, b = [ax for ax in range(3) if ax != d]
        anyc = np.zeros((n, R, R, R), bool)
        for c in range(4):
            o = [0, 0, 0]
            o[a], o[b] = -(c & 1), -(c >> 1)
            anyc |= cube(o[2], o[1], o[0])
        masks[..., d] = (w0 > 0) & (w1 > 0) & ((t0 < 0) != (t1 < 0)) & anyc
    ids = np.full(masks.shape, -1, np.int64)
    ids[masks] = np.arange(int(masks.sum()))
    z_, y_, x_ = np.mgrid[0:R, 0:R, 0:R]
    un, zz, yy, xx, dd = np.nonzero(masks)
    p0 = np.stack([(keys[un, 0] * R + xx + 0.5) * voxel_length, (keys[un, 1] * R + yy + 0.5) * voxel_length,
                   (keys[un, 2] * R + zz + 0.5) * voxel_length], 1)
    f0 = T[un, zz, yy, xx]
    n1 = np.stack([xx + (dd == 0), yy + (dd == 1), zz + (dd == 2)], 1)
    f1 = PT[un, n1[:, 2] + 1, n1[:, 1] + 1, n1[:, 0] + 1]
    c0 = Cc[un, zz, yy, xx]
    c1 = PC[un, n1[:, 2] + 1, n1[:, 1] + 1, n1[:, 0] + 1]
    t = np.abs(f0) / (np.abs(f0) + np.abs(f1))
    verts = p0.copy()
    verts[np.arange(len(dd)), dd] += t * voxel_length
    cols = (c0 + t[:, None] * (c1 - c0)) / 255.0
    # triangles
    Pid = _padded(ids, keys, -1)
    vcase = case[:, 1:, 1:, 1:]
    vvalid = valid[:, 1:, 1:, 1:] & (vcase != 0) & (vcase != 255)
    cu, cz, cy, cx = np.nonzero(vvalid)
    cases = vcase[cu, cz, cy, cx]
    tris = []
    owner = []
    for e, (a, b) in enumerate(EDGES):
        d = [k for k in range(3) if CORNERS[a][k] != CORNERS[b][k]][0]
        lo = a if CORNERS[a][d] < CORNERS[b][d] else b
        owner.append((CORNERS[lo], d))
    per_cube = []
    for ci, u, z, y, x in zip(cases.tolist(), cu.tolist(), cz.tolist(), cy.tolist(), cx.tolist()):
        for tri in TABLE[ci]:
            row = []
            for e in tri:
                (ox, oy, oz), d = owner[e]
                row.append(Pid[u, z + oz + 1, y + oy + 1, x + ox + 1, d])
            per_cube.append(row)
    tris = np.array(per_cube, dtype=np.int64).reshape(-1, 3)
    assert (tris >= 0).all()
    return verts, tris, cols


# ---- cleaning
def components(V, tris):
    """label = smallest vertex id of the component over triangle edges"""
    lab = np.arange(V)
    if len(tris) == 0:
        return lab
    e = np.concatenate([tris[:, [0, 1]], tris[:, [1, 2]], tris[:, [2, 0]]])
    while True:
        m = np.minimum(lab[e[:, 0]], lab[e[:, 1]])
        new = lab.copy()
        np.minimum.at(new, e[:, 0], m)
        np.minimum.at(new, e[:, 1], m)
        new = new[new]
        if (new == lab).all():
            return lab
        lab = new


def clean(verts, tris, cols, min_len=100):
    """(vertices, triangles, colours, vertex map) as sgr_mesh_components / sgr_mesh_compact"""
    V = len(verts)
    lab = components(V, tris)
    size = np.bincount(lab, minlength=V)
    keepv = size[lab] >= min_len
    vmap = np.full(V, -1, np.int64)
    vmap[keepv] = np.arange(int(keepv.sum()))
    keep = np.zeros(len(tris), bool)
    seen = set()
    for i, (a, b, c) in enumerate(tris.tolist()):
        if not keepv[a] or a == b or b == c or a == c:
            continue
        n = np.cross(verts[b] - verts[a], verts[c] - verts[a])
        if not n.any():
            continue
        k = tuple(sorted((a, b, c)))
        if k in seen:
            continue
        seen.add(k)
        keep[i] = True
    return verts[keepv], vmap[tris[keep]], cols[keepv], vmap


# ---- mesh properties
def edge_use(tris):
    """directed edge -> count, and undirected edge -> count"""
    e = np.concatenate([tris[:, [0, 1]], tris[:, [1, 2]], tris[:, [2, 0]]])
    und = np.sort(e, 1)
    ue, uc = np.unique(und, axis=0, return_counts=True)
    de, dc = np.unique(e, axis=0, return_counts=True)
    return (de, dc), (ue, uc)


def closed_and_oriented(tris):
    (de, dc), (ue, uc) = edge_use(tris)
    return bool((uc == 2).all() and (dc == 1).all())


def euler(V, tris):
    (_, _), (ue, _) = edge_use(tris)
    return V - len(ue) + len(tris)


def sphere_views(n_views, radius, W, H, f, dist, centre=(0.0, 0.0, 0.0), seed=0):
    """analytic depth / colour of a sphere seen from n_views cameras looking at its centre: list of frame dicts (numpy)"""
    rng = np.random.default_rng(seed)
    dirs = [np.array(d, float) for d in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))]
    dirs += [np.array((sx, sy, sz), float) / np.sqrt(3) for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]
    while len(dirs) < n_views:
        v = rng.normal(size=3)
        dirs.append(v / np.linalg.norm(v))
    centre = np.asarray(centre, float)
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    frames = []
    for k in range(n_views):
        fwd = -dirs[k] + 1e-3 * rng.normal(size=3)
        fwd /= np.linalg.norm(fwd)
        up = np.array([0.0, 1.0, 0.0]) if abs(fwd[1]) < 0.9 else np.array([1.0, 0.0, 0.0])
        right = np.cross(up, fwd)
        right /= np.linalg.norm(right)
        down = np.cross(fwd, right)
        Rm = np.stack([right, down, fwd])
        eye = centre - fwd * dist
        w2c = np.eye(4)
        w2c[:3, :3] = Rm
        w2c[:3, 3] = -Rm @ eye
        v, u = np.mgrid[0:H, 0:W].astype(np.float64)
        ray = np.stack([(u - cx) / f, (v - cy) / f, np.ones_like(u)], -1)
        rw = ray @ Rm                                   # world directions (unnormalised, z_cam = 1)
        oc = eye - centre
        a = (rw * rw).sum(-1)
        b = 2 * (rw @ oc)
        c = oc @ oc - radius ** 2
        disc = b * b - 4 * a * c
        t = np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a), 0.0)
        depth = np.where(disc > 0, t, 0.0).astype(np.float32)   # t is the camera z (ray z = 1)
        pts = eye + t[..., None] * rw
        colr = np.stack([0.5 + 0.4 * np.sin(3 * pts[..., 0]), 0.5 + 0.4 * np.cos(2 * pts[..., 1]), 0.5 + 0.3 * pts[..., 2]], 0)
        frames.append(dict(render=np.clip(colr, 0, 1).astype(np.float32), depth=depth, w2c=w2c, fx=f, fy=f, cx=cx, cy=cy))
    return frames
