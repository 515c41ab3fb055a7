"""The volumes, meshes and frames that hold the kernels of csrc/sgr_mesh.hip to tests/mesh_ref.py away from the smooth interior, and
the conditions that make each of them meaningful.  Shared by tests/test_mesh_cpu.py, which proves the conditions on the restatement
alone, and tests/test_gpu_mesh_edges.py, which can therefore exclude nothing.  Seeded numpy (torch for the one large mesh), no GPU.

A volume is the dict of TSDFVolume.voxels(): keys int64 [n,3] ascending, tsdf / weight fp32 [n,4096], color fp32 [n,4096,3] on
0..255, voxel v = x + 16 y + 256 z."""
import fractions

import numpy as np
import torch

import mesh_ref as ref

R = ref.R
U = 2.0 ** -24                                   # unit roundoff of fp32


# ---- volumes
def _units_of_block(keys, T, Wt, C, origin):
    """cuts the units `keys` out of block arrays [Z,Y,X(,3)] whose voxel (0,0,0) is voxel 0 of unit `origin`"""
    keys = np.array(sorted(map(tuple, keys)), dtype=np.int64).reshape(-1, 3)
    sl = lambda k, a: slice((k[a] - origin[a]) * R, (k[a] - origin[a] + 1) * R)
    cut = lambda A: np.stack([A[sl(k, 2), sl(k, 1), sl(k, 0)].reshape((R ** 3,) + A.shape[3:]) for k in keys])
    return dict(keys=keys, tsdf=cut(T).astype(np.float32), weight=cut(Wt).astype(np.float32), color=cut(C).astype(np.float32))


def _noise(rng, shape):
    """uniform in +-1 with |T| >= 2^-10"""
    return (rng.uniform(2.0 ** -10, 1.0, shape) * rng.choice([-1.0, 1.0], shape)).astype(np.float32)


# the voxels (x, y, z) of noise_block's 32^3 block that hold an exact zero, a negative zero or a subnormal: inside a unit, on unit
# faces (a coordinate of 15 or 16), and next to the corner where the eight units meet
MARKS = (((5, 6, 7), 0.0), ((15, 9, 20), 0.0), ((16, 16, 16), 0.0), ((22, 15, 3), -0.0), ((15, 15, 15), -0.0),
         ((9, 16, 25), 1e-40), ((16, 4, 15), 1e-40), ((25, 25, 9), -1e-40), ((15, 20, 16), -1e-40))


def noise_block(seed=0):
    """2x2x2 units with keys in {-1, 0}^3: noise of weight 1 and random colours inside a closed shell of T = +1 (the outermost voxel
    layer).  The voxels of MARKS hold exactly 0.0, -0.0 or a subnormal; the +x, +y, +z neighbours of each are on the other side
    (T < 0 next to 0.0, -0.0 and the positive subnormal, which count as outside; T > 0 next to the negative one), so its three edges
    toward them are active and their vertices sit on the voxel itself.  Returns (volume, block) with block = dict(T, W) [32,32,32]
    indexed [z, y, x], voxel (0,0,0) of the block being voxel 0 of unit (-1,-1,-1)."""
    rng = np.random.default_rng(seed)
    n = 2 * R
    T = _noise(rng, (n, n, n))
    T[[0, -1], :, :] = T[:, [0, -1], :] = T[:, :, [0, -1]] = 1.0
    for (x, y, z), val in MARKS:
        val = np.float32(val)
        T[z, y, x] = val
        side = 1.0 if (val < 0) else -1.0
        for dx, dy, dz in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):
            T[z + dz, y + dy, x + dx] = side * abs(T[z + dz, y + dy, x + dx])
    Wt = np.ones((n, n, n), np.float32)
    C = np.floor(rng.uniform(0, 256, (n, n, n, 3))).astype(np.float32)
    keys = [(x, y, z) for x in (-1, 0) for y in (-1, 0) for z in (-1, 0)]
    return _units_of_block(keys, T, Wt, C, (-1, -1, -1)), dict(T=T, W=Wt)


FAR = (-300, 299, 5)
_CUBE7 = [(x, y, z) for x in (-1, 0) for y in (-1, 0) for z in (-1, 0) if (x, y, z) != (0, -1, 0)]
HOLE_KEYS = {1: [FAR],
             3: [FAR, (0, 0, 0), (1, 1, 0)],                              # (1,1,0) touches (0,0,0) along an edge only
             5: [FAR, (0, 0, 0), (1, 1, 0), (-1, -1, -1), (0, 1, 1)],     # and two more that meet the others only diagonally
             7: _CUBE7,                                                   # the block of noise_block without one unit
             9: _CUBE7 + [FAR, (1, 1, 1)]}                                # (1,1,1) touches the block at one corner


def holes(n_units, seed=1):
    """the units HOLE_KEYS[n_units] of the same noise with no shell and about 5 % of the voxels at weight 0.  n_units is 1, 3, 5, 7
    or 9: a single unit, and counts that the bitonic sort has to pad with empty keys"""
    rng = np.random.default_rng(seed + n_units)
    keys = np.array(sorted(HOLE_KEYS[n_units]), dtype=np.int64)
    n = len(keys)
    T = _noise(rng, (n, R ** 3))
    Wt = (rng.uniform(size=(n, R ** 3)) >= 0.05).astype(np.float32)
    C = np.floor(rng.uniform(0, 256, (n, R ** 3, 3))).astype(np.float32)
    return dict(keys=keys, tsdf=T, weight=Wt, color=C)


def cube_tables(vox):
    """what decides every cube with its base in a unit of vox (base voxel 0..15 per axis), by the rule of DESIGN.md (4) restated on
    padded arrays: valid [n,16,16,16] (z, y, x), case, span (how many units hold its corners, 0 where one of them is missing), and
    why an invalid cube is skipped: hole (a corner of weight 0 in a unit that exists), face / diagonal (a corner in a missing unit
    that shares a face / only an edge or a corner with the base's unit)"""
    keys = np.asarray(vox["keys"], dtype=np.int64)
    n = len(keys)
    T = np.asarray(vox["tsdf"], dtype=np.float64).reshape(n, R, R, R)
    Wt = np.asarray(vox["weight"], dtype=np.float64).reshape(n, R, R, R)
    PT, PW, PU = ref._padded(T, keys, 0.0), ref._padded(Wt, keys, 0.0), ref._padded(np.ones_like(Wt), keys, 0.0) > 0
    z_, y_, x_ = np.mgrid[0:R, 0:R, 0:R]
    shape = (n, R, R, R)
    valid, hole, face, diag = np.ones(shape, bool), np.zeros(shape, bool), np.zeros(shape, bool), np.zeros(shape, bool)
    case = np.zeros(shape, np.int64)
    units = np.zeros(shape + (8,), np.int64)
    for c, (ox, oy, oz) in enumerate(ref.CORNERS):
        s = (slice(None), slice(1 + oz, 1 + oz + R), slice(1 + oy, 1 + oy + R), slice(1 + ox, 1 + ox + R))
        crossed = ((x_ + ox) // R) + ((y_ + oy) // R) + ((z_ + oz) // R)          # how many unit borders the corner is across
        valid &= PW[s] > 0
        hole |= PU[s] & ~(PW[s] > 0)
        face |= ~PU[s] & (crossed == 1)[None]
        diag |= ~PU[s] & (crossed >= 2)[None]
        case |= (PT[s] < 0).astype(np.int64) << c
        units[..., c] = ((x_ + ox) // R) + 2 * ((y_ + oy) // R) + 4 * ((z_ + oz) // R)
    span = np.array([len(set(row)) for row in units.reshape(-1, 8)[:R ** 3]]).reshape(R, R, R)[None] * (~face & ~diag)
    return dict(valid=valid, case=case, span=span, hole=hole, face=face, diagonal=diag, PT=PT, PW=PW)


def dead_active_edges(vox):
    """how many voxel edges change sign between two voxels of weight > 0 while none of their four cubes is valid: no vertex may
    appear there"""
    t = cube_tables(vox)
    keys = np.asarray(vox["keys"], dtype=np.int64)
    n = len(keys)
    # validity of the cubes with base voxel -1..15: the cubes of the neighbour units at index 15, nothing where there is none
    pv = ref._padded(t["valid"], keys, False)[:, 0:R + 1, 0:R + 1, 0:R + 1]
    PT, PW = t["PT"], t["PW"]
    t0, w0 = PT[:, 1:R + 1, 1:R + 1, 1:R + 1], PW[:, 1:R + 1, 1:R + 1, 1:R + 1]
    dead = 0
    for d in range(3):
        s = [1, 1, 1]
        s[2 - d] += 1
        t1 = PT[:, s[0]:s[0] + R, s[1]:s[1] + R, s[2]:s[2] + R]
        w1 = PW[:, s[0]:s[0] + R, s[1]:s[1] + R, s[2]:s[2] + R]
        a, b = [ax for ax in range(3) if ax != d]
        anyc = np.zeros((n, R, R, R), bool)
        for c in range(4):
            o = [0, 0, 0]
            o[a], o[b] = -(c & 1), -(c >> 1)
            anyc |= pv[:, 1 + o[2]:1 + o[2] + R, 1 + o[1]:1 + o[1] + R, 1 + o[0]:1 + o[0] + R]
        dead += int(((w0 > 0) & (w1 > 0) & ((t0 < 0) != (t1 < 0)) & ~anyc).sum())
    return dead


STRIP_UNITS, STRIP_FIRST = 4100, -2050


def strip_of_units(n=STRIP_UNITS, first=STRIP_FIRST):
    """n units (i, 0, 0), i from `first`, with T = (iz - 7.3) / 8 and weight 1: one flat sheet between the voxel layers iz = 7 and 8,
    longer than one 4096-unit scan block.  Returns (volume, t) with t the fp64 place of the sheet on its edge, from the fp32 T"""
    keys = np.stack([np.arange(first, first + n), np.zeros(n, np.int64), np.zeros(n, np.int64)], 1).astype(np.int64)
    Tz = ((np.arange(R, dtype=np.float64) - 7.3) / 8).astype(np.float32)
    unit = np.repeat(Tz, R * R)                                      # voxel v = x + 16 y + 256 z
    f0, f1 = abs(float(Tz[7])), abs(float(Tz[8]))
    return dict(keys=keys, tsdf=np.tile(unit, (n, 1)), weight=np.ones((n, R ** 3), np.float32),
                color=np.zeros((n, R ** 3, 3), np.float32)), f0 / (f0 + f1)


def vertex_bound(p, voxel_length):
    """|device vertex - fp64 vertex| per component, from the operations of mc_emit_kernel with u = 2^-24 (see
    test_gpu_mesh_edges.test_extraction_of_noise_and_holes_equals_the_restatement): 2 u |p| + 4 u voxel_length, second-order terms
    covered by the factor"""
    return (2 * U * np.abs(p) + 4 * U * voxel_length) * (1 + 2.0 ** -20)


# ---- one frame whose colour bytes can be predicted
def color_frame(seed=5, W=64, H=48):
    """a plane at z = 0.9 facing a camera at the origin (identity pose), exposure a = 0.3, b = -0.07 and a random render.  A byte
    changes with the rounding of exp(a) r + b only where that lands within an ulp of some k / 255, which a random value does once
    in 10^5: so each value of the render is moved by up to 8 ulps to where, for one of the three candidates of exp(a) in turn, the
    separately rounded byte and the fused one differ, wherever these 17 neighbours hold such a value (about one in seven)."""
    rng = np.random.default_rng(seed)
    fr = dict(render=None, depth=np.full((H, W), 0.9, np.float32), w2c=np.eye(4), fx=80.0, fy=80.0, cx=(W - 1) / 2.0,
              cy=(H - 1) / 2.0, exposure_a=np.array([0.3], np.float32), exposure_b=np.array([-0.07], np.float32))
    eb = np.float64(fr["exposure_b"][0])
    cands = exposure_candidates(fr)
    k = rng.integers(1, 255, (3, H, W))
    which = rng.integers(0, 3, (3, H, W))
    ea = np.array([np.float64(e) for e in cands])[which]
    r0 = ((k / 255.0 - eb) / ea).astype(np.float32)                      # exp(a) r0 + b is about k / 255
    render = rng.uniform(0, 1, (3, H, W)).astype(np.float32)
    found = np.zeros((3, H, W), bool)
    for j in range(-8, 9):
        r = (r0.view(np.int32) + j).view(np.float32)
        fr["render"] = r
        hit = np.zeros((3, H, W), bool)
        for c, e in enumerate(cands):
            hit |= (which == c) & (color_bytes(fr, e) != color_bytes(fr, e, fused=True))
        render = np.where(hit & ~found, r, render)
        found |= hit
    fr["render"] = render
    return fr


def exposure_candidates(fr):
    """the fp32 neighbours of exp(a): numpy's and one ulp to either side (the device's expf may round the other way)"""
    e = np.float32(np.exp(np.float64(fr["exposure_a"][0])))
    return [np.nextafter(e, np.float32(0)), e, np.nextafter(e, np.float32(4))]


def color_bytes(fr, ea, fused=False):
    """int [3,H,W]: (int)(clamp(ea r + b, 0, 1) 255) with every step rounded to fp32 on its own, or, fused, with ea r + b rounded
    once (the exact product of two fp32 is an fp64)"""
    r, eb = fr["render"], np.float32(fr["exposure_b"][0])
    if fused:
        lin = (np.float64(ea) * r.astype(np.float64) + np.float64(eb)).astype(np.float32)
    else:
        lin = (np.float32(ea) * r).astype(np.float32) + eb
    img = np.clip(lin.astype(np.float32), np.float32(0), np.float32(1))
    return (img * np.float32(255.0)).astype(np.float32).astype(np.int64)


def voxel_pixels(fr, keys, voxel_length, sdf_trunc):
    """per voxel of the units `keys` [n,4096]: the pixel (u, v) it projects to in fp64, and whether that is clear: in front of the
    camera, 1e-3 px away from every pixel border and image edge, depth > 0 and the sdf 1e-5 inside the truncation"""
    keys = np.asarray(keys, dtype=np.int64)
    z_, y_, x_ = np.mgrid[0:R, 0:R, 0:R]
    g = lambda a, i: (((keys[:, a, None] * R + i.reshape(1, -1)) + 0.5) * voxel_length)
    pw = np.stack([g(0, x_), g(1, y_), g(2, z_)], 0)
    w2c = np.asarray(fr["w2c"], dtype=np.float64)
    x, y, z = np.einsum("ij,jnv->inv", w2c[:3, :3], pw) + w2c[:3, 3][:, None, None]
    H, W = fr["depth"].shape
    with np.errstate(divide="ignore", invalid="ignore"):
        uf, vf = x * fr["fx"] / z + fr["cx"] + 0.5, y * fr["fy"] / z + fr["cy"] + 0.5
    far = lambda a: np.abs(a - np.round(a)) >= 1e-3
    ok = (z > 0) & (uf >= 1e-4 + 1e-3) & (uf < W) & (vf >= 1e-4 + 1e-3) & (vf < H) & far(uf) & far(vf)
    ui, vi = np.where(ok, uf, 0).astype(np.int64), np.where(ok, vf, 0).astype(np.int64)
    d = fr["depth"].astype(np.float64)[vi, ui]
    sdf = (d - z) * np.sqrt(((ui - fr["cx"]) / fr["fx"]) ** 2 + ((vi - fr["cy"]) / fr["fy"]) ** 2 + 1)
    return ui, vi, ok & (d > 0) & (sdf > -sdf_trunc + 1e-5)


# ---- meshes for clean_mesh
KEPT, SMALL, REPEATED, ZERO_AREA, DUPLICATE = range(5)


def _strip_points(rng, m, origin):
    """m points of a zigzag strip, generic fp32 values: every three consecutive ones, and the other triples used below, span a fat
    triangle"""
    i = np.arange(m)
    p = np.stack([0.4 * i, (i & 1).astype(np.float64), np.zeros(m)], 1) + rng.uniform(-0.1, 0.1, (m, 3)) + np.asarray(origin)
    return p.astype(np.float32).astype(np.float64)


def _strip_faces(m, base):
    i = np.arange(m - 2)
    return np.stack([i, i + 1, i + 2], 1) + base


SMALL_FRONT = 12                                 # cleaning_small begins with this many copies whose originals come later
ORDERS = ((0, 1, 2), (1, 2, 0), (2, 0, 1), (0, 2, 1), (2, 1, 0), (1, 0, 2))


def cleaning_small(seed=2, min_len=100):
    """(vertices fp32 [V,3], faces int64 [F,3], colours fp32 [V,3]) for clean_mesh(min_len=100): lone vertices and strips of 99, 100
    and 101 vertices first, a strip of 99 that reaches 100 only through a face with a repeated index, then two long strips that
    carry faces with a repeated index, faces of three different indices with two bitwise equal positions, faces with
    p2 - p0 = 2 (p1 - p0) exactly, copies of kept faces in all six index orders before and after the original, and copies of
    dropped degenerate faces."""
    rng = np.random.default_rng(seed)
    V, F_front, F, F_back = [], [], [], []
    nv = lambda: sum(len(v) for v in V)
    V.append(_strip_points(rng, 3, (0, 50, 0)))                                       # three vertices used by no face
    for k, m in enumerate((99, 100, 101)):
        b = nv()
        V.append(_strip_points(rng, m, (0, 3.0 * k, 0)))
        F.append(_strip_faces(m, b))
        F_back.append(_strip_faces(m, b)[[4, 20]][:, [1, 2, 0]])                      # copies in every component, kept or not
    b = nv()                                                                          # 99 + 1: the 100th hangs on (a, a, b) alone
    V.append(_strip_points(rng, 100, (0, 12, 0)))
    F.append(_strip_faces(99, b))
    F.append(np.array([[b + 5, b + 5, b + 99]]))
    for k, m in enumerate((1000, 700)):
        b = nv()
        pts = _strip_points(rng, m + 7, (0, 20 + 3.0 * k, 5))
        # m strip vertices, then w = a copy of strip vertex 40's position, then q0, q1 = q0 + e, q2 = q0 + 2 e, then three spare
        w, q0 = b + m, b + m + 1
        pts[m] = pts[40]
        grid = 2.0 ** 19                                  # coordinates below 32 on this grid are fp32, and so are their small sums
        pts[m + 1] = np.round((pts[0] + [0.3, 0.5, 1.0] + rng.uniform(-0.1, 0.1, 3)) * grid) / grid
        e = np.round(rng.uniform(0.05, 0.3, 3) * grid) / grid
        pts[m + 2], pts[m + 3] = pts[m + 1] + e, pts[m + 1] + 2 * e
        V.append(pts)
        F.append(_strip_faces(m, b))
        F.append(np.array([[w, b + 45, b + 46], [q0, b, b + 1], [q0 + 1, b + 2, b + 3], [q0 + 2, b + 4, b + 5],   # fat ties
                           [b + 10, b + 10, b + 11], [b + 10, b + 11, b + 10], [b + 11, b + 10, b + 10], [b + 12, b + 12, b + 12],
                           [b + 40, w, b + 41], [b + 41, b + 40, w], [b + 40, b + 41, w], [w, b + 39, b + 40],
                           [q0, q0 + 1, q0 + 2], [q0 + 1, q0, q0 + 2], [q0 + 2, q0 + 1, q0], [q0 + 1, q0 + 2, q0]]))
        F_back.append(np.array([[b + 41, b + 40, w], [q0, q0 + 1, q0 + 2], [b + 10, b + 10, b + 11]]))    # copies of dropped faces
        orig = _strip_faces(m, b)
        for j, o in enumerate(ORDERS):                                                # six orders, before and after the original
            F_front.append(orig[[100 + 7 * j]][:, list(o)])
            F_back.append(orig[[200 + 7 * j]][:, list(o)])
        F_back.append(orig[[100]])                                                    # a third copy of one face
    verts = np.concatenate(V).astype(np.float32)
    assert np.array_equal(verts.astype(np.float64), np.concatenate(V))                # every position is an fp32
    assert len(F_front) == SMALL_FRONT
    faces = np.concatenate(F_front + F + F_back).astype(np.int64)
    cols = rng.uniform(0, 1, verts.shape).astype(np.float32)
    return verts, faces, cols


def exact_cross(verts, face):
    """the cross product (p1 - p0) x (p2 - p0) of fp32 positions in exact rational arithmetic"""
    p = [[fractions.Fraction(float(x)) for x in verts[i]] for i in face]
    a, b = [p[1][k] - p[0][k] for k in range(3)], [p[2][k] - p[0][k] for k in range(3)]
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def fused_cross_is_zero(verts, face):
    """whether a cross product whose components are fma(a, b, -fl(c d)) in fp32, on fp32 edge vectors, comes out as zero"""
    v = verts.astype(np.float32)
    e1, e2 = (v[face[1]] - v[face[0]]).astype(np.float64), (v[face[2]] - v[face[0]]).astype(np.float64)
    f = lambda a, b, c, d: np.float32(a * b - np.float64(np.float32(c * d)))          # a b is exact in fp64
    return not (f(e1[1], e2[2], e1[2], e2[1]) or f(e1[2], e2[0], e1[0], e2[2]) or f(e1[0], e2[1], e1[1], e2[0]))


def drop_reasons(verts, faces, min_len=100):
    """per face KEPT, SMALL (component below min_len), REPEATED (index), ZERO_AREA (exactly) or DUPLICATE (of a kept face of lower
    index), tested in that order; and the kept-vertex flags.  Independent of mesh_ref.clean but for the components."""
    lab = ref.components(len(verts), faces)
    keepv = np.bincount(lab, minlength=len(verts))[lab] >= min_len
    out = np.full(len(faces), KEPT)
    seen = set()
    for i, f in enumerate(faces.tolist()):
        if not keepv[f[0]]:
            out[i] = SMALL
        elif len(set(f)) < 3:
            out[i] = REPEATED
        elif not any(exact_cross(verts, f)):
            out[i] = ZERO_AREA
        elif tuple(sorted(f)) in seen:
            out[i] = DUPLICATE
        else:
            seen.add(tuple(sorted(f)))
    return out, keepv


LARGE_STRIPS = 10647      # V = 100 S = 1 064 700 > 2^20 + 4096 (260 scan blocks), F = 197 S = 2 097 459 > 2^21 (513 scan blocks)


def cleaning_large(strips=LARGE_STRIPS, seed=3):
    """independent strips of 99, 100 and 101 vertices in rotation (strips a multiple of 3), built without a Python loop.  A strip of
    m vertices has the faces (i, i+1, i+2) and (i, i+1, i+3), vertex-major, a copy of its face (7, 8, 9) as (9, 7, 8) and one
    degenerate face.  In an even strip that is (20, 21, 20); in an odd strip the last vertex has the position of vertex m - 6 and
    the face is (m-10, m-6, m-1): two bitwise equal edge vectors.  The copies of the odd strips stand before all other faces (so the
    copy stays and the original goes), those of the even strips after them, and the degenerate faces last.
    Returns dict(vertices, faces, colors, keep_vertex bool [V], vertex_map int32 [V], keep_face bool [F]): the answer of clean_mesh
    (min_len=100) in closed form."""
    assert strips % 3 == 0
    g = torch.Generator().manual_seed(seed)
    S = torch.arange(strips)
    lens = 99 + S % 3
    ends = torch.cumsum(lens, 0)
    starts = ends - lens
    V = int(ends[-1])
    sid = torch.repeat_interleave(S, lens)
    loc = torch.arange(V) - starts[sid]
    m = lens[sid]
    pos = torch.stack([0.4 * loc, (loc & 1).double(), torch.zeros(V, dtype=torch.float64)], 1)
    pos = pos + (torch.rand(V, 3, generator=g, dtype=torch.float64) * 0.2 - 0.1)
    pos[:, 1] += 3.0 * (sid % 1000)
    pos[:, 2] += 3.0 * (sid // 1000)
    pos = pos.float()
    odd = (S % 2) == 1
    last, twin = ends - 1, ends - 6
    pos[last[odd]] = pos[twin[odd]]
    v = torch.arange(V)
    body = torch.stack([torch.stack([v, v + 1, v + 2], 1), torch.stack([v, v + 1, v + 3], 1)], 1)          # [V, 2, 3]
    exists = torch.stack([loc < m - 2, loc < m - 3], 1)
    body_sid = sid[:, None].expand(V, 2)[exists]
    is_orig = torch.stack([loc == 7, torch.zeros(V, dtype=torch.bool)], 1)[exists]
    body = body[exists]
    copies = torch.stack([starts + 9, starts + 7, starts + 8], 1)
    degenerate = torch.where(odd[:, None], torch.stack([ends - 10, ends - 6, ends - 1], 1),
                             torch.stack([starts + 20, starts + 21, starts + 20], 1))
    faces = torch.cat([copies[odd], body, copies[~odd], degenerate]).int()
    kept_strip = lens >= 100
    keep_face = torch.cat([kept_strip[odd], kept_strip[body_sid] & ~(is_orig & odd[body_sid]),
                           torch.zeros(int((~odd).sum()) + strips, dtype=torch.bool)])
    keep_vertex = kept_strip[sid]
    vmap = torch.where(keep_vertex, torch.cumsum(keep_vertex.long(), 0) - 1, torch.full((V,), -1)).int()
    colors = torch.rand(V, 3, generator=g)
    return dict(vertices=pos, faces=faces, colors=colors, keep_vertex=keep_vertex, vertex_map=vmap, keep_face=keep_face)
