"""Synthetic inputs of the reprojection tests (tests/test_reproject.py, tests/test_gpu_reproject.py): cameras, a world of bounded planes traced
in numpy into guide films and normals, and accumulator films whose counts and values are chosen as test_accumulate.exact_film chooses them.
No code shared with the library or with the model (tests/reproject64.py): the rays here are built forwards, camera to world."""
import math

import numpy as np

F, D = np.float32, np.float64


def rot_y(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[c, 0, -s], [0, 1, 0], [s, 0, c]], D)


def rot_x(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[1, 0, 0], [0, c, s], [0, -s, c]], D)


def camera(width, height, origin=(0.0, 0.0, 0.0), m3=None, fov=1.1, aperture_radius=0.0, focal_distance=1.0):
    """a CameraDesc: rows of m3 are the camera's x, y, z axes in the world (row-vector convention), it looks down its -z"""
    from phosphorus_mk2_amd.scenes import CameraDesc
    M = np.eye(4, dtype=D)
    if m3 is not None:
        M[:3, :3] = m3
    M[3, :3] = origin
    return CameraDesc(width, height, fov=fov, to_world=M.astype(F), focal_distance=focal_distance, aperture_radius=aperture_radius)


# planes: (point, normal, lowest world x, highest world x)
FLOOR = ((0.0, -1.0, 0.0), (0.0, 1.0, 0.0), -1e30, 1e30)
WALL = ((0.0, 0.0, -10.0), (0.0, 0.0, 1.0), -6.0, 6.0)   # bounded: beside it the sky
WORLD = [FLOOR, WALL]
OPEN_WALL = [((0.0, 0.0, -10.0), (0.0, 0.0, 1.0), -1e30, 1e30)]  # every ray that looks down -z meets it: for films of one row or column, which look past the room


def trace(planes, cam, ox=0.0, oy=0.0):
    """the guide film (H, W, 8) f32 and the normals (H, W, 3) f32 of `planes` under CameraDesc `cam`: pixel (x, y)'s ray leaves through film point
    (x + ox, y + oy) (ox, oy scalars or (H, W) arrays: where inside the pixel the mean hit lies); a ray that hits nothing has coverage 0"""
    W, H = cam.width, cam.height
    M = cam.to_world.astype(D)
    zoom, ratio = 1.12 * math.tan(0.5 * float(F(cam.fov))), W / H
    ys, xs = np.mgrid[0:H, 0:W].astype(D)
    nx, ny = (xs + ox) / W - 0.5, 0.5 - (ys + oy) / H
    d = np.stack([nx * ratio * zoom, ny * zoom, -np.ones_like(nx)], -1) @ M[:3, :3]
    o = M[3, :3]
    best = np.full((H, W), np.inf)
    normal = np.zeros((H, W, 3))
    for point, n, lo, hi in planes:
        n, point = np.asarray(n, D), np.asarray(point, D)
        with np.errstate(all="ignore"):
            t = ((point - o) @ n) / (d @ n)
            x = o[0] + t * d[..., 0]
            hit = np.isfinite(t) & (t > 1e-9) & (x >= lo) & (x <= hi) & (t < best)
        best = np.where(hit, t, best)
        normal[hit] = n
    hit = np.isfinite(best)
    g = np.zeros((H, W, 8), F)
    g[..., 0:3] = 1.0
    g[..., 3] = hit
    t = np.where(hit, best, 0.0)
    g[..., 4:7] = np.where(hit[..., None], o + t[..., None] * d, 0.0)
    g[..., 7] = np.where(hit, t * np.linalg.norm(d, axis=-1), 0.0)
    return g, np.where(hit[..., None], normal, 0.0).astype(F)


def layout(pc=4):
    """(xstride, (normals, m2, samples) offsets) of xpu.accumulator(W, H, pc, normals=True)"""
    return pc + 7, (pc, pc + 3, pc + 6)


def accumulator(normals, pc=4, seed=3, xstride=None, offs=None, specials=True):
    """an accumulator film over `normals` (H, W, 3): per pixel n in {4, 8, 16, 32} integer samples in [0, 64], V = sum / n and
    m2 = (n * sum of squares - sum^2) / n^3, both exact in fp32 (test_accumulate.exact_film); floats of no channel are random.  specials: a
    sprinkle of pixels that are no tap — NaN and infinite colours, a negative m2, n = 1, n = NaN, a NaN normal."""
    H, W, _ = normals.shape
    xs, o = layout(pc)
    xstride, (no, mo, so) = xstride or xs, offs or o
    rng = np.random.default_rng(seed)
    n = rng.choice([4, 8, 16, 32], (H, W))
    acc = rng.uniform(1.0, 2.0, (H, W, xstride)).astype(F)
    for k in (4, 8, 16, 32):
        x = rng.integers(0, 65, (H, W, 3, k)).astype(D)
        s1, s2 = x.sum(-1), (x * x).sum(-1)
        V, m2 = s1 / D(k), (k * s2 - s1 * s1) / D(k ** 3)
        pick = n == k
        acc[..., 0:3][pick] = V[pick]
        acc[..., mo:mo + 3][pick] = m2[pick]
    acc[..., so] = n
    acc[..., no:no + 3] = normals
    if specials and H * W >= 64:
        flat = acc.reshape(-1, xstride)
        where = rng.choice(H * W, 6, replace=False)
        flat[where[0], 1] = np.nan
        flat[where[1], mo] = np.inf
        flat[where[2], mo + 2] = -0.25
        flat[where[3], so] = 1.0
        flat[where[4], so] = np.nan
        flat[where[5], no + 1] = np.nan
    return acc


def spoil_guides(g, seed=4):
    """a copy of a guide film with a NaN albedo, an infinite position, a NaN distance and a pixel of coverage 0 sprinkled in"""
    g = g.copy()
    H, W, xs = g.shape
    if H * W >= 64:
        rng = np.random.default_rng(seed)
        where = rng.choice(H * W, 4, replace=False)
        flat = g.reshape(-1, xs)
        flat[where[0], 0] = np.nan
        flat[where[1], 5] = np.inf
        flat[where[2], 7] = np.nan
        flat[where[3], 3] = 0.0
    return g


def pairs(W, H):
    """the camera pairs of the tests: name -> (camera_from, camera_to)"""
    base = camera(W, H)
    return {
        "identical": (base, camera(W, H)),
        "translation": (base, camera(W, H, origin=(0.35, 0.1, 0.2))),
        "rotation": (base, camera(W, H, m3=rot_y(0.12) @ rot_x(-0.05))),
        "both": (base, camera(W, H, origin=(-0.4, 0.2, 0.5), m3=rot_y(-0.1))),
        "behind": (base, camera(W, H, origin=(0.0, 0.5, 6.0), m3=rot_x(-0.25))),  # it sees floor that lies behind the old camera
    }
