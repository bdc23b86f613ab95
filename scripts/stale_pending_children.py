#!/usr/bin/env python3
"""How much of a closest-hit walk is spent on children that were recorded as pending BEFORE the hit was known?  CPU only.

The traversal (csrc/bvh8.h: traverse8, the loop k_trace runs per lane) culls a node's children against the best distance known when the
NODE is visited; a child group pushed earlier stays on the stack although a later hit may lie in front of all of it.  An upper bound on what
any mechanism that drops such entries could save: trace every ray twice through the host harness (tests/native/host_bvh8.cpp, the same
template compiled for the CPU) -- once as the device does, from tmax = FLT_MAX, and once with tmax = the hit distance found x (1 + 1e-6), i.e.
with the final answer known in advance -- and compare node visits and triangle tests per ray.

Rays: the camera rays of the bench frame's Soup(100 000) (one per pixel of a 640 x 360 film), then three generations of bounce rays, each
leaving the previous generation's hits in a cosine-distributed direction about the face normal (numpy, seeded): incoherent rays like the
ones k_trace spends its time on.

    python scripts/stale_pending_children.py [triangles] > profiles/r07_stale_pending_children.md
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import tri_abc  # noqa: E402
from oracle import oracle as orc  # noqa: E402
from phosphorus_mk2_amd import abi, scenes  # noqa: E402

F = np.float32
FMAX = np.finfo(F).max


def harness():
    d = os.path.join(ROOT, "tests", "native")
    so = os.path.join(d, "libhost_bvh8.so")
    src = [os.path.join(d, "host_bvh8.cpp"), os.path.join(ROOT, "phosphorus_mk2_amd", "csrc", "bvh_build.cpp")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in src):
        subprocess.run(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-march=haswell", "-mfma", "-ffp-contract=off", "-pthread", "-DPHX_STUDY_KNOBS=1", "-o", so] + src, check=True)
    lib = C.CDLL(so)
    lib.hb8_build.restype = C.c_void_p; lib.hb8_build.argtypes = [abi.f32p, C.c_uint32, C.c_int]
    lib.hb8_trace.argtypes = [C.c_void_p, C.c_uint32, abi.f32p, abi.f32p, abi.f32p, C.c_int, abi.f32p, abi.f32p, abi.f32p, abi.u32p, C.POINTER(C.c_uint64)]
    lib.hb8_trace.restype = C.c_int
    return lib


def trace(lib, h, o, d, tmax):
    n = len(tmax)
    o = np.ascontiguousarray(o, F); d = np.ascontiguousarray(d, F); tmax = np.ascontiguousarray(tmax, F)
    t = np.zeros(n, F); u = np.zeros(n, F); v = np.zeros(n, F); prim = np.zeros(n, np.uint32)
    cnt = (C.c_uint64 * 2)()
    fp = lambda a: a.ctypes.data_as(abi.f32p)
    lib.hb8_trace(h, n, fp(o), fp(d), fp(tmax), 0, fp(t), fp(u), fp(v), prim.ctypes.data_as(abi.u32p), cnt)
    return t, prim, cnt[0] / n, cnt[1] / n


def bounce(rng, abc, o, d, t, prim):
    """cosine-distributed directions about the hit faces' normals (turned towards the incoming ray), from just above the hit points"""
    hit = prim != 0xffffffff
    o, d, t, prim = o[hit], d[hit], t[hit], prim[hit]
    tri = abc[prim].reshape(-1, 3, 3).astype(np.float64)
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    n[(n * d).sum(1) > 0] *= -1.0
    p = o.astype(np.float64) + d.astype(np.float64) * t[:, None]
    a = np.where(np.abs(n[:, :1]) < 0.9, [[1.0, 0.0, 0.0]], [[0.0, 1.0, 0.0]])
    tx = np.cross(n, a); tx /= np.linalg.norm(tx, axis=1, keepdims=True)
    ty = np.cross(n, tx)
    u1, u2 = rng.random(len(n)), rng.random(len(n))
    r, phi = np.sqrt(u1), 2.0 * np.pi * u2
    w = tx * (r * np.cos(phi))[:, None] + ty * (r * np.sin(phi))[:, None] + n * np.sqrt(1.0 - u1)[:, None]
    return (p + n * 1e-4).astype(F), w.astype(F)


def main():
    ntri = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
    W, H = 640, 360
    sc = scenes.soup(ntri, width=W, height=H)
    abc = tri_abc(sc)
    lib = harness()
    h = lib.hb8_build(abc.ctypes.data_as(abi.f32p), len(abc), 8)
    orc.load()
    O = orc.Oracle(sc, spp=1)
    rays = [O.camera_rays((x, y, 40, 24), 0, seed=1) for y in range(0, H, 24) for x in range(0, W, 40)]  # tile by tile (the oracle hands out at most 1 024 rays a call)
    o, d = np.concatenate([r[0] for r in rays]), np.concatenate([r[1] for r in rays])
    rng = np.random.default_rng(7)
    print(f"# Node visits and triangle tests a closest-hit walk spends on children recorded before the hit was known\n")
    print(f"`python scripts/stale_pending_children.py {ntri}`: Soup({ntri}), host-built tree, `traverse8` through `tests/native/host_bvh8.cpp`; each set of rays")
    print("traced as the device traces it (tmax = FLT_MAX) and again with tmax = the hit distance found x (1 + 1e-6).  The hits of both walks are asserted identical.\n")
    print("| rays | count | hit | node visits / ray | ... hit distance known | saved | triangle tests / ray | ... hit distance known | saved |")
    print("|---|---|---|---|---|---|---|---|---|")
    for gen in range(4):
        t, prim, nv, tt = trace(lib, h, o, d, np.full(len(o), FMAX, F))
        hit = prim != 0xffffffff
        with np.errstate(over="ignore"):  # a miss carries FLT_MAX
            known = np.where(hit, t * F(1.0 + 1e-6), FMAX).astype(F)
        t2, prim2, nv2, tt2 = trace(lib, h, o, d, known)
        assert np.array_equal(prim, prim2) and np.array_equal(t.view(np.uint32)[hit], t2.view(np.uint32)[hit])
        name = "camera rays" if gen == 0 else f"bounce {gen}"
        print(f"| {name} | {len(o)} | {hit.mean():.3f} | {nv:.2f} | {nv2:.2f} | {100 * (1 - nv2 / nv):.1f} % | {tt:.2f} | {tt2:.2f} | {100 * (1 - tt2 / tt):.1f} % |")
        o, d = bounce(rng, abc, o, d, t, prim)
    print("\nThe saving is an upper bound for any scheme that drops stacked children behind the hit: it also contains the children culled EARLIER on the")
    print("way down because the bound was tight from the start, which no such scheme can have.  Rays that miss save nothing (their bound stays FLT_MAX).")


if __name__ == "__main__":
    main()
