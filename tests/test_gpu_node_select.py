"""The device path of node_hit8 (csrc/bvh8.h) picks each child's near and far plane by the SIGN of the ray's reciprocal direction, which
make_ray_ctx forms from directions that may be +-0, below its `tiny` threshold (+-1e-21: the reciprocal is clamped to +-1e20), just above it
(+-1e-19) or huge (+-3e38: the device's reciprocal flushes to +-0).  That path is not compiled for the host, so it is checked through the
stage-level hook: phx_dev_trace (k_trace_rays: traverse8 on the device, closest-hit and any-hit) against the same traversal on the CPU
(tests/native/host_bvh8.cpp), (t, u, v, primitive) bit for bit, in one launch per mode.

Scene: Soup(62) + its two light triangles = 64 triangles, built by the host builder on both sides (the same tree: an any-hit walk reports the
first triangle it meets).  Rays: every octant, every axis-parallel direction, and directions with one or two components replaced by each of
+-0, +-1e-21, +-1e-19, +-3e38 on every choice of major axis."""
import ctypes as C
import itertools

import numpy as np
import pytest

from conftest import tri_abc

pytestmark = pytest.mark.gpu

SPECIAL = [0.0, -0.0, 1e-21, -1e-21, 1e-19, -1e-19, 3e38, -3e38]
FLT_MAX = np.finfo(np.float32).max


def rays():
    rng = np.random.default_rng(5)
    centre = np.array([0.0, 0.0, -2.5])
    O, D = [], []
    # every octant: 64 random directions per sign pattern, aimed at a point of the cloud from outside it
    for sx, sy, sz in itertools.product((1.0, -1.0), repeat=3):
        d = np.abs(rng.normal(size=(64, 3))) + 0.05
        d *= (sx, sy, sz); d /= np.linalg.norm(d, axis=1, keepdims=True)
        O.append(centre + rng.uniform(-0.9, 0.9, (64, 3)) - 4.0 * d); D.append(d)
    # a 3 x 3 grid of parallel rays through the cloud along every +-axis: plain, and with the two minor components replaced by every pair of specials
    grid = [(a, b) for a in (-0.5, 0.05, 0.6) for b in (-0.55, 0.1, 0.5)]
    for axis in range(3):
        m0, m1 = [k for k in range(3) if k != axis]
        for sign in (1.0, -1.0):
            minors = [(0.0, 0.0, 1.0), (0.0, 0.0, 3e38)] + [(s0, s1, 1.0) for s0, s1 in itertools.product(SPECIAL, repeat=2)]  # (.., 3e38): the huge component as the major one
            for (a, b), (s0, s1, major) in itertools.product(grid, minors):
                p = centre.copy(); p[m0] += a; p[m1] += b; p[axis] -= sign * 4.0
                d = np.zeros(3); d[axis] = sign * major; d[m0] = s0; d[m1] = s1
                O.append(p[None]); D.append(d[None])
    # one special component on a diagonal ray, every axis
    for axis, s in itertools.product(range(3), SPECIAL):
        for k in range(8):
            d = np.array([0.6, -0.7, -0.5]) * (1.0 if k & 1 else -1.0); d[axis] = s
            p = centre + rng.uniform(-0.5, 0.5, 3) - 4.0 * np.where(np.abs(d) < 2.0, d, 0.0)
            O.append(p[None]); D.append(d[None])
    o = np.ascontiguousarray(np.concatenate(O), np.float32); d = np.ascontiguousarray(np.concatenate(D), np.float32)
    return o, d


def test_stage_hook_matches_the_host_walk_on_every_sign_of_the_reciprocal(host_bvh8):
    from phosphorus_mk2_amd import scenes, xpu
    xpu.load_library()
    sc = scenes.soup(62, width=64, height=64)
    abc = tri_abc(sc)
    assert len(abc) == 64
    o, d = rays()
    n = len(o)
    assert 3000 <= n <= 6000
    # the special values reach make_ray_ctx as written (float32): -0 keeps its sign, 1e-21 is below tiny = 1e-20, 1e-19 above it
    assert np.signbit(d[d == 0]).any() and (np.abs(d[d != 0]).min() < 1e-20) and (np.abs(d).max() > 2.9e38)
    dev = xpu.HipDevice.make(xpu.Options(samples_per_pixel=1, paths_per_sample=1, path_depth=2, bvh_builder="host"))
    dev.preprocess(sc)
    h = host_bvh8.hb8_build(abc.ctypes.data_as(C.POINTER(C.c_float)), len(abc), 1)
    try:
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        hits = {}
        for shadow, tmax in ((False, np.full(n, FLT_MAX, np.float32)), (True, np.full(n, 4.5, np.float32))):
            g = dev.trace(o, d, tmax, shadow=shadow)
            t = np.zeros(n, np.float32); u = np.zeros(n, np.float32); v = np.zeros(n, np.float32); prim = np.zeros(n, np.uint32)
            host_bvh8.hb8_trace(h, n, fp(o), fp(d), fp(tmax), 1 if shadow else 0, fp(t), fp(u), fp(v), prim.ctypes.data_as(C.POINTER(C.c_uint32)), None)
            bad = np.flatnonzero((g["prim"] != prim) | (g["t"].view(np.uint32) != t.view(np.uint32)) | (g["u"].view(np.uint32) != u.view(np.uint32)) | (g["v"].view(np.uint32) != v.view(np.uint32)))
            assert len(bad) == 0, (shadow, len(bad), [(o[i].tolist(), d[i].tolist(), float(g["t"][i]), float(t[i]), int(g["prim"][i]), int(prim[i])) for i in bad[:5]])
            assert np.array_equal(g["hit"], prim != 0xffffffff)
            hits[shadow] = prim != 0xffffffff
        # the rays do meet the cloud: in every octant, along every axis in both directions, and with a special value in the direction
        octant = (d[:512, 0] < 0) * 4 + (d[:512, 1] < 0) * 2 + (d[:512, 2] < 0)
        for k in range(8):
            assert hits[False][:512][octant == k].sum() >= 8, k
        special = np.isin(np.abs(d), np.abs(np.array(SPECIAL, np.float32))).any(axis=1)
        assert hits[False][special].sum() > 200 and hits[True][special].sum() > 100 and (~hits[False][special]).sum() > 200
        for s in SPECIAL:
            sel = (d.view(np.uint32) == np.array([s], np.float32).view(np.uint32)[0]).any(axis=1)
            assert hits[False][sel].sum() >= 10, s
    finally:
        host_bvh8.hb8_free(h)
        dev.close()
