"""The BVH8 refit (csrc/bvh_refit.h) without a GPU: the host refit (csrc/bvh_refit_host.cpp through tests/native/refit_host.cpp) equals the
numpy model of the rule (tests/refit_model.py) byte for byte on host-built trees of the builder tests' cases, under six motions; the
refitted trees pass the finished-tree checks of tests/test_bvh_model.py against the NEW triangles; and the same sources, as a stand-alone
program under AddressSanitizer and UBSan, end clean.  The device's refit is held to the same model in tests/test_gpu_update_geometry.py.

Which finished-tree checks apply to a refitted tree (test_bvh_model's letters):
  a  partition and records   unchanged: every primitive in one record, v0 e0 e1 = a, b - a, c - a of the NEW triangles, material words, counts
  b  layout                  unchanged: the refit keeps valid, imask and the elements' places
  c  origin and scale        unchanged, on the new boxes: the origin at or below the node's box and less than a cell below, the least exponent
  d  stored boxes            unchanged, on the new boxes: containment and at most 1.001 grid units of slack
  e, f, g, h                 do NOT apply: the radix structure, the slot greedy and the collapse's cost describe the geometry the tree was
                             BUILT for; a refit keeps those cuts and slots for other triangles (limits)"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import bvh_model as M
import native_lib as NL
import refit_model as R
from conftest import bits_equal
from native_lib import CSRC, NATIVE
from test_bvh_model import check_layout, check_origin_and_scale, check_partition_and_records, check_stored_boxes
from test_gpu_bvh_builder import _case

F = np.float32

# the host library of this module: a registry of its own, as tests/test_tile_map.py keeps one
REGISTRY = {"refit_host": ([os.path.join(NATIVE, "refit_host.cpp"), os.path.join(CSRC, "bvh_build.cpp"), os.path.join(CSRC, "bvh_refit_host.cpp")], ["-pthread"])}

CASES = ["n2", "n3", "n8", "n9", "n63", "n64", "n65", "n255", "n256", "n257", "n1025", "n2049", "quads", "copies50", "cluster_outlier", "flat", "line", "mixed"]
MOTIONS = ["identity", "rigid", "rigid_half", "far", "plane", "wobble"]


def rotation(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]); ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]); rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return (rz @ ry @ rx).astype(F)


def moved(abc, motion, seed=0):
    """(n, 9) float32 -> the triangles after `motion`, float32 (whatever the rounding: the refit takes the floats it is given)"""
    v = np.ascontiguousarray(abc, F).reshape(-1, 3, 3).copy()
    rigid = lambda p: (p @ rotation(0.3, -0.7, 1.1).T + np.array([0.25, -0.4, 0.6], F)).astype(F)
    if motion == "rigid":
        v = rigid(v)
    elif motion == "rigid_half":
        v[:len(v) // 2] = rigid(v[:len(v) // 2])
    elif motion == "far":
        v = (v + np.array([1.0e4, 0.0, 0.0], F)).astype(F)
    elif motion == "plane":
        v[:, :, 1] = F(0.3)
    elif motion == "wobble":
        v = (v + np.random.default_rng(seed).uniform(-0.05, 0.05, v.shape)).astype(F)
    else:
        assert motion == "identity"
    return np.ascontiguousarray(v.reshape(-1, 9), F)


@functools.lru_cache(None)
def lib():
    from phosphorus_mk2_amd import abi
    l = NL.load("refit_host", registry=REGISTRY)
    l.hr_build.restype = C.c_void_p; l.hr_build.argtypes = [abi.f32p, C.c_uint32, C.c_int]
    l.hr_free.argtypes = [C.c_void_p]
    l.hr_info.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    l.hr_copy_pool.restype = C.c_uint64; l.hr_copy_pool.argtypes = [C.c_void_p, abi.u32p, C.c_uint64, abi.f32p]
    l.hr_refit.argtypes = [C.c_void_p, abi.f32p, C.c_uint32]
    l.hr_refit_pool.argtypes = [abi.u32p, C.c_uint32, abi.f32p, C.c_uint32, abi.f32p]
    return l


def _copy(h):
    from phosphorus_mk2_amd import abi
    grid = np.zeros(6, F)
    n_el = lib().hr_copy_pool(h, None, 0, grid.ctypes.data_as(abi.f32p))
    pool = np.zeros((n_el, 16), np.uint32)
    assert lib().hr_copy_pool(h, pool.ctypes.data_as(abi.u32p), n_el, grid.ctypes.data_as(abi.f32p)) == n_el
    return pool, grid[:3].copy(), grid[3:].copy()


@functools.lru_cache(None)
def built(name):
    """-> (abc, pool, glo, gcell, counts) of the host builder's tree of the case"""
    from phosphorus_mk2_amd import abi
    _, abc, _ = _case(name)
    h = lib().hr_build(abc.ctypes.data_as(abi.f32p), len(abc), 4)
    try:
        info = (C.c_uint64 * 3)(); lib().hr_info(h, info)
        return (abc,) + _copy(h) + (tuple(info),)
    finally:
        lib().hr_free(h)


def host_refit(pool, abc):
    """refit a copy of `pool` with the host library -> (pool, glo, gcell)"""
    from phosphorus_mk2_amd import abi
    out = np.ascontiguousarray(pool, np.uint32).copy(); grid = np.zeros(6, F)
    abc = np.ascontiguousarray(abc, F)
    assert lib().hr_refit_pool(out.ctypes.data_as(abi.u32p), len(out), abc.ctypes.data_as(abi.f32p), len(abc), grid.ctypes.data_as(abi.f32p)) == 0
    return out, grid[:3].copy(), grid[3:].copy()


def check_refitted(pool, glo, gcell, abc, material, counts):
    """items a, b, c, d against the new triangles"""
    W = M.walk_pool(pool, glo, gcell)
    boxes = M.leaf_boxes(abc)
    check_partition_and_records(W, abc, material, counts)
    check_layout(W)
    cb = M.child_boxes(W, boxes.ilo, boxes.ihi)
    check_origin_and_scale(W, cb)
    check_stored_boxes(W, cb, counts)


@pytest.mark.parametrize("motion", MOTIONS)
@pytest.mark.parametrize("name", CASES)
def test_host_refit_is_the_model(name, motion):
    abc, pool, glo, gcell, counts = built(name)
    new = moved(abc, motion, seed=len(abc))
    got, hlo, hcell = host_refit(pool, new)
    want, mlo, mcell = R.refit(pool, glo, gcell, new)
    assert bits_equal(hlo, mlo) and bits_equal(hcell, mcell), "the grid of the new bounds"
    diff = np.nonzero((got != want).any(1))[0]
    assert len(diff) == 0, f"{len(diff)} of {len(pool)} pool elements differ from the model, the first at {diff[:4].tolist()}"
    if motion == "identity":  # the refit of an unmoved scene is the builder's own emission
        assert np.array_equal(got, pool) and bits_equal(hlo, glo) and bits_equal(hcell, gcell)
    check_refitted(got, hlo, hcell, new, np.zeros(len(abc), np.uint32), counts)


def test_refit_there_and_back_restores_every_byte():
    abc, pool, glo, gcell, _ = built("n1025")
    there, lo1, cell1 = host_refit(pool, moved(abc, "rigid"))
    assert not np.array_equal(there, pool)
    back, lo2, cell2 = host_refit(there, abc)
    assert np.array_equal(back, pool) and bits_equal(lo2, glo) and bits_equal(cell2, gcell)


def test_a_pool_that_is_no_tree_is_refused_untouched():
    from phosphorus_mk2_amd import abi
    abc, pool, _, _, _ = built("n65")
    grid = np.zeros(6, F)
    call = lambda p, t: lib().hr_refit_pool(p.ctypes.data_as(abi.u32p), len(p), t.ctypes.data_as(abi.f32p), len(t), grid.ctypes.data_as(abi.f32p))
    for word, value in ((3, 0), (3, len(pool)), (3, 0xffffffff)):  # the root's child_base: behind itself, past the pool, wrapping
        bad = pool.copy(); bad[0, word] = value; before = bad.copy()
        assert call(bad, abc) == 1 and np.array_equal(bad, before)
    fewer = pool.copy()
    assert call(fewer, np.ascontiguousarray(abc[:-1])) == 1 and np.array_equal(fewer, pool)  # a record names a primitive outside the scene
    assert call(pool[:-1].copy(), abc) == 1                                                    # an element short


def test_host_refit_under_sanitizers(tmp_path):
    """native_lib.run_sanitized's pattern with this module's own source list: the stand-alone program ends with status 0 and nothing on stderr"""
    sources, flags = REGISTRY["refit_host"]
    exe = str(tmp_path / "refit_host_asan")
    subprocess.run([NL.CXX] + NL.SANITIZE + ["-DHOST_REFIT_MAIN"] + NL.HOST_FLAGS + flags + ["-o", exe] + sources, check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", (r.stdout[-2000:], r.stderr[-2000:])
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == 4 and all(l.endswith("as-expected") for l in lines), r.stdout
