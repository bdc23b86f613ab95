"""The device BVH builder (csrc/bvh_gpu.hip) against the model of its stages (tests/bvh_model.py): is the tree the one the code claims to
build — Karras' radix tree over the extended Morton keys, collapsed by the optimal cut of k_collapse_dp's programme, children in octant
order on minimal grids, phx_stats.bvh_cost_model the cost of the tree produced?  Hits, containment and reproducibility (test_gpu_parity.py)
cannot tell: any tree that contains its geometry gives the same hits.

Per case the tree is built once (bvh_builder="device"), read back (bvh_pool) and checked in this order, so that a failure names the stage
(the checks are those of tests/test_bvh_model.py, where the host builder passes them without a GPU):
  a partition and records, b layout, c origin and scale, d stored boxes, e radix structure (DP_LEVELS = 4), f slots,
  g bvh_cost_model = tree_cost(finished tree) within chain * 2^-24, h bvh_cost_model = collapse_optimum(radix tree)[root] within 2 * chain * 2^-24
where chain is the number of fp32 roundings on the longest path into the root's sum, counted by the model (bvh_model.collapse_optimum).
Items e and f assume exact fp32 agreement of keys and boxes; no case had to be restricted to a dyadic lattice.

A scene needs one emissive face set, so the helper hangs the LAST triangle of an (n, 9) array on a black emitter, in a mesh of its own; the
triangles and their order are the array's.

Observed on an MI355X: |bvh_cost_model - model| / model, and the bounds of g and h.  The two models gave the same value on every case (the
device's cut is the float64 optimum), so one difference is listed; the largest ratio to a bound is 0.148 (g, n9), 0.069 for h.
  case             difference   g bound    h bound   | case             difference   g bound    h bound
  n2               2.94e-08     4.77e-07   9.54e-07  | quads            7.62e-08     1.67e-06   3.81e-06
  n3               1.97e-08     5.36e-07   1.19e-06  | copies2          5.05e-08     4.77e-07   9.54e-07
  n8               5.49e-08     6.56e-07   1.67e-06  | copies50         5.67e-08     9.54e-07   2.15e-06
  n9               1.15e-07     7.75e-07   1.67e-06  | copies257        5.98e-08     1.25e-06   2.86e-06
  n63              1.16e-07     1.19e-06   2.86e-06  | cluster_outlier  1.46e-08     2.15e-06   4.53e-06
  n64              2.85e-09     1.13e-06   2.62e-06  | flat             1.39e-08     1.67e-06   3.81e-06
  n65              3.15e-08     1.13e-06   2.62e-06  | line             1.39e-08     1.49e-06   3.58e-06
  n255             3.95e-08     1.43e-06   3.34e-06  | mixed            2.80e-09     1.85e-06   4.29e-06
  n256             3.00e-08     1.55e-06   3.34e-06  | soup2000         7.15e-08     2.03e-06   4.29e-06
  n257             1.66e-08     1.43e-06   3.34e-06  | showroom2000     1.01e-07     2.74e-06   6.20e-06
  n1025            1.02e-08     1.85e-06   3.81e-06  | stress           4.02e-08     2.44e-06   5.25e-06
  n2049            5.79e-08     1.85e-06   4.29e-06  |
"""
import hashlib

import numpy as np
import pytest

import bvh_model as M
from conftest import tri_abc
from test_bvh_model import (CN, CT, check_cost, check_layout, check_origin_and_scale, check_partition_and_records, check_radix_structure, check_slots,
                            check_stored_boxes, cloud, mixed_sizes)

pytestmark = pytest.mark.gpu

DP_LEVELS = 4  # bvh_gpu.hip: binary levels below a node within which its cut is searched


@pytest.fixture(scope="module")
def xpu():
    from phosphorus_mk2_amd import xpu
    xpu.load_library()
    return xpu


@pytest.fixture(scope="module")
def dev(xpu):
    d = xpu.HipDevice.make(xpu.Options(samples_per_pixel=1, paths_per_sample=1, bvh_builder="device"))
    yield d
    d.close()


def scene_of(abc):
    """(n, 9) float32, n >= 2 -> (SceneDesc, material word per primitive): the first n - 1 triangles in one mesh and one face set on a diffuse
    material, the last one on a black emitter (flatten_scene refuses a scene without an emissive face set); a 16 x 16 film"""
    from phosphorus_mk2_amd import scenes
    abc = np.ascontiguousarray(abc, np.float32).reshape(-1, 9)
    n = len(abc)
    mesh = lambda t, mat: scenes.MeshDesc(vertices=t.reshape(-1, 3), faces=np.arange(3 * len(t), dtype=np.uint32).reshape(-1, 3),
                                          sets=[(mat, np.arange(len(t), dtype=np.uint32))])
    sc = scenes.SceneDesc([mesh(abc[:-1], 0), mesh(abc[-1:], 1)], [scenes.diffuse(0.73, 0.73, 0.73), scenes.emitter(0.0, 0.0, 0.0)],
                          scenes.CameraDesc(16, 16), name=f"tris{n}")
    return sc, np.array([0] * (n - 1) + [1], np.uint32)


def scene_materials(sc):
    """the material word of every primitive, in tri_abc order: material | smooth << 31 (flatten_scene)"""
    return np.concatenate([(np.uint32(mat) | (m.smooth[faces].astype(np.uint32) << np.uint32(31))) for m in sc.meshes for mat, faces in m.sets]).astype(np.uint32)


def _quads(rng, pairs):
    """axis-aligned rectangles in the coordinate planes, each as two triangles (a b c), (a c d): the halves have identical boxes"""
    out = np.zeros((pairs, 2, 3, 3), np.float32)
    for k in range(pairs):
        ax = int(rng.integers(3)); u, v = [a for a in range(3) if a != ax]
        p = rng.uniform(-1.0, 1.0, 3); w, h = rng.uniform(0.02, 0.3, 2)
        c = np.tile(p, (4, 1)); c[1, u] += w; c[2, u] += w; c[2, v] += h; c[3, v] += h
        out[k, 0] = c[[0, 1, 2]]; out[k, 1] = c[[0, 2, 3]]
    return out.reshape(-1, 9)


def _case(name):
    """-> (SceneDesc, abc, material words)"""
    from phosphorus_mk2_amd import scenes
    rng = np.random.default_rng(sum(map(ord, name)))
    if name.startswith("n"):            # boundary sizes: a full root and one over, the 64-leaf wave and the 256-leaf workgroup of k_collapse_dp, ...
        abc = cloud(rng, int(name[1:]))
    elif name == "quads":               # equal keys in pairs, as in every lamp and wall
        abc = _quads(rng, 500)
    elif name.startswith("copies"):     # all keys equal, zero centroid extent: the tree is defined by index bits alone
        abc = np.tile(cloud(rng, 1), (int(name[6:]), 1))
    elif name == "cluster_outlier":     # the whole cluster shares its position bits
        abc = np.concatenate([cloud(rng, 1000, 5e-4, (0.3, 0.2, -2.0), 5e-4), cloud(rng, 1, 0.5, (1.0e4, 0.0, 0.0), 0.0)])
    elif name == "flat":                # one axis of zero extent: u = 0 there, boxes of thickness 2 delta
        abc = cloud(rng, 600, 0.05).reshape(-1, 3, 3); abc[:, :, 1] = 0.0; abc = abc.reshape(-1, 9)
    elif name == "line":                # zero-area triangles with all vertices on one line
        t = rng.uniform(-1.0, 1.0, (300, 1)) + rng.uniform(-0.01, 0.01, (300, 3))
        abc = (np.array([0.1, -0.2, -2.5]) + t[:, :, None] * np.array([1.0, 2.0, 3.0])).astype(np.float32).reshape(-1, 9)
    elif name == "mixed":               # the size bits of the key decide the top of the tree
        abc = mixed_sizes(rng, 1500, 10)
    else:
        sc = {"soup2000": lambda: scenes.soup(2000, width=16, height=16), "showroom2000": lambda: scenes.showroom(2000, width=16, height=16),
              "stress": lambda: scenes.stress(width=16, height=16)}[name]()
        return sc, tri_abc(sc), scene_materials(sc)
    abc = np.ascontiguousarray(abc, np.float32)
    sc, mat = scene_of(abc)
    assert np.array_equal(tri_abc(sc), abc)
    return sc, abc, mat


def _build(dev, sc):
    dev.preprocess(sc)
    pool, glo, gcell = dev.bvh_pool()
    return M.walk_pool(pool, glo, gcell), dev.stats()


CASES = ["n2", "n3", "n8", "n9", "n63", "n64", "n65", "n255", "n256", "n257", "n1025", "n2049", "quads", "copies2", "copies50", "copies257",
         "cluster_outlier", "flat", "line", "mixed", "soup2000", "showroom2000", "stress"]


@pytest.mark.parametrize("name", CASES)
def test_device_tree_is_the_model_tree(dev, name):
    sc, abc, material = _case(name)
    n = len(abc)
    assert n >= 2
    keys = M.emc_keys(abc)
    if name == "quads": assert (keys[0::2] == keys[1::2]).all()
    if name.startswith("copies"): assert len(np.unique(keys)) == 1
    W, st = _build(dev, sc)
    assert st["bvh_built_on_device"] == 1
    counts = (st["bvh_nodes"], st["triangles"], st["bvh_depth"])
    boxes = M.leaf_boxes(abc)
    check_partition_and_records(W, abc, material, counts)                      # a
    assert st["bvh_bytes"] == 64 * len(W.pool)
    check_layout(W)                                                            # b
    cb = M.child_boxes(W, boxes.ilo, boxes.ihi)
    check_origin_and_scale(W, cb)                                              # c
    check_stored_boxes(W, cb, counts)                                          # d
    T = M.radix_tree(keys, boxes.ilo, boxes.ihi)
    structure = check_radix_structure(W, T, DP_LEVELS)                         # e
    check_slots(W, T, structure)                                               # f
    cost = st["bvh_cost_model"]
    model, chain = M.tree_cost(W, boxes, CN, CT, levels=DP_LEVELS)
    check_cost(name, cost, model, chain, 1, "g")                               # g
    sub, chains = M.collapse_optimum(T, levels=DP_LEVELS, cn=CN, ct=CT)
    check_cost(name, cost, float(sub[0]), int(chains[0]), 2, "h")              # h


def _canonical(W):
    """a digest of the tree that does not depend on where the builder's waves put the elements: per nodelet its first three words (origin,
    valid, exponents, imask), its 48 box bytes and the digests of its children in slot order; per triangle its record"""
    digest = [None] * len(W.node)
    for k in range(len(W.node) - 1, -1, -1):
        h = hashlib.sha1(W.pool[W.node[k], 0:3].tobytes() + W.q[k].tobytes())
        for s in range(8):
            if W.vbit[k, s]:
                h.update(digest[W.child_row[k, s]] if W.ibit[k, s] else W.pool[W.child[k, s]].tobytes())
        digest[k] = h.digest()
    return digest[0], len(W.node), W.depth, W.level.tolist()


def test_device_tree_does_not_depend_on_the_build(xpu, dev):
    """the mixed-size case built twice on one device and once on a second one: the same tree up to the order in which waves were handed pool
    elements (the walks are compared, not the bytes)"""
    sc, abc, _ = _case("mixed")
    first, st1 = _build(dev, sc)
    again, st2 = _build(dev, sc)
    other = xpu.HipDevice.make(xpu.Options(samples_per_pixel=1, paths_per_sample=1, bvh_builder="device"))
    try:
        third, st3 = _build(other, sc)
    finally:
        other.close()
    assert _canonical(first) == _canonical(again) == _canonical(third)
    assert st1["bvh_cost_model"] == st2["bvh_cost_model"] == st3["bvh_cost_model"]
