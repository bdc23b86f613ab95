"""The model of the BVH builders' stages (tests/bvh_model.py), rehearsed on the CPU: the host builder's finished trees (default mode: binned
SAH + the optimal collapse) pass the finished-tree checks the device trees get in tests/test_gpu_bvh_builder.py, the host library's
emulation of the device's binary tree (PHX_HOST_LBVH=1: plain Morton keys, cuts within 7 binary levels) agrees with radix_tree +
collapse_optimum, and collapse_optimum agrees with a brute-force enumeration of every cut.

The checks, by the letters the GPU tests use:
  a  partition and records   every primitive in exactly one triangle record, v0 e0 e1 = a, b - a, c - a bit for bit, the material word,
                             every pool element referenced once, the counts
  b  layout                  imask within valid, empty slots inverted, a level's elements in front of the next level's
  c  origin and scale        the decoded origin at or below the node's fp32 box and less than a cell below it; the least exponent
  d  stored boxes            contain the child's fp32 box, and lie within (1 + 1e-3) grid units of it
  e  radix structure         every child is a node of the model's radix tree within the DP's depth; children partition their parent
  f  slots                   every child sits in the slot the greedy of k_collapse gives on the model's boxes
  g  objective               the reported cost is tree_cost of the finished tree, within chain * 2^-24 relative
  h  optimality              the reported cost is collapse_optimum's root value, within 2 * chain * 2^-24 relative

Largest observed |difference| / bound on the host (g, default mode: cornell 0.07, soup 17 0.02, soup 3000 0.004, stress 0.004, showroom 0.004;
g and h of the emulation: below 0.03)."""
import ctypes as C
import itertools

import numpy as np
import pytest

import bvh_model as M
from conftest import bits_equal, tri_abc

CN, CT = 1.6, 1.0  # the collapse's costs of a node visit and a triangle test (bvh_gpu.hip, bvh_build.cpp)


# ---- inputs --------------------------------------------------------------------------------------------------------------------

def cloud(rng, n, size=0.1, centre=(0.0, 0.0, -2.5), spread=1.0):
    """n random triangles: centres uniform in a cube of half-width `spread`, vertices within `size` of their centre -> (n, 9) float32"""
    c = rng.uniform(-spread, spread, (n, 1, 3)) + np.asarray(centre)
    return np.ascontiguousarray((c + rng.uniform(-size, size, (n, 3, 3))).astype(np.float32).reshape(n, 9))


def mixed_sizes(rng, small, large):
    """`small` triangles of size 0.01 among `large` of size 1, shuffled"""
    abc = np.concatenate([cloud(rng, small, 0.01), cloud(rng, large, 1.0)])
    return np.ascontiguousarray(abc[rng.permutation(len(abc))])


# ---- the finished-tree checks (either builder) -------------------------------------------------------------------------------

def check_partition_and_records(W, abc, material, counts=None):
    """item a.  counts: (nodelets, triangles, depth) as the builder reports them"""
    n = len(abc)
    assert len(W.tri_prim) == n and np.array_equal(np.sort(W.tri_prim), np.arange(n)), "a: the triangle records are not a permutation of the primitives"
    t = np.asarray(abc, np.float32).reshape(n, 3, 3)[W.tri_prim]
    want = np.concatenate([t[:, 0], (t[:, 1] - t[:, 0]).astype(np.float32), (t[:, 2] - t[:, 0]).astype(np.float32)], 1)
    assert bits_equal(W.pool[W.tri_elem, 0:9].view(np.float32), want), "a: v0, e0, e1 differ from a, b - a, c - a"
    assert np.array_equal(W.tri_material, np.asarray(material, np.uint32)[W.tri_prim]), "a: material word"
    assert not W.pool[W.tri_elem, 11:16].any(), "a: the spare words of a triangle record are not zero"
    assert (W.refs == 1).all(), f"a: pool elements referenced {np.unique(W.refs).tolist()} times"
    assert not (W.is_node & W.is_tri).any() and len(W.pool) == len(W.node) + n, "a: len(pool) != nodelets + triangles"
    if counts is not None:
        assert (len(W.node), n, W.depth) == tuple(int(x) for x in counts), f"a: walked {(len(W.node), n, W.depth)}, reported {tuple(counts)}"


def check_layout(W):
    """item b"""
    assert not (W.imask & ~W.valid).any(), "b: imask outside valid"
    assert (W.vbit.sum(1) >= 1).all(), "b: a nodelet without children"
    used = np.repeat(W.vbit[:, None, :], 3, 1)
    assert (W.q[:, 0:3, :][~used] == 255).all() and (W.q[:, 3:6, :][~used] == 0).all(), "b: an empty slot is not the inverted box"
    for L in range(int(W.elem_level.max())):
        a, b = np.nonzero(W.elem_level == L)[0], np.nonzero(W.elem_level == L + 1)[0]
        assert a.max() < b.min(), f"b: an element of level {L + 1} lies in front of one of level {L}"


def _ulp32(*xs):
    return np.spacing(np.maximum.reduce([np.abs(np.asarray(x, np.float64)) for x in xs]).astype(np.float32)).astype(np.float64)


def check_origin_and_scale(W, cb):
    """item c.  cb = M.child_boxes(W, ...): the node's fp32 box is the union of the inflated boxes of its triangles"""
    _, _, nlo, nhi = cb
    nlo = nlo.astype(np.float64); nhi = nhi.astype(np.float64)
    cell = W.gcell.astype(np.float64)[None, :]
    assert (W.org <= nlo).all(), "c: a decoded origin above its node's box"
    free = (W.gi > 0) & (W.gi < M.GRID_MAX)
    # the origin is fma(i, cell, lo) ROUNDED to fp32, so "the largest index at or below" holds up to one rounding of the operands
    assert ((nlo - W.org) < cell + _ulp32(W.org, nlo))[free].all(), "c: an origin a full grid cell below its node's box"
    ext = (nhi - W.org) * 1.00001
    pos = ext > 0
    assert (W.e[~pos] == -126).all(), "c: exponent of a flat extent"
    assert (np.ldexp(255.0, W.e) >= ext)[pos & (W.e < 127)].all(), "c: 255 grid units do not reach the node's upper bound"
    assert (np.ldexp(255.0, W.e - 1) < ext)[pos & (W.e > -126)].all(), "c: an exponent larger than needed"


def check_stored_boxes(W, cb, counts):
    """item d"""
    assert M.check_containment(W.pool, W.glo, W.gcell) == tuple(int(x) for x in counts)
    clo, chi, _, _ = cb
    v = np.repeat(W.vbit[:, None, :], 3, 1)                                        # [n, axis, slot]
    clo = np.transpose(clo, (0, 2, 1)).astype(np.float64); chi = np.transpose(chi, (0, 2, 1)).astype(np.float64)
    assert (W.lo <= clo)[v].all() and (W.hi >= chi)[v].all(), "d: a stored box does not contain its child's fp32 box"
    unit = (1.0 + 1e-3) * W.scale[:, :, None]; org = np.broadcast_to(W.org[:, :, None], clo.shape)
    qlo, qhi = W.q[:, 0:3, :], W.q[:, 3:6, :]
    clo = np.where(v, clo, 0.0); chi = np.where(v, chi, 0.0)  # (empty slots hold +-inf)
    ok_lo = (clo - W.lo) <= unit + _ulp32(clo, org)  # plus one fp32 rounding of the operands
    ok_hi = (W.hi - chi) <= unit + _ulp32(chi, org)
    assert ok_lo[v & (qlo > 0) & (qlo < 255)].all(), "d: a lower bound more than 1.001 grid units below the child's box"
    assert ok_hi[v & (qhi > 0) & (qhi < 255)].all(), "d: an upper bound more than 1.001 grid units above the child's box"


def check_radix_structure(W, T, max_levels):
    """items e / j -> per nodelet row (its radix node, [(slot, radix node of the child)] by range start)"""
    pos = np.empty(T.n, np.int64); pos[T.order] = np.arange(T.n)
    below = M.prims_below(W)
    mine = {0: 0}
    out = [None] * len(W.node)
    for k in range(len(W.node)):
        m = mine[k]
        kids = []
        for s in range(8):
            if below[k][s] is None: continue
            p = pos[below[k][s]]
            f, l = int(p.min()), int(p.max())
            assert l - f + 1 == len(p), f"e: nodelet {k} slot {s}: the primitives below it are not a range of the sorted order"
            assert (f, l) in T.by_range, f"e: nodelet {k} slot {s}: positions {f}..{l} are not a node of the radix tree"
            v = T.by_range[(f, l)]
            assert 1 <= T.depth[v] - T.depth[m] <= max_levels, f"e: nodelet {k} slot {s}: {T.depth[v] - T.depth[m]} binary levels below its parent"
            assert T.is_leaf(v) == (not W.ibit[k, s])
            if W.ibit[k, s]: mine[int(W.child_row[k, s])] = v
            kids.append((f, l, s, v))
        kids.sort()
        assert 2 <= len(kids) <= 8, f"e: nodelet {k} has {len(kids)} children"
        assert kids[0][0] == T.first[m] and kids[-1][1] == T.last[m] and all(a[1] + 1 == b[0] for a, b in zip(kids, kids[1:])), \
            f"e: the children of nodelet {k} do not partition its range"
        out[k] = (m, [(s, v) for _, _, s, v in kids])
    return out


def check_slots(W, T, structure):
    """item f"""
    for k, (m, kids) in enumerate(structure):
        vs = [v for _, v in kids]
        want = M.slot_order(T.lo[vs], T.hi[vs], T.lo[m], T.hi[m])
        assert [s for s, _ in kids] == want, f"f: nodelet {k}: children in slots {[s for s, _ in kids]}, the greedy gives {want}"


def check_cost(label, reported, model, chain, factor, item):
    """items g (factor 1) and h (factor 2): |reported - model| <= factor * chain * 2^-24 * model; prints the figures"""
    bound = factor * chain * M.EPS32
    diff = abs(reported - model) / model
    print(f"[bvh-cost] {label} {item}: reported {reported:.9g} model {model:.9g} rel diff {diff:.3g} bound {bound:.3g} ratio {diff / bound:.3g}")
    assert diff <= bound, f"{item}: {label}: reported {reported!r}, model {model!r}: {diff:.3g} relative, bound {bound:.3g} ({chain} roundings)"
    return diff / bound


# ---- the host library ----------------------------------------------------------------------------------------------------------

def host_tree(lib, abc):
    """build with the host library -> (Walk, (nodelets, triangles, depth), Bvh8::cost)"""
    from phosphorus_mk2_amd import abi
    lib.hb8_copy_pool.restype = C.c_uint64
    lib.hb8_copy_pool.argtypes = [C.c_void_p, abi.u32p, C.c_uint64, abi.f32p, abi.f32p]
    abc = np.ascontiguousarray(abc, np.float32)
    h = lib.hb8_build(abc.ctypes.data_as(abi.f32p), len(abc), 4)
    try:
        info = (C.c_uint64 * 3)(); lib.hb8_info(h, info)
        grid = np.zeros(6, np.float32); cost = np.zeros(1, np.float32)
        n_el = lib.hb8_copy_pool(h, None, 0, grid.ctypes.data_as(abi.f32p), cost.ctypes.data_as(abi.f32p))
        pool = np.zeros((n_el, 16), np.uint32)
        assert lib.hb8_copy_pool(h, pool.ctypes.data_as(abi.u32p), n_el, grid.ctypes.data_as(abi.f32p), cost.ctypes.data_as(abi.f32p)) == n_el
    finally:
        lib.hb8_free(h)
    return M.walk_pool(pool, grid[:3], grid[3:]), tuple(info), float(cost[0])


def _scene(name):
    from phosphorus_mk2_amd import scenes
    return {"cornell": lambda: scenes.cornell(16, 16), "soup17": lambda: scenes.soup(17, width=16, height=16),
            "soup3000": lambda: scenes.soup(3000, width=16, height=16), "stress": scenes.stress,
            "showroom3000": lambda: scenes.showroom(3000, width=16, height=16)}[name]()


@pytest.mark.parametrize("name", ["cornell", "soup17", "soup3000", "stress", "showroom3000"])
def test_host_builder_finished_tree(host_bvh8, name):
    """the host builder in its default mode: items a, b, c, d, and g on Bvh8::cost (a cut of <= 8 lies within 7 binary levels)"""
    abc = tri_abc(_scene(name))
    W, counts, cost = host_tree(host_bvh8, abc)
    boxes = M.leaf_boxes(abc)
    check_partition_and_records(W, abc, np.zeros(len(abc), np.uint32), counts)
    check_layout(W)
    cb = M.child_boxes(W, boxes.ilo, boxes.ihi)
    check_origin_and_scale(W, cb)
    check_stored_boxes(W, cb, counts)
    model, chain = M.tree_cost(W, boxes, CN, CT, levels=7)
    check_cost(name, cost, model, chain, 1, "g")


REHEARSAL = {"n2": 2, "n3": 3, "n9": 9, "n65": 65, "n257": 257, "n300": 300, "mixed": (280, 8)}


@pytest.mark.parametrize("name", list(REHEARSAL))
def test_host_lbvh_emulation_matches_the_model(host_bvh8, monkeypatch, name):
    """PHX_HOST_LBVH=1: the host library builds the device's kind of binary tree (plain Morton keys, ranges split at the highest differing bit)
    and collapses it with cuts within 7 levels.  On distinct keys radix_tree + collapse_optimum(levels=7) must describe that tree: items e (j:
    every child is a radix node within the emulation's depth), f, g, h."""
    monkeypatch.setenv("PHX_HOST_LBVH", "1")
    for k in ("PHX_DP_HEAP", "PHX_COLLAPSE", "PHX_WIDTH", "PHX_CNODE"):
        monkeypatch.delenv(k, raising=False)
    rng = np.random.default_rng(100 + len(name))
    spec = REHEARSAL[name]
    abc = mixed_sizes(rng, *spec) if isinstance(spec, tuple) else cloud(rng, spec)
    keys = M.emc_keys(abc, plain=True)
    assert len(np.unique(keys)) == len(keys), "the rehearsal needs distinct keys (the emulation breaks ties by the median)"
    boxes = M.leaf_boxes(abc)
    T = M.radix_tree(keys, boxes.ilo, boxes.ihi, median_ties=True)
    W, counts, cost = host_tree(host_bvh8, abc)
    check_partition_and_records(W, abc, np.zeros(len(abc), np.uint32), counts)
    check_layout(W)
    cb = M.child_boxes(W, boxes.ilo, boxes.ihi)
    check_origin_and_scale(W, cb)
    check_stored_boxes(W, cb, counts)
    structure = check_radix_structure(W, T, 7)
    check_slots(W, T, structure)
    model, chain = M.tree_cost(W, boxes, CN, CT, levels=7)
    check_cost(name, cost, model, chain, 1, "g")
    sub, chains = M.collapse_optimum(T, levels=7, cn=CN, ct=CT)
    check_cost(name, cost, float(sub[0]), int(chains[0]), 2, "h")


# ---- the model against itself ----------------------------------------------------------------------------------------------------

def _cuts(T, v, lev, levels):
    yield (v,)
    if not T.is_leaf(v) and lev < levels:
        for a, b in itertools.product(list(_cuts(T, T.left[v], lev + 1, levels)), list(_cuts(T, T.right[v], lev + 1, levels))):
            yield a + b


def _brute_sub(T, levels, slots, cn, ct):
    sub = np.full(len(T.first), np.nan)
    for m in range(len(T.first) - 1, -1, -1):
        if T.is_leaf(m): continue
        g2 = M.grid2(T.lo[m], T.hi[m])
        best = np.inf
        for a, b in itertools.product(list(_cuts(T, T.left[m], 1, levels)), list(_cuts(T, T.right[m], 1, levels))):
            K = a + b
            if len(K) > slots: continue
            best = min(best, sum(M.area_q(T.lo[c], T.hi[c], g2) * (ct if T.is_leaf(c) else cn) + (0.0 if T.is_leaf(c) else sub[c]) for c in K))
        sub[m] = best
    return sub


@pytest.mark.parametrize("n,levels,slots", [(2, 4, 8), (3, 4, 8), (6, 1, 8), (9, 2, 8), (10, 4, 8), (10, 7, 8), (10, 4, 3), (10, 3, 4)])
def test_collapse_optimum_equals_brute_force(n, levels, slots):
    """every cut of at most `slots` elements within `levels` binary levels, enumerated: the programme's sub() is their minimum at every node"""
    rng = np.random.default_rng(n * 100 + levels * 10 + slots)
    abc = mixed_sizes(rng, n - n // 3, n // 3) if n > 3 else cloud(rng, n)
    boxes = M.leaf_boxes(abc)
    T = M.radix_tree(M.emc_keys(abc), boxes.ilo, boxes.ihi)
    sub, chain = M.collapse_optimum(T, levels=levels, slots=slots, cn=CN, ct=CT)
    want = _brute_sub(T, levels, slots, CN, CT)
    inner = ~np.isnan(want)
    assert inner.sum() == n - 1 and np.array_equal(np.isnan(sub), ~inner)
    assert np.allclose(sub[inner], want[inner], rtol=1e-13, atol=0.0)
    assert (chain[inner] >= M.AREA_ROUNDINGS + 1).all()


def test_model_stages_on_known_inputs():
    """small known answers: fma32 against exact rational arithmetic, the key layout, the index tie-break, the slot greedy"""
    from fractions import Fraction
    rng = np.random.default_rng(5)
    i = rng.integers(0, M.GRID_MAX + 1, 4000); cell = np.float32(rng.uniform(1e-7, 1e-3)); lo = np.float32(-rng.uniform(0.1, 1e4))
    got = M.fma32(i, cell, lo)
    for k in range(0, 4000, 7):
        x = Fraction(int(i[k])) * Fraction(float(cell)) + Fraction(float(lo))
        c = np.float32(float(x))
        cands = [c, np.nextafter(c, np.float32(-np.inf)), np.nextafter(c, np.float32(np.inf))]
        d = [abs(Fraction(float(y)) - x) for y in cands]
        assert Fraction(float(got[k])) in [Fraction(float(y)) for y, e in zip(cands, d) if e == min(d)]
    # keys: two triangles at opposite corners, one of them as large as the scene
    abc = np.array([[0, 0, 0, 0.25, 0, 0, 0, 0.25, 0], [1, 1, 1, 1, 1, 1, 1, 1, 1], [0, 0, 0, 1, 1, 1, 0, 1, 0]], np.float32)
    k = M.emc_keys(abc)
    B = M.leaf_boxes(abc)
    assert B.delta == np.float32(2.0 * 2.0 ** -18) and bits_equal(B.ilo[1], np.full(3, np.float32(1) - B.delta, np.float32))
    assert int(k[1]) == int("1110" * 15, 2)                       # centroid at the far corner: q = 2^21 - 1; a point has size 0
    assert int(k[2]) & int("0001" * 15, 2) == int("0001" * 15, 2)   # the scene-sized triangle: size 32767, every size bit set
    assert int(k[0]) >> 56 == 0                                   # near the origin corner: no leading position bit
    assert int(M.emc_keys(abc, plain=True)[1]) == (1 << 63) - 1
    # equal keys: the tree is defined by the bits of the sorted position alone
    same = np.tile(abc[:1], (5, 1))
    Bs = M.leaf_boxes(same)
    T = M.radix_tree(M.emc_keys(same), Bs.ilo, Bs.ihi)
    assert T.order.tolist() == [0, 1, 2, 3, 4] and (0, 3) in T.by_range and (4, 4) in T.by_range and (0, 1) in T.by_range and (2, 3) in T.by_range
    Tm = M.radix_tree(M.emc_keys(same), Bs.ilo, Bs.ihi, median_ties=True)
    assert (0, 1) in Tm.by_range and (2, 4) in Tm.by_range
    # slots: a child in the (+, +, +) corner is cheapest in slot 7 (all signs flipped), one in the (-, -, -) corner in slot 0
    lo = np.array([[0.5, 0.5, 0.5], [-1, -1, -1]], np.float32); hi = np.array([[1, 1, 1], [-0.5, -0.5, -0.5]], np.float32)
    assert M.slot_order(lo, hi, [-1, -1, -1], [1, 1, 1]) == [7, 0]
    assert M.slot_order(lo[:1].repeat(3, 0), hi[:1].repeat(3, 0), [-1, -1, -1], [1, 1, 1])[0] == 7  # ties: the first child, the first slot
