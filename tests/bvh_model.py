"""A plain model of the device BVH builder (csrc/bvh_gpu.hip) and of the 8-wide pool it writes (csrc/bvh8.h), for tests: numpy and
Python integers, no GPU, no ctypes.

Restated from the comments and code of bvh_gpu.hip and bvh8.h, stage by stage; it shares no code with either builder:

  walk_pool        decodes a finished pool (either builder's): nodelets level by level, triangle records, who references whom
  leaf_boxes       k_prim_bounds + k_leaf_boxes in float32: triangle boxes, geometry bounds, tri_box_inflation, the grown boxes
  emc_keys         k_morton in float32: the extended Morton key "xyzs" x 15 (plain=True: the 63-bit keys of the host's LBVH emulation)
  radix_tree       the sort by (key, primitive) + k_radix_tree + k_fit: Karras' tree over key << 32 | sorted position
  collapse_optimum the sub(m) programme stated above k_collapse_dp, in float64
  tree_cost        the same objective evaluated on a finished 8-wide tree alone (needs no binary tree: either builder's)
  slot_order       k_collapse's greedy octant-order slot assignment in float32

The library is compiled with -ffp-contract=off -fno-fast-math, so the float32 stages (boxes, keys, k_fit's min / max, the slot
greedy's dot products) are reproduced bit for bit by numpy.float32 arithmetic: one rounding per operation, in the code's order.
The stages above them are integer logic, or floating point that the float64 model bounds (`chain`: the number of fp32 roundings
on the longest path into a sum; all terms are positive, so a sum's relative error is at most its worst term's plus one rounding).
"""
import numpy as np

F32 = np.float32
GRID_MAX = (1 << 18) - 1
TWO_M18 = F32(3.814697265625e-6)  # 2^-18 of tri_box_inflation
EPS32 = 2.0 ** -24                # one fp32 rounding, relative


# ---- the pool ----------------------------------------------------------------------------------------------------------------

def fma32(i, cell, lo):
    """fmaf((float)i, cell, lo) exactly: i < 2^18 times a 24-bit cell is exact in float64; the sum's float64 rounding error (TwoSum)
    decides the one case a double rounding could get wrong, a float64 sum that lies exactly between two floats"""
    p = np.asarray(i, np.float64) * np.asarray(cell, np.float32).astype(np.float64)
    l = np.broadcast_to(np.asarray(lo, np.float32).astype(np.float64), p.shape)
    t = p + l
    bb = t - p
    r = (p - (t - bb)) + (l - bb)
    f = t.astype(np.float32)
    d = t - f.astype(np.float64)
    other = np.nextafter(f, np.where(d > 0, F32(np.inf), F32(-np.inf)).astype(np.float32))
    mid = 0.5 * (f.astype(np.float64) + other.astype(np.float64))
    fix = (d != 0) & (t == mid) & (r != 0) & ((r > 0) == (d > 0))
    return np.where(fix, other, f).astype(np.float32)


def decode_nodes(pool, idx, glo, gcell):
    """the nodelets pool[idx] (bvh8.h: Node8) -> dict of arrays, one row per nodelet: grid indices `gi`, decoded origin `org` (the
    float fma(i, cell, lo), widened), `valid`, `imask`, `base`, unbiased exponents `e`, `scale` = 2^e, the 6 x 8 bytes `q` (rows lox loy
    loz hix hiy hiz, columns slots), decoded child boxes `lo`, `hi` [n, axis, slot] in float64, `vbit`, `ibit` [n, slot] and the pool
    index `child` [n, slot] of every slot's element (meaningful where vbit: base + rank among the valid slots)"""
    u8 = pool.view(np.uint8).reshape(-1, 64)
    slot = np.arange(8)
    w = pool[idx].astype(np.uint64)
    ix = w[:, 0] & 0x3ffff; iy = ((w[:, 0] >> 18) | (w[:, 1] << 14)) & 0x3ffff; iz = (w[:, 1] >> 4) & 0x3ffff
    valid = ((w[:, 1] >> 22) & 0xff).astype(np.uint32); imask = (w[:, 2] >> 24).astype(np.uint32); base = w[:, 3].astype(np.int64)
    gi = np.stack([ix, iy, iz], 1).astype(np.int64)
    org = fma32(gi, gcell, glo).astype(np.float64)
    e = np.stack([w[:, 2] & 0xff, (w[:, 2] >> 8) & 0xff, (w[:, 2] >> 16) & 0xff], 1).astype(np.int64) - 127
    scale = np.ldexp(1.0, e)
    q = u8[idx][:, 16:].reshape(-1, 6, 8)
    qf = q.astype(np.float64)
    lo = org[:, :, None] + qf[:, 0:3, :] * scale[:, :, None]; hi = org[:, :, None] + qf[:, 3:6, :] * scale[:, :, None]
    vbit = ((valid[:, None] >> slot) & 1).astype(bool); ibit = ((imask[:, None] >> slot) & 1).astype(bool)
    child = base[:, None] + np.cumsum(vbit, 1) - vbit
    return dict(gi=gi, org=org, valid=valid, imask=imask, base=base, e=e, scale=scale, q=q, lo=lo, hi=hi, vbit=vbit, ibit=ibit, child=child)


class Walk:
    """walk_pool's result.  Per nodelet, breadth first (row k; the root is row 0): `node` (pool index), `level` (root 0), `parent` (row, -1),
    `parent_slot`, and everything decode_nodes gives; `child_row` [n, slot]: the row of an inner child, else -1.  Per pool element:
    `refs` (how many slots point at it; the root counts as referenced once), `elem_level` (-1: unreached), `is_node`, `is_tri`.
    `tri_elem`, `tri_prim`, `tri_material`: the triangle records reached, in walk order; `depth`: levels of nodelets."""


def walk_pool(pool, glo, gcell):
    pool = np.ascontiguousarray(pool, np.uint32).reshape(-1, 16)
    glo = np.asarray(glo, np.float32); gcell = np.asarray(gcell, np.float32)
    n_el = len(pool)
    W = Walk()
    W.pool = pool; W.glo = glo; W.gcell = gcell
    W.refs = np.zeros(n_el, np.int64); W.refs[0] = 1
    W.elem_level = np.full(n_el, -1, np.int64); W.elem_level[0] = 0
    W.is_node = np.zeros(n_el, bool); W.is_tri = np.zeros(n_el, bool)
    parts, level, parent, pslot, L, offset = [], np.array([0], np.int64), np.array([-1], np.int64), np.array([-1], np.int64), 0, 0
    while len(level):
        d = decode_nodes(pool, level, glo, gcell)
        W.is_node[level] = True
        cn, cs = np.nonzero(d["vbit"])
        ch = d["child"][cn, cs]
        if len(ch) and (ch.min() < 0 or ch.max() >= n_el):
            raise ValueError(f"level {L}: a child index lies outside the pool of {n_el} elements")
        np.add.at(W.refs, ch, 1)
        W.elem_level[ch] = L + 1
        tn, ts = np.nonzero(d["vbit"] & ~d["ibit"])
        W.is_tri[d["child"][tn, ts]] = True
        d.update(node=level, level=np.full(len(level), L, np.int64), parent=parent, parent_slot=pslot)
        parts.append(d)
        inn, ins = np.nonzero(d["vbit"] & d["ibit"])
        parent, pslot = offset + inn, ins
        offset += len(level); level = d["child"][inn, ins]; L += 1
        if offset + len(level) > n_el:
            raise ValueError("more nodelets than pool elements: the tree has a cycle or a shared child")
    for k in parts[0]:
        setattr(W, k, np.concatenate([p[k] for p in parts]))
    W.child = np.where(W.vbit, W.child, -1)
    row_of = np.full(n_el, -1, np.int64); row_of[W.node] = np.arange(len(W.node))
    W.child_row = np.where(W.vbit & W.ibit, row_of[np.where(W.vbit, W.child, 0)], -1)
    tn, ts = np.nonzero(W.vbit & ~W.ibit)
    W.tri_elem = W.child[tn, ts]
    W.tri_prim = pool[W.tri_elem, 9].astype(np.int64); W.tri_material = pool[W.tri_elem, 10]
    W.depth = L
    return W


def prims_below(W):
    """-> list per nodelet row of 8 entries: the primitives below each slot (int64 array; None for an empty slot)"""
    prim_of = np.full(len(W.pool), -1, np.int64); prim_of[W.tri_elem] = W.tri_prim
    out = [None] * len(W.node)
    for k in range(len(W.node) - 1, -1, -1):
        row = []
        for s in range(8):
            if not W.vbit[k, s]: row.append(None)
            elif W.ibit[k, s]: row.append(np.concatenate([x for x in out[W.child_row[k, s]] if x is not None]))
            else: row.append(prim_of[W.child[k, s]:W.child[k, s] + 1])
        out[k] = row
    return out


def child_boxes(W, ilo, ihi):
    """fp32 box of every slot's subtree, the union of the inflated boxes of its triangles (min / max are exact, so this is what k_fit or the
    host's grow() holds for that child whatever the binary tree was) -> (clo, chi [n, slot, 3] with +-inf in empty slots, nlo, nhi [n, 3])"""
    n = len(W.node)
    clo = np.full((n, 8, 3), np.inf, np.float32); chi = np.full((n, 8, 3), -np.inf, np.float32)
    nlo = np.full((n, 3), np.inf, np.float32); nhi = np.full((n, 3), -np.inf, np.float32)
    prim_of = np.full(len(W.pool), -1, np.int64); prim_of[W.tri_elem] = W.tri_prim
    for k in range(n - 1, -1, -1):
        for s in np.nonzero(W.vbit[k])[0]:
            if W.ibit[k, s]: clo[k, s], chi[k, s] = nlo[W.child_row[k, s]], nhi[W.child_row[k, s]]
            else: p = prim_of[W.child[k, s]]; clo[k, s], chi[k, s] = ilo[p], ihi[p]
        nlo[k] = clo[k].min(0); nhi[k] = chi[k].max(0)
    return clo, chi, nlo, nhi


def check_containment(pool, glo, gcell):
    """walk the 8-wide tree breadth first (numpy, a level at a time), then bottom-up: the box a nodelet stores for a child must contain
    every TRIANGLE that hangs below that child (a child's own stored boxes live on the child's grid and may stick out of the parent's
    box by a grid unit of the child: the invariant is about the geometry).  -> (nodelets, triangles, deepest level)"""
    n_el = len(pool)
    true_lo = np.full((n_el, 3), np.inf); true_hi = np.full((n_el, 3), -np.inf)
    levels = []
    level = np.array([0], np.int64)
    nodes = tris = 0
    while len(level):
        d = decode_nodes(pool, level, glo, gcell)
        vbit, ibit, child, lo, hi = d["vbit"], d["ibit"], d["child"], d["lo"], d["hi"]
        assert not (ibit & ~vbit).any()
        assert child[vbit].max() < n_el
        tn, ts = np.nonzero(vbit & ~ibit)
        if len(tn):  # triangle records: a, a + e0, a + e1 (the builder's fp32 v0, e0, e1: b and c up to a rounding)
            ti = child[tn, ts]
            rec = pool[ti].view(np.float32).astype(np.float64)
            a3 = rec[:, 0:3]; b3 = a3 + rec[:, 3:6]; c3 = a3 + rec[:, 6:9]
            true_lo[ti] = np.minimum(np.minimum(a3, b3), c3); true_hi[ti] = np.maximum(np.maximum(a3, b3), c3)
            tris += len(tn)
        nodes += len(level)
        levels.append((level, child, vbit, lo, hi))
        cn, cs = np.nonzero(ibit)
        level = child[cn, cs]
    for level, child, vbit, lo, hi in reversed(levels):  # bottom-up: true bounds of every subtree, checked against the stored boxes
        cl = np.where(vbit[:, :, None], true_lo[np.where(vbit, child, 0)], np.inf); ch = np.where(vbit[:, :, None], true_hi[np.where(vbit, child, 0)], -np.inf)  # [n, slot, axis]
        assert np.isfinite(cl[vbit]).all() and np.isfinite(ch[vbit]).all()
        eps = 1e-5 * (1.0 + np.abs(cl) + np.abs(ch))
        slo = np.transpose(lo, (0, 2, 1)); shi = np.transpose(hi, (0, 2, 1))
        ok = (slo <= cl + eps) & (shi >= ch - eps)
        assert ok[vbit].all(), "geometry sticks out of the box its ancestor stores for it"
        true_lo[level] = cl.min(1); true_hi[level] = ch.max(1)
    return nodes, tris, len(levels)


# ---- boxes and keys, float32 ---------------------------------------------------------------------------------------------------

class LeafBoxes:
    """leaf_boxes' result: `lo`, `hi` [n, 3] the triangles' boxes; `glo`, `ghi` the geometry bounds; `delta`; `ilo`, `ihi` the boxes grown by delta"""


def leaf_boxes(abc):
    abc = np.ascontiguousarray(abc, np.float32).reshape(-1, 3, 3)
    B = LeafBoxes()
    B.lo = np.minimum(np.minimum(abc[:, 0], abc[:, 1]), abc[:, 2]); B.hi = np.maximum(np.maximum(abc[:, 0], abc[:, 1]), abc[:, 2])
    B.glo = B.lo.min(0); B.ghi = B.hi.max(0)
    ext = F32(0); mag = F32(0)
    for a in range(3):  # tri_box_inflation (bvh8.h), in its order
        ext = max(ext, F32(B.ghi[a] - B.glo[a]))
        mag = max(mag, max(abs(B.glo[a]), abs(B.ghi[a])))
    B.delta = F32(F32(ext + mag) * TWO_M18)
    B.ilo = (B.lo - B.delta).astype(np.float32); B.ihi = (B.hi + B.delta).astype(np.float32)
    return B


def _spread21(q):
    r = np.zeros(len(q), np.uint64)
    for b in range(21):
        r |= ((q >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b)
    return r


def emc_keys(abc, plain=False):
    """k_morton's key of every triangle (uint64 [n]): 15 groups "x y z s" from bit 20 - g of the quantised centroid and bit 14 - g of the
    size; plain=True: the 63-bit Morton code of the 21-bit centroid alone (PHX_EMC=0, and the host's PHX_HOST_LBVH emulation)"""
    B = leaf_boxes(abc)
    c = (F32(0.5) * (B.lo + B.hi)).astype(np.float32)  # the centroid of the box BEFORE inflation
    clo = c.min(0); chi = c.max(0)
    q = np.zeros((len(c), 3), np.uint64)
    d2 = np.zeros(len(c), np.float32); D2 = F32(0)
    for a in range(3):
        ext = F32(chi[a] - clo[a])
        if ext > 0: u = ((c[:, a] - clo[a]).astype(np.float32) / ext).astype(np.float32)
        else: u = np.zeros(len(c), np.float32)
        u = np.minimum(np.maximum(u, F32(0)), F32(1))
        q[:, a] = np.minimum((u * F32(2097152.0)).astype(np.float32), F32(2097151.0)).astype(np.uint64)
        e = (B.hi[:, a] - B.lo[:, a]).astype(np.float32); E = F32(B.ghi[a] - B.glo[a])
        d2 = (d2 + (e * e).astype(np.float32)).astype(np.float32); D2 = F32(D2 + F32(E * E))
    if plain:
        return (_spread21(q[:, 0]) << np.uint64(2)) | (_spread21(q[:, 1]) << np.uint64(1)) | _spread21(q[:, 2])
    rel = np.sqrt((d2 / D2).astype(np.float32)).astype(np.float32) if D2 > 0 else np.zeros(len(c), np.float32)
    sz = np.minimum((rel * F32(32768.0)).astype(np.float32), F32(32767.0)).astype(np.uint64)
    key = np.zeros(len(c), np.uint64)
    one = np.uint64(1)
    for g in range(15):
        bit = np.uint64(20 - g)
        grp = (((q[:, 0] >> bit) & one) << np.uint64(2)) | (((q[:, 1] >> bit) & one) << one) | ((q[:, 2] >> bit) & one)
        key = (key << np.uint64(3)) | grp
        key = (key << one) | ((sz >> np.uint64(14 - g)) & one)
    return key


# ---- the binary tree -----------------------------------------------------------------------------------------------------------

class Tree2:
    """radix_tree's result.  `order` [n]: the primitive at every sorted position; nodes are numbered parents before children, the root is 0:
    `first`, `last` (range of sorted positions, inclusive), `left`, `right` (-1 in a leaf), `parent`, `depth` (root 0), `lo`, `hi` (fp32
    boxes [nodes, 3]); `by_range`: {(first, last): node}"""
    def is_leaf(self, v):
        return self.left[v] < 0


def radix_tree(keys, ilo, ihi, median_ties=False):
    """Stable sort by (key, primitive), then Karras' tree over the augmented integers key << 32 | sorted position: every range splits at the
    highest differing bit of its first and last element (delta()'s 64 + clz(i ^ j) branch is that rule on the index bits).  Leaf boxes are
    (ilo, ihi)[order]; an inner node's is the fp32 min / max of its children's (k_fit).  median_ties=True: a range of equal keys splits at
    first + count / 2 instead, the host emulation's rule."""
    keys = np.asarray(keys, np.uint64)
    n = len(keys)
    T = Tree2()
    T.n = n
    T.order = np.lexsort((np.arange(n), keys))  # by key, ties by primitive index: what a stable radix sort of (key, index) pairs gives
    ks = [int(k) for k in keys[T.order]]
    aug = [(k << 32) | i for i, k in enumerate(ks)]
    first, last, left, right, parent, depth = [0], [n - 1], [-1], [-1], [-1], [0]
    todo = [0]
    while todo:
        v = todo.pop()
        f, l = first[v], last[v]
        if f == l: continue
        if median_ties and ks[f] == ks[l]:
            mid = f + (l - f + 1) // 2
        else:
            bit = (aug[f] ^ aug[l]).bit_length() - 1
            lo_, hi_ = f, l  # the first position whose bit is set (sorted: the bits above `bit` are shared, so the bit is monotone)
            while lo_ < hi_:
                m = (lo_ + hi_) // 2
                if (aug[m] >> bit) & 1: hi_ = m
                else: lo_ = m + 1
            mid = lo_
        for (cf, cl) in ((f, mid - 1), (mid, l)):
            first.append(cf); last.append(cl); left.append(-1); right.append(-1); parent.append(v); depth.append(depth[v] + 1)
        left[v] = len(first) - 2; right[v] = len(first) - 1
        todo += [right[v], left[v]]
    T.first, T.last, T.left, T.right, T.parent, T.depth = (np.array(x, np.int64) for x in (first, last, left, right, parent, depth))
    nn = len(first)
    T.lo = np.zeros((nn, 3), np.float32); T.hi = np.zeros((nn, 3), np.float32)
    for v in range(nn - 1, -1, -1):
        if left[v] < 0: T.lo[v] = ilo[T.order[first[v]]]; T.hi[v] = ihi[T.order[first[v]]]
        else: T.lo[v] = np.minimum(T.lo[left[v]], T.lo[right[v]]); T.hi[v] = np.maximum(T.hi[left[v]], T.hi[right[v]])
    T.by_range = {(first[v], last[v]): v for v in range(nn)}
    return T


# ---- the collapse ----------------------------------------------------------------------------------------------------------------

AREA_ROUNDINGS = 7  # fp32 roundings on the longest path into 2 (dx dy + dy dz + dz dx), dx = (hi - lo) + g2: 2 per extent, a product 2 + 2 + 1, two sums


def grid2(lo, hi):
    """two grid units per axis of an 8-wide node with the fp32 box (lo, hi): e = clamp(ceil(log2(ext * 1.00001 / 255))), 2 * 2^e.  (frexp
    gives ceil(log2 x) exactly: x = m 2^k with m in [0.5, 1) -> k, or k - 1 for m = 0.5)"""
    g = np.zeros(3)
    for a in range(3):
        ext = float(hi[a]) - float(lo[a])
        e = -126
        if ext > 0.0:
            m, k = np.frexp(ext * 1.00001 / 255.0)
            e = int(k) if m > 0.5 else int(k) - 1
        g[a] = 2.0 * 2.0 ** max(-126, min(127, e))
    return g


def area_q(lo, hi, g2):
    dx = float(hi[0]) - float(lo[0]) + g2[0]; dy = float(hi[1]) - float(lo[1]) + g2[1]; dz = float(hi[2]) - float(lo[2]) + g2[2]
    return 2.0 * (dx * dy + dy * dz + dz * dx)


def collapse_optimum(T, levels=4, slots=8, cn=1.6, ct=1.0):
    """sub(m) = min over cuts K of m's binary subtree, |K| <= slots, every element at most `levels` binary levels below m, of the sum over
    c in K of area(box(c) + 2 grid units of m) * (cn | ct) + (sub(c) if c is inner), in float64 -> (sub, chain), both per node (nan / 0 in
    leaves).  chain[m]: the fp32 roundings on the longest path into the device's sub[m] over EVERY cut the programme may look at — an
    element L levels below m passes L additions; an inner one adds the `sub` addition on top of max(its area, its sub)."""
    nn = len(T.first)
    sub = np.full(nn, np.nan); chain = np.zeros(nn, np.int64)
    L_, R_, lo_, hi_ = T.left.tolist(), T.right.tolist(), T.lo, T.hi
    for m in range(nn - 1, -1, -1):
        if L_[m] < 0: continue
        g2 = grid2(lo_[m], hi_[m])
        worst = [0]

        def best(v, lev):  # -> b[j], j = 1 .. slots - 1: cheapest way to hang v below m in at most j slots
            aq = area_q(lo_[v], hi_[v], g2)
            if L_[v] < 0:
                worst[0] = max(worst[0], AREA_ROUNDINGS + lev)
                return [aq * ct] * slots
            worst[0] = max(worst[0], max(AREA_ROUNDINGS + 1, int(chain[v])) + 1 + lev)
            one = aq * cn + sub[v]
            if lev >= levels: return [one] * slots
            a, b = best(L_[v], lev + 1), best(R_[v], lev + 1)
            r = [one] * slots
            for j in range(2, slots):
                r[j] = min(one, min(a[k] + b[j - k] for k in range(1, j)))
            return r
        a, b = best(L_[m], 1), best(R_[m], 1)
        sub[m] = min(a[k] + b[slots - k] for k in range(1, slots))
        chain[m] = worst[0]
    return sub, chain


def tree_cost(W, boxes, cn=1.6, ct=1.0, levels=7):
    """the collapse objective of a finished 8-wide tree, from the walk and the inflated triangle boxes alone, in float64 -> (cost of the
    root, chain).  chain as in collapse_optimum, along the tree as built: a child of a node with k children lies at most min(levels, k - 1)
    binary levels below it."""
    clo, chi, nlo, nhi = child_boxes(W, boxes.ilo, boxes.ihi)
    n = len(W.node)
    sub = np.zeros(n); chain = np.zeros(n, np.int64)
    for k in range(n - 1, -1, -1):
        g2 = grid2(nlo[k], nhi[k])
        used = np.nonzero(W.vbit[k])[0]
        adds = min(levels, len(used) - 1)
        for s in used:
            aq = area_q(clo[k, s], chi[k, s], g2)
            if W.ibit[k, s]:
                r = W.child_row[k, s]
                sub[k] += aq * cn + sub[r]; chain[k] = max(chain[k], max(AREA_ROUNDINGS + 1, chain[r]) + 1 + adds)
            else:
                sub[k] += aq * ct; chain[k] = max(chain[k], AREA_ROUNDINGS + adds)
    return float(sub[0]), int(chain[0])


def slot_order(clo, chi, nlo, nhi):
    """k_collapse's slot greedy in float32.  clo, chi [k, 3]: the children's boxes in cut order (by range start); nlo, nhi: the node's box.
    cen = 0.5 (lo + hi) of the child minus 0.5 (lo + hi) of the node; cost(child, slot) = (+-cen.x +- cen.y) +- cen.z with - where the
    slot's bit (4, 2, 1) is set; k times: the smallest cost over (child not placed, slot not used), strict <, child loop outside.
    -> the slot of every child"""
    clo = np.asarray(clo, np.float32); chi = np.asarray(chi, np.float32)
    half = F32(0.5)
    cen = ((half * (clo + chi)).astype(np.float32) - (half * (np.asarray(nlo, np.float32) + np.asarray(nhi, np.float32))).astype(np.float32)).astype(np.float32)
    k = len(cen)
    cost = np.zeros((k, 8), np.float32)
    for s in range(8):
        sx, sy, sz = (F32(-1) if s & 4 else F32(1)), (F32(-1) if s & 2 else F32(1)), (F32(-1) if s & 1 else F32(1))
        cost[:, s] = (((cen[:, 0] * sx).astype(np.float32) + (cen[:, 1] * sy).astype(np.float32)).astype(np.float32) + (cen[:, 2] * sz).astype(np.float32)).astype(np.float32)
    c = cost.astype(np.float64).tolist()
    slot_of = [-1] * k; used = [False] * 8
    for _ in range(k):
        bi = bs = -1; bc = float(np.finfo(np.float32).max)
        for i in range(k):
            if slot_of[i] >= 0: continue
            for s in range(8):
                if not used[s] and c[i][s] < bc: bc = c[i][s]; bi = i; bs = s
        slot_of[bi] = bs; used[bs] = True
    return slot_of
