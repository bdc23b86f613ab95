"""A plain model of the BVH8 refit (csrc/bvh_refit.h), for tests: numpy over bvh_model.walk_pool's structures, no GPU, no ctypes.

Restated from the comments of bvh_refit.h and bvh8.h; it shares no code with the library.  The rule: topology, slots, valid, imask,
child_base and prim stay.  From the new triangles abc:

  bounds    the fp32 min / max of every vertex; delta = tri_box_inflation(bounds); the scene grid of the bounds grown by delta
  triangle  its record's v0, e0, e1 = a, b - a, c - a in fp32; its box the vertices' min / max grown by delta (bvh_model.leaf_boxes)
  nodelet   its box the fp32 min / max of its children's boxes, bottom-up (bvh_model.child_boxes); then the encode: the largest grid
            index whose decoded coordinate fma(i, cell, lo) does not exceed the box's lower corner; per axis the least exponent e with
            255 * 2^e >= (hi - origin) * 1.00001, within -126 .. 127; per child floor((lo - origin) / 2^e - 1e-3) and
            ceil((hi - origin) / 2^e + 1e-3) in binary64, clamped to 0 .. 255; 255 / 0 in empty slots

refit(pool, glo, gcell, abc) -> (pool, glo, gcell) after the refit."""
import numpy as np

import bvh_model as M

F32, F64 = np.float32, np.float64


def scene_grid(lo, hi):
    """make_scene_grid: cell = fp32((hi - lo) / (2^18 - 1)) in binary64, 1e-30 where that is not a positive finite float"""
    c = ((hi.astype(F64) - lo.astype(F64)) / float(M.GRID_MAX)).astype(F32)
    bad = ~(c > 0) | ~(c < F32(3.0e38))
    return lo.astype(F32), np.where(bad, F32(1.0e-30), c).astype(F32)


def grid_index_below(x, lo, cell):
    """per axis [n, 3]: the largest index whose decoded coordinate does not exceed x (0 when x lies below the grid)"""
    t = np.floor((x.astype(F64) - lo.astype(F64)[None, :]) / cell.astype(F64)[None, :])
    t = np.where(t > 0.0, t, 0.0)
    i = np.minimum(t, float(M.GRID_MAX)).astype(np.int64)
    while True:
        over = (i > 0) & (M.fma32(i, cell[None, :], lo[None, :]) > x)
        if not over.any():
            return i
        i = i - over


def exponents(ext):
    """the least e with 255 * 2^e >= ext * 1.00001, clamped to -126 .. 127; -126 for ext <= 0.  ceil(log2 x) from frexp (exact), then the
    correction loop of the encode"""
    e = np.full(ext.shape, -126, np.int64)
    pos = ext > 0.0
    want = ext * 1.00001
    m, k = np.frexp(np.where(pos, want / 255.0, 1.0))
    c = np.where(m > 0.5, k, k - 1).astype(np.int64)
    while True:
        short = pos & (np.ldexp(255.0, c) < want)
        if not short.any():
            break
        c = c + short
    return np.clip(np.where(pos, c, e), -126, 127)


def refit(pool, glo, gcell, abc):
    pool = np.ascontiguousarray(pool, np.uint32).reshape(-1, 16)
    abc = np.ascontiguousarray(abc, F32).reshape(-1, 9)
    W = M.walk_pool(pool, glo, gcell)
    B = M.leaf_boxes(abc)
    nglo, ncell = scene_grid((B.glo - B.delta).astype(F32), (B.ghi + B.delta).astype(F32))
    out = pool.copy()
    # triangle records
    t = abc.reshape(-1, 3, 3)[W.tri_prim]
    rec = np.concatenate([t[:, 0], (t[:, 1] - t[:, 0]).astype(F32), (t[:, 2] - t[:, 0]).astype(F32)], 1).astype(F32)
    out[W.tri_elem, 0:9] = rec.view(np.uint32)
    # nodelets
    clo, chi, nlo, nhi = M.child_boxes(W, B.ilo, B.ihi)
    gi = grid_index_below(nlo, nglo, ncell)
    org = M.fma32(gi, ncell[None, :], nglo[None, :]).astype(F64)
    e = exponents(nhi.astype(F64) - org)
    scale = np.ldexp(1.0, e)
    v = W.vbit[:, :, None]                                                                     # [n, slot, 1]
    qlo = np.floor((np.where(v, clo, 0).astype(F64) - org[:, None, :]) / scale[:, None, :] - 1e-3)
    qhi = np.ceil((np.where(v, chi, 0).astype(F64) - org[:, None, :]) / scale[:, None, :] + 1e-3)
    qlo = np.where(v, np.clip(qlo, 0.0, 255.0), 255.0).astype(np.uint8)                         # [n, slot, axis]
    qhi = np.where(v, np.clip(qhi, 0.0, 255.0), 0.0).astype(np.uint8)
    word = gi[:, 0].astype(np.uint64) | (gi[:, 1].astype(np.uint64) << np.uint64(18)) | (gi[:, 2].astype(np.uint64) << np.uint64(36)) | \
        (W.valid.astype(np.uint64) << np.uint64(54))
    out[W.node, 0] = (word & np.uint64(0xffffffff)).astype(np.uint32)
    out[W.node, 1] = (word >> np.uint64(32)).astype(np.uint32)
    eb = (e + 127).astype(np.uint32)
    out[W.node, 2] = eb[:, 0] | (eb[:, 1] << np.uint32(8)) | (eb[:, 2] << np.uint32(16)) | (W.imask.astype(np.uint32) << np.uint32(24))
    planes = np.concatenate([np.transpose(qlo, (0, 2, 1)), np.transpose(qhi, (0, 2, 1))], 1)    # [n, 6, slot]: lox loy loz hix hiy hiz
    out8 = out.view(np.uint8).reshape(-1, 64)
    out8[W.node, 16:] = planes.reshape(-1, 48)
    return out, nglo, ncell
