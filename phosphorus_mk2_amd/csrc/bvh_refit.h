// bvh_refit.h — the one statement of how a nodelet of bvh8.h is encoded from boxes, and the refit built on it: same topology, new boxes.
//
// encode_node8 is what the device builder's emission (bvh_gpu.hip: k_collapse) writes of a nodelet besides its topology: the grid index at
// or below the node's lower corner, the three scale exponents, the outward 8-bit planes of every child.  It reads the node's fp32 box and
// the children's fp32 boxes and nothing else, so a tree whose triangles moved is brought up to date by recomputing boxes bottom-up and
// encoding every nodelet again — slots, valid, imask, child_base and prim stay.  The header compiles for the device (the
// builder, bvh_refit.hip: one launch per level) and for the host (bvh_refit_host.cpp: refit_bvh8, the CPU tests' yardstick).
#pragma once
#include "bvh8.h"

#include <cstddef>

namespace phx {

struct RefitBox { float lo[3], hi[3]; };

// The header words (origin + valid, exponents) and the 48 plane bytes of `nd` from the node's box and the boxes of its children by SLOT
// (cbox: 6 floats per slot, lo.xyz hi.xyz; read where `valid` has the slot's bit).  imask and child_base are not touched.
// Everything is relative to the DECODED origin fma(i, cell, lo): the exponent is the least e with 255 * 2^e >= (hi - origin) * 1.00001
// (ceil(log2) and a correction loop against a log2 that rounds down), a plane is floor(x / 2^e - 1e-3) or ceil(x / 2^e + 1e-3) clamped to
// 0 .. 255; an empty slot holds the inverted box 255 > 0.
PHX_HD void encode_node8(Node8& nd, const SceneGrid& grid, const float* nlo, const float* nhi, const float* cbox, uint32_t valid) {
  uint32_t gi[3]; float org[3];
  for (int a = 0; a < 3; ++a) { gi[a] = grid_index_below(nlo[a], grid.lo[a], grid.cell[a]); org[a] = fmaf((float)gi[a], grid.cell[a], grid.lo[a]); }
  double scale[3]; uint8_t eb[3];
  for (int a = 0; a < 3; ++a) {
    const double ext = (double)nhi[a] - (double)org[a];
    int ex = -126;
    if (ext > 0.0) {
      ex = (int)ceil(log2(ext * 1.00001 / 255.0));
      while (ldexp(255.0, ex) < ext * 1.00001) ++ex;
    }
    ex = ex < -126 ? -126 : (ex > 127 ? 127 : ex);
    eb[a] = (uint8_t)(ex + 127);
    scale[a] = ldexp(1.0, ex);
  }
  nd.ex = eb[0]; nd.ey = eb[1]; nd.ez = eb[2];
  for (int s = 0; s < 8; ++s) {
    uint8_t ql[3] = {255, 255, 255}, qh[3] = {0, 0, 0};
    if (valid & (1u << s)) {
      const float* b = cbox + 6 * s;
      for (int a = 0; a < 3; ++a) {
        double lo = floor(((double)b[a] - (double)org[a]) / scale[a] - 1e-3);
        double hi = ceil(((double)b[3 + a] - (double)org[a]) / scale[a] + 1e-3);
        lo = fmax(0.0, fmin(255.0, lo)); hi = fmax(0.0, fmin(255.0, hi));
        ql[a] = (uint8_t)lo; qh[a] = (uint8_t)hi;
      }
    }
    nd.qlox[s] = ql[0]; nd.qloy[s] = ql[1]; nd.qloz[s] = ql[2]; nd.qhix[s] = qh[0]; nd.qhiy[s] = qh[1]; nd.qhiz[s] = qh[2];
  }
  node_origin_encode(nd, gi[0], gi[1], gi[2], valid);
}

// ---- the refit's two element rules ---------------------------------------------------------------------------------------------------------
// A triangle record from its three vertices t[0..8] (a, b, c): v0, e0, e1 by the builders' expressions; prim, material and the spare words
// stay.  Its box is the vertices' min / max (not v0 + e0: that sum rounds) grown by delta.
PHX_HD void refit_triangle(TriRec& R, const float* t, float delta, RefitBox& box) {
  R.v0x = t[0]; R.v0y = t[1]; R.v0z = t[2];
  R.e0x = t[3] - t[0]; R.e0y = t[4] - t[1]; R.e0z = t[5] - t[2];
  R.e1x = t[6] - t[0]; R.e1y = t[7] - t[1]; R.e1z = t[8] - t[2];
  for (int a = 0; a < 3; ++a) {
    box.lo[a] = fminf(fminf(t[a], t[3 + a]), t[6 + a]) - delta;
    box.hi[a] = fmaxf(fmaxf(t[a], t[3 + a]), t[6 + a]) + delta;
  }
}
// A nodelet from the boxes of its children, `boxes` indexed by pool element (the children lie behind the node: a deeper level).  Its own
// box is their fp32 min / max, which is exact, so the order shows nowhere.
PHX_HD void refit_nodelet(Node8& nd, const SceneGrid& grid, const RefitBox* boxes, RefitBox& own) {
  const uint32_t valid = (nd.origin_hi >> 22) & 0xffu;
  float cbox[48];
  for (int a = 0; a < 3; ++a) { own.lo[a] = FLT_MAX; own.hi[a] = -FLT_MAX; }
  uint32_t rank = 0;
  for (int s = 0; s < 8; ++s) {
    if (!(valid & (1u << s))) continue;
    const RefitBox b = boxes[nd.child_base + rank++];
    for (int a = 0; a < 3; ++a) {
      cbox[6 * s + a] = b.lo[a]; cbox[6 * s + 3 + a] = b.hi[a];
      own.lo[a] = fminf(own.lo[a], b.lo[a]); own.hi[a] = fmaxf(own.hi[a], b.hi[a]);
    }
  }
  encode_node8(nd, grid, own.lo, own.hi, cbox, valid);
}

// What the elements of a pool are, by one walk from the root: REFIT_NODE, REFIT_TRI, 0 = not reached.
enum : uint8_t { REFIT_NODE = 1, REFIT_TRI = 2 };
// The children of nodelet `nd` at pool index e: -> their count, or -1 when they do not lie behind e inside the pool (a pool that is not
// the breadth-first layout of bvh8.h; nothing may be written by such a node's indices)
PHX_HD int refit_children(const Node8& nd, uint32_t e, uint32_t num_elems, uint32_t& valid, uint32_t& imask) {
  valid = (nd.origin_hi >> 22) & 0xffu; imask = nd.imask;
  const uint32_t cnt = (uint32_t)popc32(valid);
  if (nd.child_base <= e || nd.child_base > num_elems || cnt > num_elems - nd.child_base || (imask & ~valid)) return -1;
  return (int)cnt;
}

// ---- host (bvh_refit_host.cpp) -------------------------------------------------------------------------------------------------------------------
// Refits `pool` (num_elems elements, either builder's) to the triangles abc (9 floats per primitive, num_prims of them, indexed by the
// records' prim): the geometry bounds, delta = tri_box_inflation(bounds), the scene grid of the bounds grown by delta (as both builders
// derive them), every triangle record and every nodelet.  -> 0 and *grid, or 1 for a pool that is not a tree over num_prims primitives
// (it is left as it was).
int refit_bvh8(PoolElem* pool, uint32_t num_elems, const float* abc, uint32_t num_prims, SceneGrid* grid);

}  // namespace phx
