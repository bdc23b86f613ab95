// bvh_refit_host.cpp — the host's refit of a BVH8 pool (bvh_refit.h): the rule the device's refit (bvh_refit.hip) is held to, without a device.
// Host code only.
#include "bvh_refit.h"

#include <vector>

namespace phx {

int refit_bvh8(PoolElem* pool, uint32_t num_elems, const float* abc, uint32_t num_prims, SceneGrid* grid) {
  if (!pool || !abc || !grid || num_elems == 0 || num_prims == 0) return 1;
  // what every element is: the pool is breadth first, so one ascending pass meets every nodelet before its children
  std::vector<uint8_t> kind(num_elems, 0);
  kind[0] = REFIT_NODE;
  uint32_t tris = 0;
  for (uint32_t e = 0; e < num_elems; ++e) {
    if (kind[e] == REFIT_TRI) { if (pool[e].tri.prim >= num_prims) return 1; ++tris; continue; }
    if (kind[e] != REFIT_NODE) return 1;  // an element no nodelet points at
    uint32_t valid, imask;
    const int cnt = refit_children(pool[e].node, e, num_elems, valid, imask);
    if (cnt < 0) return 1;
    uint32_t rank = 0;
    for (int s = 0; s < 8; ++s) {
      if (!(valid & (1u << s))) continue;
      uint8_t& k = kind[pool[e].node.child_base + rank++];
      if (k) return 1;  // two parents
      k = (imask & (1u << s)) ? REFIT_NODE : REFIT_TRI;
    }
  }
  if (tris != num_prims) return 1;

  float glo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, ghi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
  for (size_t i = 0; i < 9 * (size_t)num_prims; ++i) { glo[i % 3] = fminf(glo[i % 3], abc[i]); ghi[i % 3] = fmaxf(ghi[i % 3], abc[i]); }
  const float delta = tri_box_inflation(glo, ghi);
  for (int a = 0; a < 3; ++a) { glo[a] -= delta; ghi[a] += delta; }
  *grid = make_scene_grid(glo, ghi);

  std::vector<RefitBox> boxes(num_elems);
  for (uint32_t e = num_elems; e-- > 0;) {  // children before parents
    if (kind[e] == REFIT_TRI) refit_triangle(pool[e].tri, abc + 9 * (size_t)pool[e].tri.prim, delta, boxes[e]);
    else refit_nodelet(pool[e].node, *grid, boxes.data(), boxes[e]);
  }
  return 0;
}

}  // namespace phx
