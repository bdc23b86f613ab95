// bvh_gpu.h — device-side LBVH build of the BVH8 pool of bvh8.h (see bvh_gpu.hip).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

#include "bvh8.h"

namespace phx {

struct GpuBvh {
  PoolElem* pool;      // hipMalloc'd (2 x triangles elements reserved), owned by the caller after a successful build
  uint32_t num_elems;  // elements in use: nodelets + triangle records (material word already filled)
  uint32_t num_nodes, num_tris, depth;
  SceneGrid grid;      // the grid the nodelets' origins are stored on
  float cost;          // modelled traversal cost of the collapse (sub(root) of k_collapse_dp; 0 if greedy): comparable with Bvh8::cost
};

// d_abc: 9 floats per primitive (a, b, c) in scene_t::triangles() order, device memory.
// d_prim_material: per-primitive material word (material | smooth << 31), device memory.
// Returns 0 on success; on failure writes a message to err and leaves *out empty: BVH_GPU_RECOVERABLE when the cause is one a host
// build can step around (the builder's scratch or pool did not fit the device's free memory; the tree is deeper than the traversal's
// tables), 1 for everything else — a HIP error from a launch or a sync, or a builder that lost triangles: bugs, never to be hidden.
enum { BVH_GPU_RECOVERABLE = 2 };
// d_elem_of_prim (optional, n words of device memory): receives the pool index of every primitive's triangle record.
int build_bvh8_gpu(hipStream_t stream, const float* d_abc, const uint32_t* d_prim_material, uint32_t n, GpuBvh* out, char* err, size_t errlen, uint32_t* d_elem_of_prim = nullptr);

// The geometry bounds of d_abc as the builder takes them (k_prim_bounds: fp32 min / max of every vertex) -> lo[3], hi[3]; synchronises the
// stream.  Returns like build_bvh8_gpu.
int geometry_bounds_gpu(hipStream_t stream, const float* d_abc, uint32_t n, float* lo, float* hi, char* err, size_t errlen);

// ---- refit (bvh_refit.hip; the rule is bvh_refit.h's) --------------------------------------------------------------------------------------
struct GpuRefit {
  uint32_t levels;   // levels of pool elements walked: the nodelets' and the deepest triangles' below them
  float bounds[6];   // geometry bounds of d_abc, lo.xyz hi.xyz
  float delta;       // tri_box_inflation(bounds)
  SceneGrid grid;    // of the bounds grown by delta: what every nodelet is now encoded on
};
// Refits `pool` (num_elems elements, either builder's, device memory) in place to the n triangles of d_abc: topology, slots, masks, child
// bases and prims stay; triangle records, nodelet origins, exponents and planes are what the builder's emission would write for this
// topology over d_abc.  d_elem_of_prim (n words) receives every primitive's pool index.  Scratch (a byte and a box per element) lives
// during the call.  Returns like build_bvh8_gpu.  Checked by the walk, before the first write: every nodelet's children lie behind its level
// inside the pool, every element is reached, there are n triangle records and each names a primitive below n.  Not checked: that no two records
// name the same primitive (the other's d_elem_of_prim word then stays 0xffffffff, which the commit's kernels skip).
int refit_bvh8_gpu(hipStream_t stream, PoolElem* pool, uint32_t num_elems, const float* d_abc, uint32_t n, uint32_t* d_elem_of_prim, GpuRefit* out, char* err, size_t errlen);
// d_elem_of_prim (n words) of a finished pool, by the refit's walk
int pool_elem_of_prim_gpu(hipStream_t stream, const PoolElem* pool, uint32_t num_elems, uint32_t n, uint32_t* d_elem_of_prim, char* err, size_t errlen);
// by_prim[p] = by_elem[elem_of_prim[p]] for rows of `width` floats (a word that is no index into the num_elems rows of by_elem is skipped)
void launch_gather_rows(hipStream_t stream, const float* by_elem, const uint32_t* elem_of_prim, float* by_prim, uint32_t n, uint32_t width, uint32_t num_elems);

}  // namespace phx
