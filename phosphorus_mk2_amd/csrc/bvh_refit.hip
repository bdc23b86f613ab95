// bvh_refit.hip — the device's refit of the BVH8 pool (bvh_refit.h): the triangles moved, the topology stays.
//
// The pool is breadth first (bvh8.h): a level is a contiguous range of elements and the children of a nodelet are contiguous in the next.
//   k_refit_mark    top-down, one launch per level: every nodelet of the level marks its children as nodelet or triangle record and
//                   raises the end of the next level (one atomicMax per nodelet); the host reads that end between launches, as the builder
//                   reads its queue length.  A nodelet whose children do not lie behind its level inside the pool, an element no nodelet
//                   pointed at and a triangle record whose prim lies outside the scene raise an error word, and the records are counted:
//                   nothing below is launched on a pool that fails there, so such a pool is refused before the first write.
//   k_refit_level   bottom-up, one launch per level: a triangle record is rewritten from abc (v0, e0, e1), its box (the vertices' min / max
//                   grown by delta) and its elem_of_prim word are stored; a nodelet takes the boxes the deeper launch left for its children,
//                   stores their union as its own and is encoded again on the new scene grid (encode_node8).
// No workgroup waits for another inside a launch: the hand-off between levels is the kernel boundary.  Stores are plain vector stores.
#include "bvh_gpu.h"
#include "bvh_refit.h"

#include <cstdio>
#include <cstring>
#include <vector>

#include <hip/hip_runtime.h>

namespace phx {
namespace {

#define RB 256

__global__ void __launch_bounds__(RB) k_refit_mark(const PoolElem* __restrict__ pool, uint32_t begin, uint32_t end, uint32_t num_elems, uint32_t num_prims,
                                                   uint8_t* __restrict__ kind, uint32_t* __restrict__ state /* [0] end of the next level, [1] error, [2] triangle records */) {
  const uint32_t e = begin + blockIdx.x * RB + threadIdx.x;
  const uint8_t mine = e < end ? kind[e] : (uint8_t)0xff;
  // the level's triangle records, counted per wave (one address sustains ~90 atomics per microsecond: a million records one by one would be 11 ms)
  const unsigned long long tris = __ballot(mine == REFIT_TRI);
  if (tris && __lane_id() == (unsigned)__ffsll((long long)tris) - 1u) atomicAdd(&state[2], (uint32_t)__popcll(tris));
  if (e >= end) return;
  if (mine == REFIT_TRI) {
    if (pool[e].tri.prim >= num_prims) atomicOr(&state[1], 2u);
    return;
  }
  if (mine != REFIT_NODE) { atomicOr(&state[1], 4u); return; }  // an element no nodelet points at
  const uint4 h = *reinterpret_cast<const uint4*>(&pool[e]);
  Node8 nd; nd.origin_lo = h.x; nd.origin_hi = h.y; nd.imask = (uint8_t)(h.z >> 24); nd.child_base = h.w;
  uint32_t valid, imask;
  const int cnt = refit_children(nd, end - 1u, num_elems, valid, imask);  // behind the whole level: the next one
  if (cnt < 0) { atomicOr(&state[1], 1u); return; }
  uint32_t rank = 0;
  for (int s = 0; s < 8; ++s) if (valid & (1u << s)) kind[nd.child_base + rank++] = (imask & (1u << s)) ? REFIT_NODE : REFIT_TRI;
  atomicMax(&state[0], nd.child_base + (uint32_t)cnt);
}

__global__ void __launch_bounds__(RB) k_refit_level(PoolElem* __restrict__ pool, uint32_t begin, uint32_t end, const uint8_t* __restrict__ kind, const float* __restrict__ abc,
                                                    uint32_t num_prims, float delta, SceneGrid grid, RefitBox* __restrict__ boxes, uint32_t* __restrict__ elem_of_prim,
                                                    uint32_t* __restrict__ state) {
  const uint32_t e = begin + blockIdx.x * RB + threadIdx.x;
  if (e >= end) return;
  uint4* w = reinterpret_cast<uint4*>(&pool[e]);
  RefitBox own;
  if (kind[e] == REFIT_TRI) {
    const uint32_t p = pool[e].tri.prim;
    if (p >= num_prims) { atomicOr(&state[1], 2u); return; }
    const float* src = abc + 9 * (size_t)p;
    float t[9];
    for (int k = 0; k < 9; ++k) t[k] = src[k];
    TriRec R;
    refit_triangle(R, t, delta, own);
    w[0] = make_uint4(__float_as_uint(R.v0x), __float_as_uint(R.v0y), __float_as_uint(R.v0z), __float_as_uint(R.e0x));
    w[1] = make_uint4(__float_as_uint(R.e0y), __float_as_uint(R.e0z), __float_as_uint(R.e1x), __float_as_uint(R.e1y));
    pool[e].tri.e1z = R.e1z;  // prim, material and the spare words stay
    elem_of_prim[p] = e;
  } else if (kind[e] == REFIT_NODE) {
    Node8 nd = pool[e].node;
    refit_nodelet(nd, grid, boxes, own);
    const uint4* q = reinterpret_cast<const uint4*>(&nd);
    w[0] = q[0]; w[1] = q[1]; w[2] = q[2]; w[3] = q[3];
  } else {
    atomicOr(&state[1], 4u);  // an element no nodelet points at
    return;
  }
  boxes[e] = own;
}

// the pool index of every primitive's triangle record, read back from a pool (a rebuild carries the corner UVs over by it)
__global__ void __launch_bounds__(RB) k_elem_of_prim(const PoolElem* __restrict__ pool, uint32_t num_elems, const uint8_t* __restrict__ kind, uint32_t num_prims,
                                                     uint32_t* __restrict__ elem_of_prim) {
  const uint32_t e = blockIdx.x * RB + threadIdx.x;
  if (e >= num_elems || kind[e] != REFIT_TRI) return;
  const uint32_t p = pool[e].tri.prim;
  if (p < num_prims) elem_of_prim[p] = e;
}

// by_prim[p] = by_elem[elem_of_prim[p]], rows of `width` floats: a table by pool element back in primitive order
__global__ void __launch_bounds__(RB) k_gather_rows(const float* __restrict__ by_elem, const uint32_t* __restrict__ elem_of_prim, float* __restrict__ by_prim, uint32_t n, uint32_t width, uint32_t num_elems) {
  const uint32_t p = blockIdx.x * RB + threadIdx.x;
  if (p >= n) return;
  const uint32_t e = elem_of_prim[p];
  if (e >= num_elems) return;  // (a primitive without a record: pool_elem_of_prim_gpu left 0xffffffff)
  for (uint32_t k = 0; k < width; ++k) by_prim[(size_t)p * width + k] = by_elem[(size_t)e * width + k];
}

#define RCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::snprintf(err, errlen, "%s: %s", #x, hipGetErrorString(e_)); return 1; } } while (0)

struct Scratch {  // freed when the call returns
  std::vector<void*> bufs;
  void* get(size_t bytes) { void* p = nullptr; if (hipMalloc(&p, bytes < 16 ? 16 : bytes) != hipSuccess) { (void)hipGetLastError(); return nullptr; } bufs.push_back(p); return p; }
  ~Scratch() { for (void* p : bufs) (void)hipFree(p); }
};

// Marks every element of the pool and finds the levels: levels[k] .. levels[k + 1] is level k (the root's is 0 .. 1).
int mark_levels(hipStream_t stream, const PoolElem* pool, uint32_t num_elems, uint32_t num_prims, uint8_t* kind, uint32_t* state, std::vector<uint32_t>& levels, char* err, size_t errlen) {
  RCHK(hipMemsetAsync(kind, 0, num_elems, stream));
  const uint8_t root = REFIT_NODE;
  RCHK(hipMemcpyAsync(kind, &root, 1, hipMemcpyHostToDevice, stream));
  uint32_t h_state[3] = {1u, 0u, 0u};
  RCHK(hipMemcpyAsync(state, h_state, sizeof(h_state), hipMemcpyHostToDevice, stream));
  levels.assign({0u, 1u});
  for (;;) {
    const uint32_t begin = levels[levels.size() - 2], end = levels.back();
    hipLaunchKernelGGL(k_refit_mark, dim3((end - begin + RB - 1) / RB), dim3(RB), 0, stream, pool, begin, end, num_elems, num_prims, kind, state);
    RCHK(hipGetLastError());
    RCHK(hipMemcpyAsync(h_state, state, sizeof(h_state), hipMemcpyDeviceToHost, stream));
    RCHK(hipStreamSynchronize(stream));
    if (h_state[1] || h_state[0] < end || h_state[0] > num_elems) {
      std::snprintf(err, errlen, "refit: the pool is not a breadth-first BVH8 over %u primitives (level %zu, error bits %u)", num_prims, levels.size() - 2, h_state[1]);
      return 1;
    }
    if (h_state[0] == end) break;  // a level of triangle records alone: the last
    levels.push_back(h_state[0]);
    // nodelet levels + the triangles' below them
    if (levels.size() - 1 > (size_t)PHX_MAX_BVH_DEPTH + 1) { std::snprintf(err, errlen, "refit: more than %d levels", PHX_MAX_BVH_DEPTH); return 1; }
  }
  if (levels.back() != num_elems) { std::snprintf(err, errlen, "refit: the walk reached %u of %u pool elements", levels.back(), num_elems); return 1; }
  if (h_state[2] != num_prims) { std::snprintf(err, errlen, "refit: the pool holds %u triangle records for %u primitives", h_state[2], num_prims); return 1; }
  return 0;
}

}  // namespace

int refit_bvh8_gpu(hipStream_t stream, PoolElem* pool, uint32_t num_elems, const float* d_abc, uint32_t n, uint32_t* d_elem_of_prim, GpuRefit* out, char* err, size_t errlen) {
  std::memset(out, 0, sizeof(*out));
  if (!pool || !d_abc || !d_elem_of_prim || num_elems == 0 || n == 0) { std::snprintf(err, errlen, "refit: null argument"); return 1; }
  Scratch tmp;
  uint8_t* kind = (uint8_t*)tmp.get(num_elems);
  uint32_t* state = (uint32_t*)tmp.get(16);
  RefitBox* boxes = (RefitBox*)tmp.get(sizeof(RefitBox) * (size_t)num_elems);
  if (!kind || !state || !boxes) { std::snprintf(err, errlen, "hipMalloc failed (refit scratch)"); return BVH_GPU_RECOVERABLE; }
  float glo[3], ghi[3];
  if (const int rc = geometry_bounds_gpu(stream, d_abc, n, glo, ghi, err, errlen)) return rc;
  std::vector<uint32_t> levels;
  if (const int rc = mark_levels(stream, pool, num_elems, n, kind, state, levels, err, errlen)) return rc;
  RCHK(hipMemsetAsync(d_elem_of_prim, 0xff, 4 * (size_t)n, stream));  // (a primitive two records name leaves its twin's word at 0xffffffff: the commit's kernels skip it)
  const float delta = tri_box_inflation(glo, ghi);
  for (int a = 0; a < 3; ++a) { out->bounds[a] = glo[a]; out->bounds[3 + a] = ghi[a]; glo[a] -= delta; ghi[a] += delta; }
  out->delta = delta; out->grid = make_scene_grid(glo, ghi);
  for (size_t k = levels.size() - 1; k-- > 0;) {  // the deepest level first
    const uint32_t begin = levels[k], end = levels[k + 1];
    hipLaunchKernelGGL(k_refit_level, dim3((end - begin + RB - 1) / RB), dim3(RB), 0, stream, pool, begin, end, kind, d_abc, n, delta, out->grid, boxes, d_elem_of_prim, state);
  }
  RCHK(hipGetLastError());
  uint32_t h_state[2];
  RCHK(hipMemcpyAsync(h_state, state, sizeof(h_state), hipMemcpyDeviceToHost, stream));
  RCHK(hipStreamSynchronize(stream));
  if (h_state[1]) { std::snprintf(err, errlen, "refit: a triangle record names a primitive outside the scene, or an element is unreached (%u)", h_state[1]); return 1; }
  out->levels = (uint32_t)levels.size() - 1;
  return 0;
}

void launch_gather_rows(hipStream_t stream, const float* by_elem, const uint32_t* elem_of_prim, float* by_prim, uint32_t n, uint32_t width, uint32_t num_elems) {
  if (n) hipLaunchKernelGGL(k_gather_rows, dim3((n + RB - 1) / RB), dim3(RB), 0, stream, by_elem, elem_of_prim, by_prim, n, width, num_elems);
}

int pool_elem_of_prim_gpu(hipStream_t stream, const PoolElem* pool, uint32_t num_elems, uint32_t n, uint32_t* d_elem_of_prim, char* err, size_t errlen) {
  Scratch tmp;
  uint8_t* kind = (uint8_t*)tmp.get(num_elems);
  uint32_t* state = (uint32_t*)tmp.get(16);
  if (!kind || !state) { std::snprintf(err, errlen, "hipMalloc failed (refit scratch)"); return BVH_GPU_RECOVERABLE; }
  std::vector<uint32_t> levels;
  if (const int rc = mark_levels(stream, pool, num_elems, n, kind, state, levels, err, errlen)) return rc;
  RCHK(hipMemsetAsync(d_elem_of_prim, 0xff, 4 * (size_t)n, stream));
  hipLaunchKernelGGL(k_elem_of_prim, dim3((num_elems + RB - 1) / RB), dim3(RB), 0, stream, pool, num_elems, kind, n, d_elem_of_prim);
  RCHK(hipGetLastError());
  RCHK(hipStreamSynchronize(stream));
  return 0;
}

}  // namespace phx
