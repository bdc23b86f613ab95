// refit_host.cpp — the host builder (csrc/bvh_build.cpp) and the host refit (csrc/bvh_refit_host.cpp over bvh_refit.h) behind a C interface for
// tests/test_bvh_refit.py, compiled with a plain host compiler.  With -DHOST_REFIT_MAIN it is a stand-alone program instead, for a run
// under AddressSanitizer / UBSan: it builds trees of exactly sized heap arrays, refits them to moved triangles and checks what the refit
// promises without a model — the identity refit changes no byte, a refit and the refit back restore every byte, every triangle record is
// a, b - a, c - a of its primitive, and a pool that is no tree is refused untouched.
#include "../../phosphorus_mk2_amd/csrc/bvh_build.h"
#include "../../phosphorus_mk2_amd/csrc/bvh_refit.h"

#include <cstdio>
#include <cstring>

using namespace phx;

extern "C" {

void* hr_build(const float* tri_abc, uint32_t n, int threads) { Bvh8* b = new Bvh8(); build_bvh8(tri_abc, n, *b, threads); return b; }
void hr_free(void* h) { delete (Bvh8*)h; }
void hr_info(void* h, uint64_t* out) { Bvh8* b = (Bvh8*)h; out[0] = b->num_nodes; out[1] = b->num_tris; out[2] = b->depth; }
// the pool's elements; fills grid6 (grid.lo, grid.cell) and, when `capacity` elements suffice, the pool's 16 words per element
uint64_t hr_copy_pool(void* h, uint32_t* out, uint64_t capacity, float* grid6) {
  Bvh8* b = (Bvh8*)h;
  if (grid6) for (int a = 0; a < 3; ++a) { grid6[a] = b->grid.lo[a]; grid6[3 + a] = b->grid.cell[a]; }
  if (out && capacity >= b->pool.size()) std::memcpy(out, b->pool.data(), b->pool.size() * sizeof(PoolElem));
  return b->pool.size();
}
// refit the tree in place to the n triangles of tri_abc -> refit_bvh8's status
int hr_refit(void* h, const float* tri_abc, uint32_t n) {
  Bvh8* b = (Bvh8*)h;
  return refit_bvh8(b->pool.data(), (uint32_t)b->pool.size(), tri_abc, n, &b->grid);
}
// refit a caller's pool (any builder's) in place -> the status; grid6 receives the new grid
int hr_refit_pool(uint32_t* pool, uint32_t num_elems, const float* tri_abc, uint32_t n, float* grid6) {
  SceneGrid g{};
  const int rc = refit_bvh8(reinterpret_cast<PoolElem*>(pool), num_elems, tri_abc, n, &g);
  if (!rc) for (int a = 0; a < 3; ++a) { grid6[a] = g.lo[a]; grid6[3 + a] = g.cell[a]; }
  return rc;
}

}  // extern "C"

#ifdef HOST_REFIT_MAIN
namespace {

uint32_t lcg(uint32_t& s) { s = s * 1664525u + 1013904223u; return s >> 8; }
float unit(uint32_t& s) { return (float)lcg(s) / 16777216.0f; }

std::vector<float> cloud(uint32_t n, uint32_t seed) {
  std::vector<float> abc(9 * (size_t)n);
  for (uint32_t i = 0; i < n; ++i) {
    const float c[3] = {2.0f * unit(seed) - 1.0f, 2.0f * unit(seed) - 1.0f, 2.0f * unit(seed) - 3.5f};
    for (int k = 0; k < 9; ++k) abc[9 * (size_t)i + k] = c[k % 3] + 0.2f * unit(seed) - 0.1f;
  }
  return abc;
}

int check(const char* name, uint32_t n) {
  const std::vector<float> abc = cloud(n, 17u + n);
  Bvh8 b; build_bvh8(abc.data(), n, b, 2);
  std::vector<PoolElem> pool(b.pool.begin(), b.pool.end());  // an allocation of exactly the pool's size
  const std::vector<PoolElem> built = pool;
  SceneGrid g{};
  int bad = 0;
  auto same = [](const std::vector<PoolElem>& x, const std::vector<PoolElem>& y) { return std::memcmp(x.data(), y.data(), x.size() * sizeof(PoolElem)) == 0; };
  // identity
  bad += refit_bvh8(pool.data(), (uint32_t)pool.size(), abc.data(), n, &g) != 0;
  bad += !same(pool, built) || std::memcmp(&g, &b.grid, sizeof(g)) != 0;
  // moved (a shear and a far translation: another grid), records checked, then back
  std::vector<float> moved(abc);
  for (size_t i = 0; i < moved.size(); i += 3) { moved[i] = moved[i] + 0.5f * moved[i + 1] + 1.0e4f; moved[i + 2] = 0.25f * moved[i + 2]; }
  bad += refit_bvh8(pool.data(), (uint32_t)pool.size(), moved.data(), n, &g) != 0;
  uint32_t tris = 0;
  for (uint32_t p = 0; p < n; ++p) {
    const TriRec& T = pool[b.elem_of_prim[p]].tri;
    const float* t = moved.data() + 9 * (size_t)p;
    if (T.prim == p && T.v0x == t[0] && T.v0y == t[1] && T.v0z == t[2] && T.e0x == t[3] - t[0] && T.e0y == t[4] - t[1] && T.e0z == t[5] - t[2] &&
        T.e1x == t[6] - t[0] && T.e1y == t[7] - t[1] && T.e1z == t[8] - t[2]) ++tris;
  }
  bad += tris != n;
  bad += refit_bvh8(pool.data(), (uint32_t)pool.size(), abc.data(), n, &g) != 0;
  bad += !same(pool, built);
  // refusals: a child base that points back, a primitive outside the scene, fewer primitives than records
  std::vector<PoolElem> broken = built;
  broken[0].node.child_base = 0;
  bad += refit_bvh8(broken.data(), (uint32_t)broken.size(), abc.data(), n, &g) == 0;
  broken[0].node.child_base = (uint32_t)broken.size();
  bad += refit_bvh8(broken.data(), (uint32_t)broken.size(), abc.data(), n, &g) == 0;
  broken[0].node.child_base = built[0].node.child_base;
  bad += !same(broken, built);
  bad += refit_bvh8(pool.data(), (uint32_t)pool.size(), abc.data(), n - 1, &g) == 0;
  bad += !same(pool, built);
  std::printf("%s %u elements %s\n", name, (unsigned)pool.size(), bad ? "FAILED" : "as-expected");
  return bad;
}

}  // namespace

int main() {
  int bad = 0;
  bad += check("n2", 2); bad += check("n9", 9); bad += check("n65", 65); bad += check("n1025", 1025);
  return bad;
}
#endif
