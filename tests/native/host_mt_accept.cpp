// Test helper (tests only): mt_intersect of csrc/bvh8.h — the triangle test the host and the device share — on caller-made rays and
// triangle records, one call per pair (tests/test_mt_accept_edges.py).
#include "../../phosphorus_mk2_amd/csrc/bvh8.h"
using namespace phx;
extern "C" {
// tri: n x 9 floats (v0, e0, e1); o, d: n x 3.  accept[i] = mt_intersect's result; us, vs, ds as it leaves them.
void hmt_accept(uint32_t n, const float* tri, const uint32_t* prim, const float* o, const float* d, const float* tmax, const uint32_t* best_prim,
                uint8_t* accept, float* us, float* vs, float* ds) {
  for (uint32_t i = 0; i < n; ++i) {
    const float* t = tri + 9 * (size_t)i;
    TriRec T{};
    T.v0x = t[0]; T.v0y = t[1]; T.v0z = t[2]; T.e0x = t[3]; T.e0y = t[4]; T.e0z = t[5]; T.e1x = t[6]; T.e1y = t[7]; T.e1z = t[8];
    T.prim = prim[i];
    accept[i] = mt_intersect(T, v3(o[3 * i], o[3 * i + 1], o[3 * i + 2]), v3(d[3 * i], d[3 * i + 1], d[3 * i + 2]), tmax[i], best_prim[i], us[i], vs[i], ds[i]) ? 1 : 0;
  }
}
}
