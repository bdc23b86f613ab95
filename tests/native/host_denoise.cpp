// host_denoise.cpp — the argument check of phx_dev_denoise (csrc/denoise_check.cpp) behind a C interface for tests/test_denoise.py, compiled
// with a plain host compiler.  With -DHOST_DENOISE_MAIN it is a stand-alone program instead, for a run under AddressSanitizer / UBSan: it
// checks the cases listed in main() and prints, per line, the case and the answer.
#include "../../phosphorus_mk2_amd/csrc/denoise_check.h"

#include <cstdio>
#include <cstring>
#include <limits>

using namespace phx;

extern "C" {

// -> the status; err: the refusal's text (empty when accepted).  The films are addresses only: nothing is read through them.
int hd_check(const phx_denoise* d, const float* film_in, const float* film_out, char* err, uint32_t err_room) {
  std::string why;
  const int rc = denoise_check(*d, film_in, film_out, why);
  if (err && err_room) { std::strncpy(err, why.c_str(), err_room - 1); err[err_room - 1] = 0; }
  return rc;
}

uint32_t hd_sizeof(void) { return (uint32_t)sizeof(phx_denoise); }

}  // extern "C"

#ifdef HOST_DENOISE_MAIN
namespace {
phx_denoise good() {
  phx_denoise d{};
  d.width = 64; d.height = 48; d.xstride = 11; d.normals_offset = 4; d.m2_offset = 7; d.samples_offset = 10; d.spp = 16; d.iterations = 5;
  d.sigma_l = 4.0f; d.normal_power_log2 = 7; d.on_device = 0;
  return d;
}
void show(const char* name, const phx_denoise& d, const float* in, const float* out) {
  char err[128];
  const int rc = hd_check(&d, in, out, err, sizeof err);
  std::printf("%s %d %s\n", name, rc, err);
}
}  // namespace

int main() {
  static float a[64 * 48 * 11 * 2];
  float* b = a + 64 * 48 * 11;
  phx_denoise d = good();
  show("good", d, a, b);
  show("in-place", d, a, a);
  show("overlap", d, a, a + 11);
  show("null-in", d, nullptr, b);
  show("null-out", d, a, nullptr);
  d = good(); d.width = 0; show("width", d, a, b);
  d = good(); d.height = 65537; show("height", d, a, b);
  d = good(); d.xstride = 5; show("xstride", d, a, b);
  d = good(); d.m2_offset = 0xfffffffeu; show("m2-wrap", d, a, b);
  d = good(); d.normals_offset = 6; show("normals-overlap", d, a, b);
  d = good(); d.samples_offset = 11; show("samples-past", d, a, b);
  d = good(); d.spp = 1; show("spp", d, a, b);
  d = good(); d.iterations = 9; show("iterations", d, a, b);
  d = good(); d.sigma_l = std::numeric_limits<float>::quiet_NaN(); show("sigma-nan", d, a, b);
  d = good(); d.normal_power_log2 = 11; show("power", d, a, b);
  d = good(); d.on_device = 2; show("on-device", d, a, b);
  d = good(); d.reserved[4] = 1; show("reserved", d, a, b);
  return 0;
}
#endif
