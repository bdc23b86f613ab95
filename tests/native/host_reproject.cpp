// host_reproject.cpp — the argument check of phx_dev_film_reproject and its camera derivation (csrc/reproject_check.cpp) behind a C interface
// for tests/test_reproject.py, compiled with a plain host compiler.  With -DHOST_REPROJECT_MAIN it is a stand-alone program instead, for a
// run under AddressSanitizer / UBSan: it checks the cases listed in main() and prints, per line, the case and the answer.
#include "../../phosphorus_mk2_amd/csrc/reproject_check.h"

#include <cstdio>
#include <cstring>
#include <limits>

using namespace phx;

extern "C" {

// -> the status; err: the refusal's text (empty when accepted).  The films are addresses only: nothing is read through them.
int hr_check(const phx_reproject* r, const float* acc_from, const float* guides_from, const float* guides_to, const float* acc_to, char* err, uint32_t err_room) {
  std::string why;
  ReprojectCamera from{}, to{};
  const int rc = reproject_check(*r, acc_from, guides_from, guides_to, acc_to, from, to, why);
  if (err && err_room) { std::strncpy(err, why.c_str(), err_room - 1); err[err_room - 1] = 0; }
  return rc;
}

// -> 1 and out16 = o[3], inv[9] row-major, zoom, ratio, w, h; or 0 for a refused camera
int hr_camera(const phx_camera* c, double* out16) {
  ReprojectCamera k{};
  if (!reproject_camera(*c, k)) return 0;
  for (int i = 0; i < 3; ++i) out16[i] = k.o[i];
  for (int i = 0; i < 9; ++i) out16[3 + i] = k.inv[i];
  out16[12] = k.zoom; out16[13] = k.ratio; out16[14] = k.w; out16[15] = k.h;
  return 1;
}

uint32_t hr_sizeof(void) { return (uint32_t)sizeof(phx_reproject); }
uint32_t hr_sizeof_summary(void) { return (uint32_t)sizeof(phx_reproject_summary); }

}  // extern "C"

#ifdef HOST_REPROJECT_MAIN
namespace {
phx_camera camera(float tx) {
  phx_camera c{};
  c.to_world[0] = c.to_world[5] = c.to_world[10] = c.to_world[15] = 1.0f;
  c.to_world[12] = tx;
  c.fov = 0.9f; c.focal_distance = 1.0f; c.film_width = 64; c.film_height = 48;
  return c;
}
phx_reproject good() {
  phx_reproject r{};
  r.width = 64; r.height = 48;
  r.xstride_a = 14; r.normals_offset_a = 4; r.m2_offset_a = 7; r.samples_offset_a = 10;
  r.xstride_g = 8; r.on_device = 0; r.from = camera(0.0f); r.to = camera(0.25f);
  r.sigma_plane = 1.0f; r.sigma_dist = 4.0f; r.max_history = 64;
  return r;
}
void show(const char* name, const phx_reproject& r, const float* a, const float* gf, const float* gt, const float* out) {
  char err[128];
  const int rc = hr_check(&r, a, gf, gt, out, err, sizeof err);
  std::printf("%s %d %s\n", name, rc, err);
}
}  // namespace

int main() {
  static float films[64 * 48 * (14 + 8 + 8 + 14)];
  float* a = films; float* gf = a + 64 * 48 * 14; float* gt = gf + 64 * 48 * 8; float* out = gt + 64 * 48 * 8;
  phx_reproject r = good();
  show("good", r, a, gf, gt, out);
  show("same", r, a, gf, gt, a);
  show("overlap-guides-from", r, a, gf, gt, gf + 1);
  show("overlap-guides-to", r, a, gf, gt, gt - 1);
  show("null-acc-from", r, nullptr, gf, gt, out);
  show("null-guides-from", r, a, nullptr, gt, out);
  show("null-guides-to", r, a, gf, nullptr, out);
  show("null-acc-to", r, a, gf, gt, nullptr);
  r = good(); r.width = 0; show("width", r, a, gf, gt, out);
  r = good(); r.height = 65537; show("height", r, a, gf, gt, out);
  r = good(); r.xstride_a = 25; show("xstride-a", r, a, gf, gt, out);
  r = good(); r.m2_offset_a = 0xfffffffeu; show("m2-wrap", r, a, gf, gt, out);
  r = good(); r.normals_offset_a = 0; show("no-normals", r, a, gf, gt, out);
  r = good(); r.samples_offset_a = 0; show("no-samples", r, a, gf, gt, out);
  r = good(); r.xstride_g = 7; show("xstride-g", r, a, gf, gt, out);
  r = good(); r.on_device = 2; show("on-device", r, a, gf, gt, out);
  r = good(); r.from.film_width = 63; show("from-size", r, a, gf, gt, out);
  r = good(); r.from.to_world[0] = 0.0f; show("from-singular", r, a, gf, gt, out);
  r = good(); r.to.to_world[13] = std::numeric_limits<float>::infinity(); show("to-origin", r, a, gf, gt, out);
  r = good(); r.to.fov = std::numeric_limits<float>::quiet_NaN(); show("to-fov", r, a, gf, gt, out);
  r = good(); r.sigma_plane = 0.0f; show("sigma-plane", r, a, gf, gt, out);
  r = good(); r.sigma_dist = std::numeric_limits<float>::quiet_NaN(); show("sigma-dist", r, a, gf, gt, out);
  r = good(); r.max_history = 1; show("max-history", r, a, gf, gt, out);
  r = good(); r.reserved[2] = 1; show("reserved", r, a, gf, gt, out);
  double k[16];
  phx_camera c = camera(0.5f);
  const int ok = hr_camera(&c, k);
  std::printf("camera %d %.17g %.17g\n", ok, k[0], k[12]);
  return 0;
}
#endif
