// host_guides.cpp — the argument checks of phx_dev_render_guides and phx_dev_denoise_guided (csrc/guides_check.cpp) behind a C interface for
// tests/test_guides.py, compiled with a plain host compiler.  With -DHOST_GUIDES_MAIN it is a stand-alone program instead, for a run under
// AddressSanitizer / UBSan: it checks the cases listed in main() and prints, per line, the case and the answer.
#include "../../phosphorus_mk2_amd/csrc/guides_check.h"

#include <cstdio>
#include <cstring>
#include <limits>

using namespace phx;

namespace {
int answer(int rc, const std::string& why, char* err, uint32_t err_room) {
  if (err && err_room) { std::strncpy(err, why.c_str(), err_room - 1); err[err_room - 1] = 0; }
  return rc;
}
}  // namespace

extern "C" {

// -> the status; err: the refusal's text (empty when accepted).  The films are addresses only: nothing is read through them.
int hg_check_guides(const phx_guides* g, uint32_t width, uint32_t height, uint32_t spp, const float* film, char* err, uint32_t err_room) {
  std::string why;
  return answer(guides_check(*g, width, height, spp, film, why), why, err, err_room);
}
int hg_check_denoise_guides(const phx_denoise* d, const phx_denoise_guides* g, char* err, uint32_t err_room) {
  std::string why;
  return answer(denoise_guides_check(*d, *g, why), why, err, err_room);
}

uint32_t hg_sizeof_guides(void) { return (uint32_t)sizeof(phx_guides); }
uint32_t hg_sizeof_denoise_guides(void) { return (uint32_t)sizeof(phx_denoise_guides); }

}  // extern "C"

#ifdef HOST_GUIDES_MAIN
namespace {
float film[8];
phx_guides good() {
  phx_guides g{};
  g.sampler_seed = 7; g.samples = 4; g.on_device = 0;
  return g;
}
phx_denoise good_film() {
  phx_denoise d{};
  d.width = 64; d.height = 48; d.xstride = 10; d.normals_offset = 4; d.m2_offset = 7; d.spp = 16; d.iterations = 5; d.sigma_l = 4.0f; d.normal_power_log2 = 7;
  return d;
}
phx_denoise_guides good_guides() {
  phx_denoise_guides g{};
  g.guides = film; g.xstride = 8; g.flags = PHX_GUIDE_DEMODULATE | PHX_GUIDE_PLANE; g.albedo_floor = 0.01f; g.sigma_x = 1.0f; g.plane_scale = 0.002f;
  return g;
}
void show(const char* name, const phx_guides& g, uint32_t spp, const float* f) {
  char err[128];
  const int rc = hg_check_guides(&g, 64, 48, spp, f, err, sizeof err);
  std::printf("%s %d %s\n", name, rc, err);
}
void show(const char* name, const phx_denoise& d, const phx_denoise_guides& g) {
  char err[128];
  const int rc = hg_check_denoise_guides(&d, &g, err, sizeof err);
  std::printf("%s %d %s\n", name, rc, err);
}
}  // namespace

int main() {
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  phx_guides g = good();
  show("good", g, 16, film);
  g = good(); g.samples = 16; show("all-samples", g, 16, film);
  g = good(); g.samples = 0; show("no-samples", g, 16, film);
  g = good(); g.samples = 17; show("samples-past-spp", g, 16, film);
  g = good(); g.samples = 0xffffffffu; show("samples-wrap", g, 0xffffffffu, film);
  g = good(); g.on_device = 2; show("on-device", g, 16, film);
  g = good(); g.reserved[3] = 1; show("reserved", g, 16, film);
  g = good(); show("null-film", g, 16, nullptr);

  const phx_denoise d = good_film();
  phx_denoise_guides q = good_guides();
  show("d-good", d, q);
  q = good_guides(); q.flags = 4; show("d-flags", d, q);
  q = good_guides(); { phx_denoise e = d; e.normals_offset = 0; show("d-plane-without-normals", e, q); }
  q = good_guides(); q.flags = PHX_GUIDE_DEMODULATE; { phx_denoise e = d; e.normals_offset = 0; show("d-demodulate-without-normals", e, q); }
  q = good_guides(); q.xstride = 7; show("d-xstride", d, q);
  q = good_guides(); q.albedo_floor = 0.0f; show("d-floor-zero", d, q);
  q = good_guides(); q.albedo_floor = nan; show("d-floor-nan", d, q);
  q = good_guides(); q.flags = PHX_GUIDE_PLANE; q.albedo_floor = nan; show("d-floor-unused", d, q);
  q = good_guides(); q.sigma_x = -1.0f; show("d-sigma-x", d, q);
  q = good_guides(); q.plane_scale = inf; show("d-plane-scale", d, q);
  q = good_guides(); q.flags = PHX_GUIDE_DEMODULATE; q.sigma_x = nan; q.plane_scale = 0.0f; show("d-plane-unused", d, q);
  q = good_guides(); q.reserved[0] = 1; show("d-reserved", d, q);
  q = good_guides(); q.guides = nullptr; show("d-null-guides", d, q);
  return 0;
}
#endif
