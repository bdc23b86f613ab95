// host_accumulate.cpp — the argument check of phx_dev_film_accumulate (csrc/accumulate_check.cpp) behind a C interface for
// tests/test_accumulate.py, compiled with a plain host compiler.  With -DHOST_ACCUMULATE_MAIN it is a stand-alone program instead, for a run
// under AddressSanitizer / UBSan: it checks the cases listed in main() and prints, per line, the case and the answer.
#include "../../phosphorus_mk2_amd/csrc/accumulate_check.h"

#include <cstdio>
#include <cstring>
#include <limits>

using namespace phx;

extern "C" {

// -> the status; err: the refusal's text (empty when accepted).  The films are addresses only: nothing is read through them.
int ha_check(const phx_accumulate* a, const float* acc, const float* frame_film, char* err, uint32_t err_room) {
  std::string why;
  const int rc = accumulate_check(*a, acc, frame_film, why);
  if (err && err_room) { std::strncpy(err, why.c_str(), err_room - 1); err[err_room - 1] = 0; }
  return rc;
}

uint32_t ha_sizeof(void) { return (uint32_t)sizeof(phx_accumulate); }
uint32_t ha_sizeof_summary(void) { return (uint32_t)sizeof(phx_accumulate_summary); }

}  // extern "C"

#ifdef HOST_ACCUMULATE_MAIN
namespace {
phx_accumulate good() {
  phx_accumulate a{};
  a.width = 64; a.height = 48;
  a.xstride_a = 11; a.normals_offset_a = 4; a.m2_offset_a = 7; a.samples_offset_a = 10;
  a.xstride_b = 10; a.normals_offset_b = 4; a.m2_offset_b = 7; a.samples_offset_b = 0;
  a.spp_b = 16; a.on_device = 0; a.tau = 0.05f; a.floor = 0.01f;
  return a;
}
void show(const char* name, const phx_accumulate& a, const float* acc, const float* frame) {
  char err[128];
  const int rc = ha_check(&a, acc, frame, err, sizeof err);
  std::printf("%s %d %s\n", name, rc, err);
}
}  // namespace

int main() {
  static float films[64 * 48 * (11 + 10)];
  float* acc = films; float* frame = films + 64 * 48 * 11;
  phx_accumulate a = good();
  show("good", a, acc, frame);
  show("same", a, acc, acc);
  show("overlap", a, acc, frame - 1);
  show("null-acc", a, nullptr, frame);
  show("null-frame", a, acc, nullptr);
  a = good(); a.width = 0; show("width", a, acc, frame);
  a = good(); a.height = 65537; show("height", a, acc, frame);
  a = good(); a.xstride_a = 25; show("xstride-a", a, acc, frame);
  a = good(); a.xstride_b = 5; show("xstride-b", a, acc, frame);
  a = good(); a.m2_offset_a = 0xfffffffeu; show("m2-wrap", a, acc, frame);
  a = good(); a.normals_offset_b = 6; show("normals-overlap", a, acc, frame);
  a = good(); a.samples_offset_a = 0; show("no-samples-a", a, acc, frame);
  a = good(); a.samples_offset_b = 10; show("samples-past", a, acc, frame);
  a = good(); a.spp_b = 0; show("spp", a, acc, frame);
  a = good(); a.on_device = 2; show("on-device", a, acc, frame);
  a = good(); a.tau = std::numeric_limits<float>::quiet_NaN(); show("tau-nan", a, acc, frame);
  a = good(); a.floor = -1.0f; show("floor", a, acc, frame);
  a = good(); a.reserved[1] = 1; show("reserved", a, acc, frame);
  return 0;
}
#endif
