// host_outlier_clamp.cpp — the argument check of phx_dev_film_outlier_clamp (csrc/outlier_clamp_check.cpp) behind a C interface for
// tests/test_outlier_clamp.py, compiled with a plain host compiler.  With -DHOST_OUTLIER_CLAMP_MAIN it is a stand-alone program instead, for
// a run under AddressSanitizer / UBSan: it checks the cases listed in main() and prints, per line, the case, the answer and whether the call
// would work from a copy of ref.
#include "../../phosphorus_mk2_amd/csrc/outlier_clamp_check.h"

#include <cstdio>
#include <cstring>
#include <limits>

using namespace phx;

extern "C" {

// -> the status; err: the refusal's text (empty when accepted); *copy: 1 when the call would take its bounds from a copy of ref.
// The films are addresses only: nothing is read through them.
int ho_check(const phx_outlier_clamp* c, const float* film, const float* ref, const float* film_out, char* err, uint32_t err_room, int* copy) {
  std::string why;
  bool needs_copy = false;
  const int rc = outlier_clamp_check(*c, film, ref, film_out, needs_copy, why);
  if (err && err_room) { std::strncpy(err, why.c_str(), err_room - 1); err[err_room - 1] = 0; }
  if (copy) *copy = needs_copy ? 1 : 0;
  return rc;
}

uint32_t ho_sizeof(void) { return (uint32_t)sizeof(phx_outlier_clamp); }
uint32_t ho_sizeof_summary(void) { return (uint32_t)sizeof(phx_outlier_clamp_summary); }

}  // extern "C"

#ifdef HOST_OUTLIER_CLAMP_MAIN
namespace {
phx_outlier_clamp good() {
  phx_outlier_clamp c{};
  c.width = 64; c.height = 48;
  c.xstride_a = 11; c.m2_offset_a = 7; c.samples_offset_a = 10; c.xstride_b = 11; c.on_device = 0;
  c.flags = PHX_OUTLIER_EXCLUDE_CENTRE | PHX_OUTLIER_UPPER_ONLY; c.radius = 2; c.trim = 2; c.min_taps = 4;
  c.gamma = 4.0f; c.floor = 0.0f; c.clamped_history = 0;
  return c;
}
void show(const char* name, const phx_outlier_clamp& c, const float* film, const float* ref, const float* out) {
  char err[128]; int copy = 0;
  const int rc = ho_check(&c, film, ref, out, err, sizeof err, &copy);
  std::printf("%s %d %d %s\n", name, rc, copy, err);
}
}  // namespace

int main() {
  static float films[3 * 64 * 48 * 11];
  float* a = films; float* b = a + 64 * 48 * 11; float* out = b + 64 * 48 * 11;
  phx_outlier_clamp c = good();
  show("good", c, a, b, out);
  show("in-place", c, a, b, a);
  show("self", c, a, a, out);
  show("self-in-place", c, a, a, a);
  show("out-is-ref", c, a, b, b);
  show("ref-overlaps-film", c, a, a + 1, out);
  show("out-overlaps-film", c, a, b, a + 11);
  show("out-overlaps-ref", c, a, b, b - 1);
  show("null-film", c, nullptr, b, out);
  show("null-ref", c, a, nullptr, out);
  show("null-out", c, a, b, nullptr);
  c = good(); c.xstride_b = 3; show("self-other-stride", c, a, a, out);
  c = good(); c.width = 0; show("width", c, a, b, out);
  c = good(); c.height = 65537; show("height", c, a, b, out);
  c = good(); c.xstride_a = 25; show("xstride-a", c, a, b, out);
  c = good(); c.m2_offset_a = 0xfffffffeu; show("m2-wrap", c, a, b, out);
  c = good(); c.samples_offset_a = 8; show("samples-in-m2", c, a, b, out);
  c = good(); c.xstride_b = 2; show("xstride-b", c, a, b, out);
  c = good(); c.on_device = 2; show("on-device", c, a, b, out);
  c = good(); c.flags = 4; show("flags", c, a, b, out);
  c = good(); c.radius = 4; show("radius", c, a, b, out);
  c = good(); c.trim = 4; show("trim", c, a, b, out);
  c = good(); c.min_taps = 26; show("min-taps", c, a, b, out);
  c = good(); c.gamma = std::numeric_limits<float>::quiet_NaN(); show("gamma", c, a, b, out);
  c = good(); c.floor = -1.0f; show("floor", c, a, b, out);
  c = good(); c.samples_offset_a = 0; c.clamped_history = 8; show("clamped-history", c, a, b, out);
  c = good(); c.reserved[1] = 1; show("reserved", c, a, b, out);
  return 0;
}
#endif
