// accumulate_check.cpp — see accumulate_check.h.
#include "accumulate_check.h"
#include "film_checks.h"

namespace phx {

namespace {
const char* accumulate_invalid(const phx_accumulate& a, const float* acc, const float* frame_film) {
  static const char* const names_a[4] = {"xstride_a", "normals_offset_a", "m2_offset_a", "samples_offset_a"};
  static const char* const names_b[4] = {"xstride_b", "normals_offset_b", "m2_offset_b", "samples_offset_b"};
  const uint32_t max_xstride = (uint32_t)PHX_ACCUMULATE_MAX_XSTRIDE;
  if (const char* field = film_size_invalid(a.width, a.height)) return field;
  if (const int k = film_layout_invalid(a.xstride_a, a.normals_offset_a, a.m2_offset_a, a.samples_offset_a, 7u, max_xstride, true); k >= 0) return names_a[k];
  if (const int k = film_layout_invalid(a.xstride_b, a.normals_offset_b, a.m2_offset_b, a.samples_offset_b, 6u, max_xstride, false); k >= 0) return names_b[k];
  if (!a.samples_offset_b && a.spp_b < 1u) return "spp_b";
  if (a.on_device > 1u) return "on_device";
  if (!finite_nonneg(a.tau)) return "tau";
  if (!finite_nonneg(a.floor)) return "floor";
  if (any_reserved(a.reserved)) return "reserved";
  if (!acc) return "acc";
  if (!frame_film) return "frame_film";
  const uint64_t npix = (uint64_t)a.width * a.height;
  if (share_a_byte(acc, npix * a.xstride_a * sizeof(float), frame_film, npix * a.xstride_b * sizeof(float))) return "frame_film";
  return nullptr;
}
}  // namespace

int accumulate_check(const phx_accumulate& a, const float* acc, const float* frame_film, std::string& err) {
  return refusal("accumulate", accumulate_invalid(a, acc, frame_film), "phx_accumulate", err);
}

}  // namespace phx
