// outlier_clamp_check.cpp — see outlier_clamp_check.h.
#include "outlier_clamp_check.h"
#include "film_checks.h"

namespace phx {

namespace {
const char* outlier_clamp_invalid(const phx_outlier_clamp& c, const float* film, const float* ref, const float* film_out, bool& ref_needs_copy) {
  static const char* const names_a[4] = {"xstride_a", nullptr /* the clamp reads no normals */, "m2_offset_a", "samples_offset_a"};
  if (const char* field = film_size_invalid(c.width, c.height)) return field;
  if (const int k = film_layout_invalid(c.xstride_a, 0u, c.m2_offset_a, c.samples_offset_a, 3u, (uint32_t)PHX_OUTLIER_MAX_XSTRIDE, false, false); k >= 0) return names_a[k];
  if (c.xstride_b < 3u || c.xstride_b > (uint32_t)PHX_OUTLIER_MAX_XSTRIDE) return "xstride_b";
  if (c.on_device > 1u) return "on_device";
  if (c.flags & ~(uint32_t)(PHX_OUTLIER_EXCLUDE_CENTRE | PHX_OUTLIER_UPPER_ONLY)) return "flags";
  if (c.radius < 1u || c.radius > (uint32_t)PHX_OUTLIER_MAX_RADIUS) return "radius";
  if (c.trim > 3u) return "trim";
  const uint32_t side = 2u * c.radius + 1u;
  if (c.min_taps < 1u || c.min_taps > side * side) return "min_taps";
  if (!finite_nonneg(c.gamma)) return "gamma";
  if (!finite_nonneg(c.floor)) return "floor";
  if (c.clamped_history && !c.samples_offset_a) return "clamped_history";
  if (any_reserved(c.reserved)) return "reserved";
  if (!film) return "film";
  if (!ref) return "ref";
  if (!film_out) return "film_out";
  const uint64_t npix = (uint64_t)c.width * c.height;
  const uint64_t bytes_a = npix * c.xstride_a * sizeof(float), bytes_b = npix * c.xstride_b * sizeof(float);
  // two films are one another exactly (the same address and the same bytes) or share no byte
  const bool ref_is_film = ref == film && bytes_b == bytes_a, out_is_film = film_out == film, out_is_ref = film_out == ref && bytes_a == bytes_b;
  if (!ref_is_film && share_a_byte(ref, bytes_b, film, bytes_a)) return "ref";
  if (!out_is_film && share_a_byte(film_out, bytes_a, film, bytes_a)) return "film_out";
  if (!out_is_ref && share_a_byte(film_out, bytes_a, ref, bytes_b)) return "film_out";
  ref_needs_copy = out_is_ref;
  return nullptr;
}
}  // namespace

int outlier_clamp_check(const phx_outlier_clamp& c, const float* film, const float* ref, const float* film_out, bool& ref_needs_copy, std::string& err) {
  ref_needs_copy = false;
  return refusal("outlier_clamp", outlier_clamp_invalid(c, film, ref, film_out, ref_needs_copy), "phx_outlier_clamp", err);
}

}  // namespace phx
