// outlier_clamp_check.cpp — see outlier_clamp_check.h.
#include "outlier_clamp_check.h"
#include "film_checks.h"

namespace phx {

namespace {
const char* outlier_clamp_invalid(const phx_outlier_clamp& c, const float* film, const float* ref, const float* film_out, bool& ref_needs_copy) {
  if (c.width < 1u || c.width > 65536u) return "width";
  if (c.height < 1u || c.height > 65536u) return "height";
  if (c.xstride_a < 3u || c.xstride_a > (uint32_t)PHX_OUTLIER_MAX_XSTRIDE) return "xstride_a";
  if (c.m2_offset_a && !channel_fits(c.m2_offset_a, 3u, c.xstride_a)) return "m2_offset_a";
  if (c.samples_offset_a && (!channel_fits(c.samples_offset_a, 1u, c.xstride_a) || (c.m2_offset_a && channels_overlap(c.samples_offset_a, 1u, c.m2_offset_a, 3u))))
    return "samples_offset_a";
  if (c.xstride_b < 3u || c.xstride_b > (uint32_t)PHX_OUTLIER_MAX_XSTRIDE) return "xstride_b";
  if (c.on_device > 1u) return "on_device";
  if (c.flags & ~(uint32_t)(PHX_OUTLIER_EXCLUDE_CENTRE | PHX_OUTLIER_UPPER_ONLY)) return "flags";
  if (c.radius < 1u || c.radius > (uint32_t)PHX_OUTLIER_MAX_RADIUS) return "radius";
  if (c.trim > 3u) return "trim";
  const uint32_t side = 2u * c.radius + 1u;
  if (c.min_taps < 1u || c.min_taps > side * side) return "min_taps";
  if (!std::isfinite(c.gamma) || c.gamma < 0.0f) return "gamma";
  if (!std::isfinite(c.floor) || c.floor < 0.0f) return "floor";
  if (c.clamped_history && !c.samples_offset_a) return "clamped_history";
  for (uint32_t w : c.reserved) if (w) return "reserved";
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
