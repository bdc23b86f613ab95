// denoise_check.cpp — see denoise_check.h.
#include "denoise_check.h"
#include "film_checks.h"

namespace phx {

namespace {
const char* denoise_invalid(const phx_denoise& d, const float* film_in, const float* film_out) {
  static const char* const layout[4] = {"xstride", "normals_offset", "m2_offset", "samples_offset"};
  if (const char* field = film_size_invalid(d.width, d.height)) return field;
  if (const int k = film_layout_invalid(d.xstride, d.normals_offset, d.m2_offset, d.samples_offset, 6u, ~0u, false); k >= 0) return layout[k];
  if (d.spp < 2u) return "spp";
  if (d.iterations > 8u) return "iterations";
  if (!finite_positive(d.sigma_l)) return "sigma_l";
  if (d.normal_power_log2 > 10u) return "normal_power_log2";
  if (d.on_device > 1u) return "on_device";
  if (any_reserved(d.reserved)) return "reserved";
  if (!film_in) return "film_in";
  if (!film_out) return "film_out";
  const uint64_t bytes = (uint64_t)d.width * d.height * d.xstride * sizeof(float);
  if (film_in != film_out && share_a_byte(film_in, bytes, film_out, bytes)) return "film_out";  // in place, or two films apart
  return nullptr;
}
}  // namespace

int denoise_check(const phx_denoise& d, const float* film_in, const float* film_out, std::string& err) {
  return refusal("denoise", denoise_invalid(d, film_in, film_out), "phx_denoise", err);
}

}  // namespace phx
