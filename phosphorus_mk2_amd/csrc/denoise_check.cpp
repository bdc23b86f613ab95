// denoise_check.cpp — see denoise_check.h.
#include "denoise_check.h"

#include <cmath>
#include <cstdint>

namespace phx {

namespace {
// a channel of `len` floats at `off`: behind "primary" and inside the pixel
bool channel_fits(uint32_t off, uint32_t len, uint32_t xstride) { return off >= 3u && (uint64_t)off + len <= xstride; }
bool channels_overlap(uint32_t a, uint32_t alen, uint32_t b, uint32_t blen) { return (uint64_t)a < (uint64_t)b + blen && (uint64_t)b < (uint64_t)a + alen; }

const char* denoise_invalid(const phx_denoise& d, const float* film_in, const float* film_out) {
  if (d.width < 1u || d.width > 65536u) return "width";
  if (d.height < 1u || d.height > 65536u) return "height";
  if (d.xstride < 6u) return "xstride";
  if (!channel_fits(d.m2_offset, 3u, d.xstride)) return "m2_offset";
  if (d.normals_offset && (!channel_fits(d.normals_offset, 3u, d.xstride) || channels_overlap(d.normals_offset, 3u, d.m2_offset, 3u))) return "normals_offset";
  if (d.samples_offset && (!channel_fits(d.samples_offset, 1u, d.xstride) || channels_overlap(d.samples_offset, 1u, d.m2_offset, 3u) ||
                           (d.normals_offset && channels_overlap(d.samples_offset, 1u, d.normals_offset, 3u))))
    return "samples_offset";
  if (d.spp < 2u) return "spp";
  if (d.iterations > 8u) return "iterations";
  if (!std::isfinite(d.sigma_l) || !(d.sigma_l > 0.0f)) return "sigma_l";
  if (d.normal_power_log2 > 10u) return "normal_power_log2";
  if (d.on_device > 1u) return "on_device";
  for (uint32_t w : d.reserved) if (w) return "reserved";
  if (!film_in) return "film_in";
  if (!film_out) return "film_out";
  if (film_in != film_out) {  // two films: they must not share a float
    const uint64_t bytes = (uint64_t)d.width * d.height * d.xstride * sizeof(float);
    const uintptr_t a = reinterpret_cast<uintptr_t>(film_in), b = reinterpret_cast<uintptr_t>(film_out);
    if ((a < b ? b - a : a - b) < bytes) return "film_out";
  }
  return nullptr;
}
}  // namespace

int denoise_check(const phx_denoise& d, const float* film_in, const float* film_out, std::string& err) {
  const char* field = denoise_invalid(d, film_in, film_out);
  if (!field) return PHX_OK;
  err = std::string("denoise: ") + field + " is outside its range (phx_denoise)";
  return PHX_ERR_ARG;
}

}  // namespace phx
