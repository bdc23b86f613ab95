// accumulate_check.cpp — see accumulate_check.h.
#include "accumulate_check.h"

#include <cmath>
#include <cstdint>

namespace phx {

namespace {
// a channel of `len` floats at `off`: behind "primary" and inside the pixel
bool channel_fits(uint32_t off, uint32_t len, uint32_t xstride) { return off >= 3u && (uint64_t)off + len <= xstride; }
bool channels_overlap(uint32_t a, uint32_t alen, uint32_t b, uint32_t blen) { return (uint64_t)a < (uint64_t)b + blen && (uint64_t)b < (uint64_t)a + alen; }

// one film's layout: -> which of its four fields (0 xstride, 1 normals, 2 m2, 3 samples) is outside its range, or -1
int layout_invalid(uint32_t xstride, uint32_t normals, uint32_t m2, uint32_t samples, bool samples_required) {
  if (xstride < (samples_required ? 7u : 6u) || xstride > (uint32_t)PHX_ACCUMULATE_MAX_XSTRIDE) return 0;
  if (!channel_fits(m2, 3u, xstride)) return 2;
  if (normals && (!channel_fits(normals, 3u, xstride) || channels_overlap(normals, 3u, m2, 3u))) return 1;
  if (!samples && samples_required) return 3;
  if (samples && (!channel_fits(samples, 1u, xstride) || channels_overlap(samples, 1u, m2, 3u) || (normals && channels_overlap(samples, 1u, normals, 3u)))) return 3;
  return -1;
}

const char* accumulate_invalid(const phx_accumulate& a, const float* acc, const float* frame_film) {
  static const char* const names_a[4] = {"xstride_a", "normals_offset_a", "m2_offset_a", "samples_offset_a"};
  static const char* const names_b[4] = {"xstride_b", "normals_offset_b", "m2_offset_b", "samples_offset_b"};
  if (a.width < 1u || a.width > 65536u) return "width";
  if (a.height < 1u || a.height > 65536u) return "height";
  if (const int k = layout_invalid(a.xstride_a, a.normals_offset_a, a.m2_offset_a, a.samples_offset_a, true); k >= 0) return names_a[k];
  if (const int k = layout_invalid(a.xstride_b, a.normals_offset_b, a.m2_offset_b, a.samples_offset_b, false); k >= 0) return names_b[k];
  if (!a.samples_offset_b && a.spp_b < 1u) return "spp_b";
  if (a.on_device > 1u) return "on_device";
  if (!std::isfinite(a.tau) || a.tau < 0.0f) return "tau";
  if (!std::isfinite(a.floor) || a.floor < 0.0f) return "floor";
  for (uint32_t w : a.reserved) if (w) return "reserved";
  if (!acc) return "acc";
  if (!frame_film) return "frame_film";
  // the two films must not share a byte: [p, p + bytes_p) and [q, q + bytes_q)
  const uint64_t npix = (uint64_t)a.width * a.height;
  const uint64_t bytes_a = npix * a.xstride_a * sizeof(float), bytes_b = npix * a.xstride_b * sizeof(float);
  const uintptr_t p = reinterpret_cast<uintptr_t>(acc), q = reinterpret_cast<uintptr_t>(frame_film);
  if (p <= q ? q - p < bytes_a : p - q < bytes_b) return "frame_film";
  return nullptr;
}
}  // namespace

int accumulate_check(const phx_accumulate& a, const float* acc, const float* frame_film, std::string& err) {
  const char* field = accumulate_invalid(a, acc, frame_film);
  if (!field) return PHX_OK;
  err = std::string("accumulate: ") + field + " is outside its range (phx_accumulate)";
  return PHX_ERR_ARG;
}

}  // namespace phx
