// film_checks.h — what the argument checks of the film calls share: the film's size, the tests of a float and of the reserved words, the one
// rule for a film's pixel layout, the test that two films share a byte, the refusal's text, and the check of the phx_adaptive setting.
// Every *_check.cpp states its call's own fields in their order and reads the rest here; device.cpp (phx_dev_set_adaptive) and
// film_calls.cpp (phx_dev_adaptive_select) read adaptive_invalid and the text.
//
// Host-only and header-only, like frame_plan.h: the ABI's structs and nothing else, every function inline, so each *_check.cpp still
// compiles alone with a plain host compiler (tests/native/host_*.cpp).
#pragma once
#include "../../include/phx_xpu.h"

#include <cmath>
#include <cstdint>
#include <string>

namespace phx {

// a film's size: the name of the first field outside [1, 65536], or nullptr
inline const char* film_size_invalid(uint32_t width, uint32_t height) {
  return width < 1u || width > 65536u ? "width" : height < 1u || height > 65536u ? "height" : nullptr;
}
inline bool finite_nonneg(float v) { return std::isfinite(v) && v >= 0.0f; }
inline bool finite_positive(float v) { return std::isfinite(v) && v > 0.0f; }
template <size_t N> inline bool any_reserved(const uint32_t (&reserved)[N]) {
  for (uint32_t w : reserved) if (w) return true;
  return false;
}

// a channel of `len` floats at `off`: behind "primary" and inside the pixel
inline bool channel_fits(uint32_t off, uint32_t len, uint32_t xstride) { return off >= 3u && (uint64_t)off + len <= xstride; }
inline bool channels_overlap(uint32_t a, uint32_t alen, uint32_t b, uint32_t blen) { return (uint64_t)a < (uint64_t)b + blen && (uint64_t)b < (uint64_t)a + alen; }

// The rule for a film's pixel layout, once: xstride within [min_xstride, max_xstride]; m2 (3 floats, 0 = none unless required) behind
// "primary" and inside the pixel; normals (3 floats, 0 = none) and samples (1 float, 0 = none unless required) likewise, overlapping neither
// m2 nor each other.
// -> which field is the first outside its range (0 xstride, 1 normals, 2 m2, 3 samples; tested in the order xstride, m2, normals, samples), or -1
inline int film_layout_invalid(uint32_t xstride, uint32_t normals, uint32_t m2, uint32_t samples, uint32_t min_xstride, uint32_t max_xstride, bool samples_required,
                               bool m2_required = true) {
  if (xstride < min_xstride || xstride > max_xstride) return 0;
  if (m2 ? !channel_fits(m2, 3u, xstride) : m2_required) return 2;
  if (normals && (!channel_fits(normals, 3u, xstride) || (m2 && channels_overlap(normals, 3u, m2, 3u)))) return 1;
  if (!samples && samples_required) return 3;
  if (samples && (!channel_fits(samples, 1u, xstride) || (m2 && channels_overlap(samples, 1u, m2, 3u)) || (normals && channels_overlap(samples, 1u, normals, 3u)))) return 3;
  return -1;
}

// [p, p + bytes_p) and [q, q + bytes_q) share a byte
inline bool share_a_byte(const void* p, uint64_t bytes_p, const void* q, uint64_t bytes_q) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
  return a <= b ? b - a < bytes_p : a - b < bytes_q;
}

// what a check says of the first field outside its range
inline std::string outside_its_range(const char* call, const char* field, const char* of_struct) {
  return std::string(call) + ": " + field + " is outside its range (" + of_struct + ")";
}
// a check's answer: PHX_OK for field == nullptr, else PHX_ERR_ARG with that text in `err`
inline int refusal(const char* call, const char* field, const char* of_struct, std::string& err) {
  if (!field) return PHX_OK;
  err = outside_its_range(call, field, of_struct);
  return PHX_ERR_ARG;
}

// phx_adaptive: the name of the first field outside its range, or nullptr
inline const char* adaptive_invalid(const phx_adaptive& a) {
  if (!finite_nonneg(a.threshold)) return "threshold";
  if (!finite_nonneg(a.floor)) return "floor";
  if (a.min_samples < 2u) return "min_samples";
  if (a.step < 1u) return "step";
  if (any_reserved(a.reserved)) return "reserved";
  return nullptr;
}

}  // namespace phx
