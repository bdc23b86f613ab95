// display_check.cpp — see display_check.h.
#include "display_check.h"
#include "film_checks.h"

namespace phx {

namespace {
const char* display_invalid(const phx_display& p, const float* film, const uint8_t* image) {
  if (const char* field = film_size_invalid(p.width, p.height)) return field;
  if (p.xstride < 3u || p.xstride > (uint32_t)PHX_DISPLAY_MAX_XSTRIDE) return "xstride";
  if (p.image_pitch && (p.image_pitch % 4u || p.image_pitch < 4ull * p.width)) return "image_pitch";
  if (p.on_device > 2u) return "on_device";
  if (p.flags & ~(uint32_t)(PHX_DISPLAY_DITHER | PHX_DISPLAY_AUTO_EXPOSURE)) return "flags";
  if (p.tone > (uint32_t)PHX_TONE_ACES) return "tone";
  if (!finite_positive(p.scale)) return "scale";
  if (p.tone == (uint32_t)PHX_TONE_REINHARD && !finite_positive(p.white)) return "white";
  if (p.flags & PHX_DISPLAY_AUTO_EXPOSURE) {
    if (!finite_positive(p.key)) return "key";
    if (p.low_q16 >= p.high_q16) return "low_q16";
    if (p.high_q16 > 65536u) return "high_q16";
    if (!finite_positive(p.min_scale)) return "min_scale";
    if (!std::isfinite(p.max_scale) || p.max_scale < p.min_scale) return "max_scale";
  }
  if (any_reserved(p.reserved)) return "reserved";
  if (!film) return "film";
  if (!image || reinterpret_cast<uintptr_t>(image) % 4u) return "image";
  if (share_a_byte(film, (uint64_t)p.width * p.height * p.xstride * sizeof(float), image, display_image_bytes(p))) return "image";
  return nullptr;
}
}  // namespace

int display_check(const phx_display& p, const float* film, const uint8_t* image, std::string& err) {
  return refusal("display", display_invalid(p, film, image), "phx_display", err);
}

}  // namespace phx
