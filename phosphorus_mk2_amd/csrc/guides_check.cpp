// guides_check.cpp — see guides_check.h.
#include "guides_check.h"
#include "film_checks.h"

namespace phx {

namespace {
const char* guides_invalid(const phx_guides& g, uint32_t width, uint32_t height, uint32_t spp, const float* film) {
  if (g.samples < 1u || g.samples > spp) return "samples";
  if ((uint64_t)width * height * g.samples >= 0x7fffffffull) return "samples";  // path = pixel * samples + sample is a 32-bit word
  if (g.on_device > 1u) return "on_device";
  if (any_reserved(g.reserved)) return "reserved";
  if (!film) return "film";
  return nullptr;
}
const char* denoise_guides_invalid(const phx_denoise& d, const phx_denoise_guides& g) {
  if (g.flags & ~(uint32_t)(PHX_GUIDE_DEMODULATE | PHX_GUIDE_PLANE)) return "flags";
  if ((g.flags & PHX_GUIDE_PLANE) && !d.normals_offset) return "normals_offset";
  if (g.xstride < 8u) return "xstride";
  if ((g.flags & PHX_GUIDE_DEMODULATE) && !finite_positive(g.albedo_floor)) return "albedo_floor";
  if ((g.flags & PHX_GUIDE_PLANE) && !finite_positive(g.sigma_x)) return "sigma_x";
  if ((g.flags & PHX_GUIDE_PLANE) && !finite_positive(g.plane_scale)) return "plane_scale";
  if (any_reserved(g.reserved)) return "reserved";
  if (!g.guides) return "guides";
  return nullptr;
}
}  // namespace

int guides_check(const phx_guides& g, uint32_t width, uint32_t height, uint32_t spp, const float* film, std::string& err) {
  return refusal("render_guides", guides_invalid(g, width, height, spp, film), "phx_guides", err);
}

int denoise_guides_check(const phx_denoise& d, const phx_denoise_guides& g, std::string& err) {
  return refusal("denoise_guided", denoise_guides_invalid(d, g), "phx_denoise_guides", err);
}

}  // namespace phx
