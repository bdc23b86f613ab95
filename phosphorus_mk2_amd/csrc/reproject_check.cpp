// reproject_check.cpp — see reproject_check.h.
#include "reproject_check.h"
#include "film_checks.h"

namespace phx {

bool reproject_camera(const phx_camera& c, ReprojectCamera& out) {
  const float* M = c.to_world;
  const double a = M[0], b = M[1], cc = M[2], d = M[4], e = M[5], f = M[6], g = M[8], h = M[9], k = M[10];
  const double A = e * k - f * h, B = f * g - d * k, C = d * h - e * g;
  const double det = (a * A + b * B) + cc * C;
  if (!std::isfinite(det) || det == 0.0) return false;
  out.inv[0] = A / det; out.inv[1] = (cc * h - b * k) / det; out.inv[2] = (b * f - cc * e) / det;
  out.inv[3] = B / det; out.inv[4] = (a * k - cc * g) / det; out.inv[5] = (cc * d - a * f) / det;
  out.inv[6] = C / det; out.inv[7] = (b * g - a * h) / det;  out.inv[8] = (a * e - b * d) / det;
  for (int i = 0; i < 3; ++i) out.o[i] = (double)M[12 + i];
  out.zoom = 1.12 * std::tan((double)c.fov * 0.5);
  out.w = (double)c.film_width; out.h = (double)c.film_height;
  if (c.film_width == 0u || c.film_height == 0u) return false;
  out.ratio = out.w / out.h;
  for (double v : out.inv) if (!std::isfinite(v)) return false;
  for (double v : out.o) if (!std::isfinite(v)) return false;
  return std::isfinite(out.zoom) && out.zoom != 0.0;
}

namespace {
const char* reproject_invalid(const phx_reproject& r, const float* acc_from, const float* guides_from, const float* guides_to, const float* acc_to,
                              ReprojectCamera& from, ReprojectCamera& to) {
  static const char* const names[4] = {"xstride_a", "normals_offset_a", "m2_offset_a", "samples_offset_a"};
  if (const char* field = film_size_invalid(r.width, r.height)) return field;
  if (const int k = film_layout_invalid(r.xstride_a, r.normals_offset_a, r.m2_offset_a, r.samples_offset_a, 10u, (uint32_t)PHX_REPROJECT_MAX_XSTRIDE, true); k >= 0) return names[k];
  if (!r.normals_offset_a) return "normals_offset_a";
  if (r.xstride_g < 8u || r.xstride_g > (uint32_t)PHX_REPROJECT_MAX_GUIDE_XSTRIDE) return "xstride_g";
  if (r.on_device > 1u) return "on_device";
  if (r.from.film_width != r.width || r.from.film_height != r.height || !reproject_camera(r.from, from)) return "from";
  if (r.to.film_width != r.width || r.to.film_height != r.height || !reproject_camera(r.to, to)) return "to";
  if (!finite_positive(r.sigma_plane)) return "sigma_plane";
  if (!finite_positive(r.sigma_dist)) return "sigma_dist";
  if (r.max_history < 2u) return "max_history";
  if (any_reserved(r.reserved)) return "reserved";
  if (!acc_from) return "acc_from";
  if (!guides_from) return "guides_from";
  if (!guides_to) return "guides_to";
  if (!acc_to) return "acc_to";
  const uint64_t npix = (uint64_t)r.width * r.height;
  const uint64_t bytes_a = npix * r.xstride_a * sizeof(float), bytes_g = npix * r.xstride_g * sizeof(float);
  if (share_a_byte(acc_to, bytes_a, acc_from, bytes_a) || share_a_byte(acc_to, bytes_a, guides_from, bytes_g) || share_a_byte(acc_to, bytes_a, guides_to, bytes_g))
    return "acc_to";
  return nullptr;
}
}  // namespace

int reproject_check(const phx_reproject& r, const float* acc_from, const float* guides_from, const float* guides_to, const float* acc_to,
                    ReprojectCamera& from, ReprojectCamera& to, std::string& err) {
  return refusal("reproject", reproject_invalid(r, acc_from, guides_from, guides_to, acc_to, from, to), "phx_reproject", err);
}

}  // namespace phx
