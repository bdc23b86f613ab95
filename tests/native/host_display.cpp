// host_display.cpp — the display pass on the host for tests/test_display.py, compiled with a plain host compiler: the argument check of
// phx_dev_film_display (csrc/display_check.cpp) and the rule's functions (csrc/display_rule.h, the text the kernels of display.hip run) behind a
// C interface, and hd_display, the whole call as loops over those functions.  With -DHOST_DISPLAY_MAIN it is a stand-alone program instead,
// for a run under AddressSanitizer / UBSan: it runs the cases listed in main() and prints, per line, the case and the answer.
#include "../../phosphorus_mk2_amd/csrc/display_check.h"
#include "../../phosphorus_mk2_amd/csrc/display_rule.h"

#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

using namespace phx;

extern "C" {

// -> the status; err: the refusal's text (empty when accepted).  The film and the image are addresses only: nothing is read through them.
int hd_check(const phx_display* p, const float* film, const uint8_t* image, char* err, uint32_t err_room) {
  std::string why;
  const int rc = display_check(*p, film, image, why);
  if (err && err_room) { std::strncpy(err, why.c_str(), err_room - 1); err[err_room - 1] = 0; }
  return rc;
}

uint32_t hd_sizeof(void) { return (uint32_t)sizeof(phx_display); }
uint32_t hd_sizeof_summary(void) { return (uint32_t)sizeof(phx_display_summary); }

// which count each of n pixels (3 floats each) adds to: 0 .. 255 a bin, 256 invalid, 257 unlit
void hd_bins(uint64_t n, const float* rgb, uint32_t* out) {
  for (uint64_t i = 0; i < n; ++i) out[i] = display_bin(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2]);
}

// the exposure rule on 256 counts
void hd_exposure(const uint64_t* h, float fallback, float key, uint32_t low_q16, uint32_t high_q16, float min_scale, float max_scale, float* scale,
                 uint32_t* from_histogram) {
  uint64_t N = 0;
  for (int k = 0; k < 256; ++k) N += h[k];
  const display_exposure_t e = display_exposure(h, N, fallback, key, low_q16, high_q16, min_scale, max_scale);
  *scale = e.scale; *from_histogram = e.from_histogram;
}

// the codes of n values under one scale and one d
void hd_codes(uint64_t n, const float* v, float scale, uint32_t tone, float white, float d, uint8_t* out) {
  for (uint64_t i = 0; i < n; ++i) out[i] = (uint8_t)display_code(v[i], scale, tone, white, d);
}

// the call on host memory (on_device is not read): the check, the histogram when the call makes one, the exposure, the encode
int hd_display(const phx_display* p, const float* film, uint8_t* image, phx_display_summary* summary, uint64_t* histogram, char* err, uint32_t err_room) {
  if (const int rc = hd_check(p, film, image, err, err_room)) return rc;
  const uint64_t npix = (uint64_t)p->width * p->height;
  float scale = p->scale;
  if ((p->flags & PHX_DISPLAY_AUTO_EXPOSURE) || summary || histogram) {
    uint64_t counts[DISPLAY_COUNTS] = {};
    for (uint64_t i = 0; i < npix; ++i) { const float* v = film + i * p->xstride; ++counts[display_bin(v[0], v[1], v[2])]; }
    uint64_t N = 0;
    for (int k = 0; k < 256; ++k) N += counts[k];
    display_exposure_t e{p->scale, 0u};
    if (p->flags & PHX_DISPLAY_AUTO_EXPOSURE) e = display_exposure(counts, N, p->scale, p->key, p->low_q16, p->high_q16, p->min_scale, p->max_scale);
    scale = e.scale;
    if (histogram) std::memcpy(histogram, counts, 256 * sizeof(uint64_t));
    if (summary) {
      summary->pixels = npix; summary->invalid = counts[DISPLAY_BIN_INVALID]; summary->unlit = counts[DISPLAY_BIN_UNLIT]; summary->counted = N;
      summary->scale = scale; summary->from_histogram = e.from_histogram;
    }
  }
  const uint64_t pitch = display_pitch(*p);
  for (uint32_t y = 0; y < p->height; ++y)
    for (uint32_t x = 0; x < p->width; ++x) {
      const float* v = film + ((uint64_t)y * p->width + x) * p->xstride;
      const float d = (p->flags & PHX_DISPLAY_DITHER) ? display_dither(x, y) : 0.5f;
      const uint32_t word = display_pixel(v[0], v[1], v[2], scale, p->tone, p->white, d);
      uint8_t* out = image + y * pitch + 4ull * x;
      out[0] = (uint8_t)word; out[1] = (uint8_t)(word >> 8); out[2] = (uint8_t)(word >> 16); out[3] = (uint8_t)(word >> 24);
    }
  return PHX_OK;
}

}  // extern "C"

#ifdef HOST_DISPLAY_MAIN
namespace {
phx_display good() {
  phx_display p{};
  p.width = 7; p.height = 5; p.xstride = 8; p.image_pitch = 0; p.on_device = 0;
  p.flags = PHX_DISPLAY_DITHER | PHX_DISPLAY_AUTO_EXPOSURE; p.tone = PHX_TONE_REINHARD;
  p.scale = 1.0f; p.white = 4.0f; p.key = 0.18f; p.low_q16 = 32768; p.high_q16 = 62259; p.min_scale = 1.0f / 4096.0f; p.max_scale = 4096.0f;
  return p;
}
void show(const char* name, const phx_display& p, const float* film, const uint8_t* image) {
  char err[128];
  const int rc = hd_check(&p, film, image, err, sizeof err);
  std::printf("%s %d %s\n", name, rc, err);
}
}  // namespace

int main() {
  static float film[7 * 5 * 8];
  alignas(4) static uint8_t image[5 * 32];
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  phx_display p = good();
  show("good", p, film, image);
  show("null-film", p, nullptr, image);
  show("null-image", p, film, nullptr);
  show("misaligned", p, film, image + 1);
  show("overlap", p, film, reinterpret_cast<const uint8_t*>(film + 7 * 5 * 8 - 1));
  p = good(); p.width = 0; show("width", p, film, image);
  p = good(); p.height = 65537; show("height", p, film, image);
  p = good(); p.xstride = 2; show("xstride", p, film, image);
  p = good(); p.image_pitch = 30; show("pitch", p, film, image);
  p = good(); p.on_device = 3; show("on-device", p, film, image);
  p = good(); p.flags = 4; show("flags", p, film, image);
  p = good(); p.tone = 3; show("tone", p, film, image);
  p = good(); p.scale = nan; show("scale", p, film, image);
  p = good(); p.white = 0.0f; show("white", p, film, image);
  p = good(); p.key = inf; show("key", p, film, image);
  p = good(); p.low_q16 = p.high_q16; show("low", p, film, image);
  p = good(); p.high_q16 = 65537; show("high", p, film, image);
  p = good(); p.min_scale = -1.0f; show("min-scale", p, film, image);
  p = good(); p.max_scale = p.min_scale / 2.0f; show("max-scale", p, film, image);
  p = good(); p.reserved[1] = 1; show("reserved", p, film, image);

  // the whole call on a film with every kind of pixel, a padded pitch, and both exposure modes
  const float special[] = {nan, inf, -inf, -1.0f, 0.0f, -0.0f, 1e-30f, 1e30f, 3.4e38f, 1.0f, 0.18f, 65536.0f};
  for (int i = 0; i < 7 * 5; ++i) for (int c = 0; c < 8; ++c) film[8 * i + c] = c < 3 ? special[(i + 5 * c) % 12] : nan;
  for (uint32_t tone = 0; tone < 3; ++tone)
    for (uint32_t flags = 0; flags < 4; ++flags) {
      p = good(); p.tone = tone; p.flags = flags; p.image_pitch = 32;
      std::memset(image, 0x5a, sizeof image);
      phx_display_summary s; uint64_t h[256]; char err[128];
      const int rc = hd_display(&p, film, image, &s, h, err, sizeof err);
      unsigned sum = 0, pad = 0;
      for (int y = 0; y < 5; ++y) { for (int b = 0; b < 28; ++b) sum += image[32 * y + b]; for (int b = 28; b < 32 && y < 4; ++b) pad += image[32 * y + b] != 0x5a; }
      std::printf("call-%u-%u %d sum %u pad %u pixels %llu invalid %llu unlit %llu counted %llu scale %.9g from %u\n", tone, flags, rc, sum, pad,
                  (unsigned long long)s.pixels, (unsigned long long)s.invalid, (unsigned long long)s.unlit, (unsigned long long)s.counted, (double)s.scale, s.from_histogram);
    }
  // the exposure on the extreme histograms
  uint64_t h[256] = {};
  float scale; uint32_t from;
  hd_exposure(h, 3.0f, 0.18f, 0, 65536, 1e-4f, 1e4f, &scale, &from); std::printf("empty 0 %.9g %u\n", (double)scale, from);
  h[255] = 1ull << 32; hd_exposure(h, 3.0f, 0.18f, 0, 65536, 1e-30f, 1e30f, &scale, &from); std::printf("top 0 %.9g %u\n", (double)scale, from);
  h[255] = 0; h[0] = 1; hd_exposure(h, 3.0f, 0.18f, 65535, 65536, 1e-30f, 1e30f, &scale, &from); std::printf("bottom 0 %.9g %u\n", (double)scale, from);
  return 0;
}
#endif
