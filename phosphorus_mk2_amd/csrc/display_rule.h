// display_rule.h — the display pass's rule (phx_display in phx_xpu.h states it operation by operation) as functions over phx_math.h:
// a pixel's histogram bin, the exposure from the 256 counts, and a pixel's encode.  ONE text: the kernels of display.hip call these, and a plain
// host compile (tests/native/host_display.cpp) calls them for the tests, which hold both to a numpy model bit for bit.
// Integer operations, fp32 in the order written (the files that include this are compiled without contraction), and powf_.
#pragma once
#include "../../include/phx_xpu.h"  // PHX_TONE_*
#include "phx_math.h"

namespace phx {

enum { DISPLAY_BINS = 256, DISPLAY_BIN_INVALID = 256, DISPLAY_BIN_UNLIT = 257, DISPLAY_COUNTS = 258 };

PHX_HD uint32_t display_bits(float f) { union { float f; uint32_t u; } c; c.f = f; return c.u; }
PHX_HD bool display_finite(float f) { return (display_bits(f) & 0x7f800000u) != 0x7f800000u; }

// which of the 258 counts a pixel adds one to: its bin 0 .. 255, DISPLAY_BIN_INVALID or DISPLAY_BIN_UNLIT
PHX_HD uint32_t display_bin(float r, float g, float b) {
  if (!(display_finite(r) && display_finite(g) && display_finite(b))) return DISPLAY_BIN_INVALID;
  const float Y = (float)((0.2126 * (double)r + 0.7152 * (double)g) + 0.0722 * (double)b);
  if (Y <= 0.0f) return DISPLAY_BIN_UNLIT;
  const int32_t k = (int32_t)(display_bits(Y) >> 20) - 888;
  return (uint32_t)(k < 0 ? 0 : k > 255 ? 255 : k);
}

struct display_exposure_t { float scale; uint32_t from_histogram; };
// the exposure from the bins h[0 .. 255]; N: their sum
PHX_HD display_exposure_t display_exposure(const uint64_t* h, uint64_t N, float fallback, float key, uint32_t low_q16, uint32_t high_q16, float min_scale,
                                           float max_scale) {
  if (N == 0u) return display_exposure_t{fallback, 0u};
  const uint64_t c_lo = (N * low_q16) >> 16, c_hi = (N * high_q16 + 65535u) >> 16;
  uint64_t C = 0u, W = 0u, S = 0u;
  for (uint32_t k = 0; k < (uint32_t)DISPLAY_BINS; ++k) {
    const uint64_t lo = C > c_lo ? C : c_lo, hi = C + h[k] < c_hi ? C + h[k] : c_hi;
    if (hi > lo) { W += hi - lo; S += (hi - lo) * (2u * k + 1u); }
    C += h[k];
  }
  const float p = (float)((double)S / (double)(16u * W) - 16.0);
  const float Ybar = powf_(2.0f, p);
  return display_exposure_t{fminf(fmaxf(key / Ybar, min_scale), max_scale), 1u};
}

// the dither's d at pixel (x, y): (B[y & 3][x & 3] + 0.5f) / 16.0f, the matrix packed a nibble an entry, row 0 lowest
PHX_HD float display_dither(uint32_t x, uint32_t y) {
  const uint64_t B = 0x5d7f'91b3'6e4c'a280ull;
  return ((float)(uint32_t)(B >> (16u * (y & 3u) + 4u * (x & 3u)) & 15u) + 0.5f) / 16.0f;
}

// one colour's code 0 .. 255
PHX_HD uint32_t display_code(float v, float scale, uint32_t tone, float white, float d) {
  float x = scale * v;
  if (!(x > 0.0f)) x = 0.0f;
  x = fminf(x, 65536.0f);
  float t = x;
  if (tone == (uint32_t)PHX_TONE_REINHARD) t = (x * (1.0f + x / (white * white))) / (1.0f + x);
  else if (tone == (uint32_t)PHX_TONE_ACES) t = (x * (2.51f * x + 0.03f)) / (x * (2.43f * x + 0.59f) + 0.14f);
  t = fminf(t, 1.0f);
  const float e = t <= 0.0031308f ? 12.92f * t : 1.055f * powf_(t, 1.0f / 2.4f) - 0.055f;
  const float q = 255.0f * e + d;
  return (uint32_t)(uint8_t)(int)q;
}

// a pixel's 32-bit word: bytes R, G, B, 255 in memory order
PHX_HD uint32_t display_pixel(float r, float g, float b, float scale, uint32_t tone, float white, float d) {
  return display_code(r, scale, tone, white, d) | display_code(g, scale, tone, white, d) << 8 | display_code(b, scale, tone, white, d) << 16 | 0xff000000u;
}

}  // namespace phx
