// display_check.h — the argument check of phx_dev_film_display (phx_display in phx_xpu.h states the ranges).
//
// Host-only, like accumulate_check.h: the ABI's struct and nothing else, so the translation unit compiles with a plain host compiler
// (tests/native/host_display.cpp, tests/test_display.py).  film_calls.cpp calls it before it touches the device.
#pragma once
#include "../../include/phx_xpu.h"

#include <string>

namespace phx {

// the largest xstride of the film: the check refuses more
enum { PHX_DISPLAY_MAX_XSTRIDE = 24 };
// the most workgroups k_display_histogram is launched with, whatever the film's size (display.hip sizes the grid by the device's compute
// units below this cap): every workgroup ends with up to 258 global atomics, and their number must not grow with the film
enum { PHX_DISPLAY_HIST_MAX_GROUPS = 2048 };

// PHX_OK, or PHX_ERR_ARG with the name of the first field outside its range in `err` ("film" / "image" for the pointers: null, an image
// that is not 4-byte aligned, or a film and an image that share a byte)
int display_check(const phx_display& p, const float* film, const uint8_t* image, std::string& err);

// bytes per image row (image_pitch, or 4 * width for 0) and the bytes from the image's first to behind its last written one
inline uint64_t display_pitch(const phx_display& p) { return p.image_pitch ? p.image_pitch : 4ull * p.width; }
inline uint64_t display_image_bytes(const phx_display& p) { return (p.height - 1ull) * display_pitch(p) + 4ull * p.width; }

}  // namespace phx
