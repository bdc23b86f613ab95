// guides_check.h — the argument checks of phx_dev_render_guides and phx_dev_denoise_guided (phx_guides and phx_denoise_guides in phx_xpu.h
// state the ranges).
//
// Host-only, like denoise_check.h: the ABI's structs and nothing else, so the translation unit compiles with a plain host compiler
// (tests/native/host_guides.cpp, tests/test_guides.py).  film_calls.cpp calls them before it touches the device.
#pragma once
#include "../../include/phx_xpu.h"

#include <string>

namespace phx {

// PHX_OK, or PHX_ERR_ARG with the name of the first field outside its range in `err`.  width x height: the scene's camera; spp: the device's
// samples_per_pixel ("samples" also when width x height x samples does not fit the kernel's 31-bit path index)
int guides_check(const phx_guides& g, uint32_t width, uint32_t height, uint32_t spp, const float* film, std::string& err);

// The guides of a denoise call whose phx_denoise `d` has passed denoise_check.  Call it only for g.flags != 0 (flags == 0 is the unguided call,
// which reads nothing else of the struct).
int denoise_guides_check(const phx_denoise& d, const phx_denoise_guides& g, std::string& err);

}  // namespace phx
