// denoise_check.h — the argument check of phx_dev_denoise (phx_denoise in phx_xpu.h states the ranges).
//
// Host-only, like frame_plan.h: the ABI's struct and nothing else, so the translation unit compiles with a plain host compiler
// (tests/native/host_denoise.cpp, tests/test_denoise.py).  film_calls.cpp calls it before it touches the device; what the checks share is film_checks.h.
#pragma once
#include "../../include/phx_xpu.h"

#include <string>

namespace phx {

// PHX_OK, or PHX_ERR_ARG with the name of the first field outside its range in `err` ("film_in" / "film_out" for the pointers: null, or two
// different films that overlap)
int denoise_check(const phx_denoise& d, const float* film_in, const float* film_out, std::string& err);

}  // namespace phx
