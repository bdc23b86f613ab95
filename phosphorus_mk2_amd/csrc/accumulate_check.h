// accumulate_check.h — the argument check of phx_dev_film_accumulate (phx_accumulate in phx_xpu.h states the ranges).
//
// Host-only, like denoise_check.h: the ABI's struct and nothing else, so the translation unit compiles with a plain host compiler
// (tests/native/host_accumulate.cpp, tests/test_accumulate.py).  film_calls.cpp calls it before it touches the device.
#pragma once
#include "../../include/phx_xpu.h"

#include <string>

namespace phx {

// the largest xstride of either film: the check refuses more, and the kernel's LDS is sized by it (accumulate.hip)
enum { PHX_ACCUMULATE_MAX_XSTRIDE = 24 };

// PHX_OK, or PHX_ERR_ARG with the name of the first field outside its range in `err` ("acc" / "frame_film" for the pointers: null, or two
// films that share a float)
int accumulate_check(const phx_accumulate& a, const float* acc, const float* frame_film, std::string& err);

}  // namespace phx
