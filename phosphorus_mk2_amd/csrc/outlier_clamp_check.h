// outlier_clamp_check.h — the argument check of phx_dev_film_outlier_clamp (phx_outlier_clamp in phx_xpu.h states the ranges and which films
// may be one another).
//
// Host-only, like reproject_check.h: the ABI's struct and nothing else, so the translation unit compiles with a plain host compiler
// (tests/native/host_outlier_clamp.cpp, tests/test_outlier_clamp.py).  film_calls.cpp calls it before it touches the device.
#pragma once
#include "../../include/phx_xpu.h"

#include <string>

namespace phx {

// the largest xstride of either film and the largest radius: the check refuses more, which bounds k_outlier_clamp's LDS (kernels.h)
enum { PHX_OUTLIER_MAX_XSTRIDE = 24, PHX_OUTLIER_MAX_RADIUS = 3 };

// PHX_OK, or PHX_ERR_ARG with the name of the first field outside its range in `err` ("film", "ref", "film_out" for the pointers: null, or
// ref overlapping film partially, or film_out overlapping film or ref partially).  After PHX_OK `ref_needs_copy` says that film_out shares
// bytes with ref (it is ref exactly, or film_out == film == ref): the call must then take its bounds from a copy of ref.
int outlier_clamp_check(const phx_outlier_clamp& c, const float* film, const float* ref, const float* film_out, bool& ref_needs_copy, std::string& err);

}  // namespace phx
