// reproject_check.h — the argument check of phx_dev_film_reproject and the host's derivation of its two cameras (phx_reproject in phx_xpu.h
// states the ranges and the derivation operation by operation).
//
// Host-only, like accumulate_check.h: the ABI's struct and nothing else, so the translation unit compiles with a plain host compiler
// (tests/native/host_reproject.cpp, tests/test_reproject.py).  film_calls.cpp calls it before it touches the device.
#pragma once
#include "../../include/phx_xpu.h"

#include <string>

namespace phx {

// the largest xstride of the accumulator films and of the guide films: the check refuses more
enum { PHX_REPROJECT_MAX_XSTRIDE = 24, PHX_REPROJECT_MAX_GUIDE_XSTRIDE = 64 };

// a camera as k_reproject reads it: the origin, the inverse I of to_world's upper 3 x 3 (row-major), zoom, ratio, W and H, all binary64
struct ReprojectCamera { double o[3], inv[9], zoom, ratio, w, h; };

// the derivation of phx_xpu.h; false for a singular or non-finite matrix, a non-finite or zero zoom or an empty film (`out` is then unspecified)
bool reproject_camera(const phx_camera& c, ReprojectCamera& out);

// PHX_OK, or PHX_ERR_ARG with the name of the first field outside its range in `err` ("from" / "to" for a camera; "acc_from", "guides_from",
// "guides_to", "acc_to" for the pointers: null, or acc_to sharing a byte with an input).  After PHX_OK `from` and `to` hold the cameras.
int reproject_check(const phx_reproject& r, const float* acc_from, const float* guides_from, const float* guides_to, const float* acc_to,
                    ReprojectCamera& from, ReprojectCamera& to, std::string& err);

}  // namespace phx
