// tile_map_check.h — the argument check of phx_dev_film_tile_map (phx_tile_map in phx_xpu.h states the ranges) and the grid's size.
//
// Host-only, like accumulate_check.h: the ABI's struct and nothing else, so the translation unit compiles with a plain host compiler
// (tests/native/tile_map_host.cpp, tests/test_tile_map.py).  film_calls.cpp calls it before it touches the device.
#pragma once
#include "../../include/phx_xpu.h"

#include <string>

namespace phx {

// the bounds of a tile's side and of the film's xstride: the check refuses what lies outside
enum { PHX_TILE_MAP_MIN_TILE = 4, PHX_TILE_MAP_MAX_TILE = 1024, PHX_TILE_MAP_MAX_XSTRIDE = 24 };

// how many tiles of `tile` pixels cover `extent` pixels (tile >= 1)
inline uint32_t tile_map_tiles(uint32_t extent, uint32_t tile) { return (extent + tile - 1u) / tile; }

// PHX_OK, or PHX_ERR_ARG with the name of the first field outside its range in `err` ("acc" / "records" for the pointers: null, or, where
// both lie in one memory space, records sharing a byte with the film)
int tile_map_check(const phx_tile_map& m, const float* acc, const phx_tile_record* records, std::string& err);

}  // namespace phx
