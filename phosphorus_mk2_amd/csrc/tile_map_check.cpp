// tile_map_check.cpp — see tile_map_check.h.
#include "tile_map_check.h"
#include "film_checks.h"

namespace phx {

namespace {
const char* tile_map_invalid(const phx_tile_map& m, const float* acc, const phx_tile_record* records) {
  static const char* const names[4] = {"xstride", "normals_offset", "m2_offset", "samples_offset"};  // (no normals are read: index 1 never comes back)
  if (const char* field = film_size_invalid(m.width, m.height)) return field;
  if (const int k = film_layout_invalid(m.xstride, 0u, m.m2_offset, m.samples_offset, 7u, (uint32_t)PHX_TILE_MAP_MAX_XSTRIDE, true); k >= 0) return names[k];
  if (m.tile_width < (uint32_t)PHX_TILE_MAP_MIN_TILE || m.tile_width > (uint32_t)PHX_TILE_MAP_MAX_TILE) return "tile_width";
  if (m.tile_height < (uint32_t)PHX_TILE_MAP_MIN_TILE || m.tile_height > (uint32_t)PHX_TILE_MAP_MAX_TILE) return "tile_height";
  if (m.on_device > 2u) return "on_device";
  if (!finite_nonneg(m.tau)) return "tau";
  if (!finite_nonneg(m.floor)) return "floor";
  if (any_reserved(m.reserved)) return "reserved";
  if (!acc) return "acc";
  if (!records) return "records";
  const uint64_t tiles = (uint64_t)tile_map_tiles(m.width, m.tile_width) * tile_map_tiles(m.height, m.tile_height);
  if (m.on_device != 2u && share_a_byte(acc, (uint64_t)m.width * m.height * m.xstride * sizeof(float), records, tiles * sizeof(phx_tile_record))) return "records";
  return nullptr;
}
}  // namespace

int tile_map_check(const phx_tile_map& m, const float* acc, const phx_tile_record* records, std::string& err) {
  return refusal("tile_map", tile_map_invalid(m, acc, records), "phx_tile_map", err);
}

}  // namespace phx
