// tile_map_host.cpp — the argument check of phx_dev_film_tile_map (csrc/tile_map_check.cpp) behind a C interface for tests/test_tile_map.py,
// compiled with a plain host compiler.  With -DTILE_MAP_HOST_MAIN it is a stand-alone program instead, for a run under AddressSanitizer /
// UBSan: it checks the cases listed in main() and prints, per line, the case and the answer.
#include "../../phosphorus_mk2_amd/csrc/tile_map_check.h"

#include <cstddef>
#include <cstdio>
#include <cstring>
#include <limits>

using namespace phx;

extern "C" {

// -> the status; err: the refusal's text (empty when accepted).  The film and the records are addresses only: nothing is read through them.
int tm_check(const phx_tile_map* m, const float* acc, const phx_tile_record* records, char* err, uint32_t err_room) {
  std::string why;
  const int rc = tile_map_check(*m, acc, records, why);
  if (err && err_room) { std::strncpy(err, why.c_str(), err_room - 1); err[err_room - 1] = 0; }
  return rc;
}

uint32_t tm_sizeof(void) { return (uint32_t)sizeof(phx_tile_map); }
uint32_t tm_sizeof_record(void) { return (uint32_t)sizeof(phx_tile_record); }
uint32_t tm_sizeof_summary(void) { return (uint32_t)sizeof(phx_tile_map_summary); }
// the offsets of a record's fields, in their order: tile, invalid, starved, converged, worst, samples
void tm_record_offsets(uint32_t* out) {
  out[0] = (uint32_t)offsetof(phx_tile_record, tile); out[1] = (uint32_t)offsetof(phx_tile_record, invalid); out[2] = (uint32_t)offsetof(phx_tile_record, starved);
  out[3] = (uint32_t)offsetof(phx_tile_record, converged); out[4] = (uint32_t)offsetof(phx_tile_record, worst); out[5] = (uint32_t)offsetof(phx_tile_record, samples);
}
uint32_t tm_tiles(uint32_t extent, uint32_t tile) { return tile_map_tiles(extent, tile); }

}  // extern "C"

#ifdef TILE_MAP_HOST_MAIN
namespace {
phx_tile_map good() {
  phx_tile_map m{};
  m.width = 64; m.height = 48; m.xstride = 11; m.m2_offset = 7; m.samples_offset = 10;
  m.tile_width = 32; m.tile_height = 16; m.on_device = 0; m.tau = 0.05f; m.floor = 0.01f;
  return m;
}
void show(const char* name, const phx_tile_map& m, const float* acc, const phx_tile_record* records) {
  char err[128];
  const int rc = tm_check(&m, acc, records, err, sizeof err);
  std::printf("%s %d %s\n", name, rc, err);
}
}  // namespace

int main() {
  static float film[64 * 48 * 11];
  static phx_tile_record records[2 * 3];
  phx_tile_map m = good();
  show("good", m, film, records);
  show("null-acc", m, nullptr, records);
  show("null-records", m, film, nullptr);
  show("records-in-film", m, film, reinterpret_cast<phx_tile_record*>(film + 8));
  m = good(); m.on_device = 2; show("records-in-film-other-space", m, film, reinterpret_cast<phx_tile_record*>(film + 8));
  m = good(); m.width = 0; show("width", m, film, records);
  m = good(); m.height = 65537; show("height", m, film, records);
  m = good(); m.xstride = 6; show("xstride-low", m, film, records);
  m = good(); m.xstride = 25; show("xstride-high", m, film, records);
  m = good(); m.m2_offset = 0; show("no-m2", m, film, records);
  m = good(); m.m2_offset = 0xfffffffeu; show("m2-wrap", m, film, records);
  m = good(); m.samples_offset = 0; show("no-samples", m, film, records);
  m = good(); m.samples_offset = 8; show("samples-in-m2", m, film, records);
  m = good(); m.tile_width = 3; show("tile-width-low", m, film, records);
  m = good(); m.tile_width = 1025; show("tile-width-high", m, film, records);
  m = good(); m.tile_height = 0; show("tile-height-low", m, film, records);
  m = good(); m.tile_height = 1025; show("tile-height-high", m, film, records);
  m = good(); m.on_device = 3; show("on-device", m, film, records);
  m = good(); m.tau = std::numeric_limits<float>::quiet_NaN(); show("tau-nan", m, film, records);
  m = good(); m.floor = -1.0f; show("floor", m, film, records);
  m = good(); m.reserved[3] = 1; show("reserved", m, film, records);
  return 0;
}
#endif
