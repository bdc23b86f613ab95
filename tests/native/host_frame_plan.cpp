// host_frame_plan.cpp — the frame planner (csrc/frame_plan.cpp) behind a C interface for tests/test_frame_plan.py, compiled with a plain host
// compiler.  Adaptive sampling comes in as (min_samples, step), min_samples == 0 meaning "off".  With -DHOST_FRAME_PLAN_MAIN it is a
// stand-alone program instead, for a run under AddressSanitizer / UBSan: it plans the cases listed in main() and prints, per line, the case
// and what the planner decided; the test checks every line against its own model.
#include "../../phosphorus_mk2_amd/csrc/frame_plan.h"

#include <algorithm>
#include <cstdio>
#include <cstring>

using namespace phx;

namespace {

struct TileList { const phx_tile* tiles; uint32_t n, cursor; };
int next_of_list(void* user, phx_tile* out) {
  TileList* l = static_cast<TileList*>(user);
  if (l->cursor == l->n) return 0;
  *out = l->tiles[l->cursor++];
  return 1;
}

struct Setting {
  phx_adaptive a{}; bool on;
  Setting(uint32_t min_samples, uint32_t step) : on(min_samples != 0) { a.min_samples = min_samples; a.step = step; }
  const phx_adaptive* get() const { return on ? &a : nullptr; }
};

}  // namespace

extern "C" {

// out: xstride, normals_offset, m2_offset, samples_offset, path_bytes
void fp_layout(uint32_t primary_components, uint32_t normals, uint32_t moments, uint32_t adaptive_on, uint64_t out[5]) {
  phx_frame f{};
  f.primary_components = primary_components; f.normals_channel = normals; f.moments_channel = moments;
  const FilmLayout l(f, adaptive_on != 0);
  out[0] = l.xstride; out[1] = l.normals_offset; out[2] = l.m2_offset; out[3] = l.samples_offset; out[4] = l.path_bytes;
}

uint64_t fp_pixel_cap(uint64_t budget, uint32_t spp, uint32_t flight, uint32_t min_samples, uint32_t step) {
  phx_options opt{};
  opt.samples_per_pixel = spp; opt.samples_in_flight = flight;
  return pixel_cap(budget, opt, Setting(min_samples, step).get());
}

// -> the number of passes; the first `room` of them as (s0, ns, round_end) in out, S in *most
uint32_t fp_passes(uint32_t P, uint32_t spp, uint32_t flight, uint64_t budget, uint32_t min_samples, uint32_t step, uint32_t limit, uint32_t* out, uint32_t room,
                   uint32_t* most) {
  std::vector<Pass> passes;
  *most = plan_passes(P, spp, flight, budget, Setting(min_samples, step).get(), limit, passes);
  for (size_t i = 0; i < passes.size() && i < room; ++i) { out[3 * i] = passes[i].s0; out[3 * i + 1] = passes[i].ns; out[3 * i + 2] = passes[i].round_end; }
  return (uint32_t)passes.size();
}

// Cuts the list into batches until it is drained or a tile is refused -> the status.  out: the batches' tiles one after the other (room for n),
// sizes: the tiles of each batch (room for n), *num_batches how many; err: the refusal's text.
int fp_cut(const phx_tile* tiles, uint32_t n, uint64_t cap, uint32_t tiles_per_batch, uint32_t width, uint32_t height, phx_tile* out, uint32_t* sizes,
           uint32_t* num_batches, char* err, uint32_t err_room) {
  TileList list{tiles, n, 0};
  BatchCutter cutter{next_of_list, &list, cap, tiles_per_batch, width, height};
  std::vector<phx_tile> batch; std::string why;
  uint32_t done = 0;
  *num_batches = 0;
  if (err_room) err[0] = 0;
  for (;;) {
    if (const int rc = cutter.next(batch, why)) { std::snprintf(err, err_room, "%s", why.c_str()); return rc; }
    if (batch.empty()) return PHX_OK;
    if (done + batch.size() > n) { std::snprintf(err, err_room, "more tiles out than in"); return -1; }
    std::memcpy(static_cast<void*>(out + done), batch.data(), batch.size() * sizeof(phx_tile));
    done += (uint32_t)batch.size();
    sizes[(*num_batches)++] = (uint32_t)batch.size();
  }
}

}  // extern "C"

#ifdef HOST_FRAME_PLAN_MAIN
namespace {

constexpr uint64_t M = 1ull << 20;

void layout(uint32_t pc, uint32_t normals, uint32_t moments, uint32_t adaptive) {
  uint64_t o[5];
  fp_layout(pc, normals, moments, adaptive, o);
  std::printf("layout %u %u %u %u :", pc, normals, moments, adaptive);
  for (uint64_t v : o) std::printf(" %llu", (unsigned long long)v);
  std::printf("\n");
}

void cap(uint64_t budget, uint32_t spp, uint32_t flight, uint32_t min_samples, uint32_t step) {
  std::printf("cap %llu %u %u %u %u : %llu\n", (unsigned long long)budget, spp, flight, min_samples, step,
              (unsigned long long)fp_pixel_cap(budget, spp, flight, min_samples, step));
}

void passes(uint32_t P, uint32_t spp, uint32_t flight, uint64_t budget, uint32_t min_samples, uint32_t step, uint32_t limit) {
  uint32_t S = 0;
  const uint32_t n = fp_passes(P, spp, flight, budget, min_samples, step, limit, nullptr, 0, &S);
  std::vector<uint32_t> out(3 * (size_t)n);  // exactly sized
  fp_passes(P, spp, flight, budget, min_samples, step, limit, out.data(), n, &S);
  std::printf("passes %u %u %u %llu %u %u %u : %u", P, spp, flight, (unsigned long long)budget, min_samples, step, limit, S);
  for (uint32_t v : out) std::printf(" %u", v);
  std::printf("\n");
}

// the film's 32-pixel tiles in row order, as phx_tiles_make lays them out for one rank, or 8-wide strips over its columns (the last one overlaps)
std::vector<phx_tile> grid(uint32_t W, uint32_t H, uint32_t ts) {
  std::vector<phx_tile> t;
  for (uint32_t y = 0; y < H; y += ts)
    for (uint32_t x = 0; x < W; x += ts) t.push_back(phx_tile{x, y, std::min(ts, W - x), std::min(ts, H - y)});
  return t;
}
std::vector<phx_tile> strips(uint32_t W, uint32_t H) {
  std::vector<phx_tile> t;
  for (uint32_t x = 0; x + 8 <= W; x += 8) t.push_back(phx_tile{x, 0, 8, H});
  if (W % 8) t.push_back(phx_tile{W - 8, 0, 8, H});
  return t;
}

void cut(const char* name, std::vector<phx_tile> tiles, uint64_t cap, uint32_t tiles_per_batch, uint32_t W, uint32_t H) {
  const uint32_t n = (uint32_t)tiles.size();
  std::vector<phx_tile> in(tiles.begin(), tiles.end()), out(n);  // exactly sized
  std::vector<uint32_t> sizes(n);
  uint32_t nb = 0; char err[64];
  const int rc = fp_cut(in.data(), n, cap, tiles_per_batch, W, H, out.data(), sizes.data(), &nb, err, sizeof(err));
  std::printf("cut %s %llu %u %u %u : %d", name, (unsigned long long)cap, tiles_per_batch, W, H, rc);
  if (rc) { std::printf(" %s\n", err); return; }
  for (uint32_t b = 0, k = 0; b < nb; ++b) {
    std::printf(" |");
    for (uint32_t i = 0; i < sizes[b]; ++i, ++k) std::printf(" %u,%u,%u,%u", out[k].x, out[k].y, out[k].w, out[k].h);
  }
  std::printf("\n");
}

}  // namespace

int main() {
  for (uint32_t pc : {3u, 4u})
    for (uint32_t normals : {0u, 1u}) {
      layout(pc, normals, 0, 0); layout(pc, normals, 1, 0); layout(pc, normals, 1, 1);
    }
  cap(512 * M, 16, 0, 0, 0); cap(512 * M, 256, 0, 0, 0); cap(512 * M, 4096, 0, 0, 0); cap(512 * M, 65536, 0, 0, 0);
  cap(512 * M, 256, 32, 0, 0); cap(512 * M, 256, 0, 16, 16); cap(512 * M, 256, 0, 300, 16);
  const uint32_t none = ~0u;
  passes(1024, 16, 0, 10000, 0, 0, none); passes(1024, 20, 0, 10000, 0, 0, none); passes(1024, 256, 0, 10000, 0, 0, none);
  passes(1024, 16, 0, 10000, 0, 0, 4); passes(1024, 5, 0, 10, 0, 0, none);
  passes(1024, 8, 3, 10000, 0, 0, none); passes(1024, 2, 3, 10000, 0, 0, none); passes(1024, 8, 3, 10, 0, 0, none);
  passes(3u << 20, 4096, 0, 1ull << 62, 0, 0, none);
  passes(1024, 16, 0, 1ull << 40, 4, 5, none); passes(1024, 16, 3, 1ull << 40, 4, 5, none);
  passes(1024, 16, 0, 1ull << 40, 16, 5, none); passes(1024, 16, 0, 1ull << 40, 40, 5, none); passes(1024, 16, 0, 1ull << 40, 4, none, none);
  passes(1024, 16, 0, 10000, 4, 5, 2);
  cut("grid", grid(320, 200, 32), 65536, 0, 320, 200); cut("grid", grid(320, 200, 32), 4096, 0, 320, 200);
  cut("grid", grid(320, 200, 32), 65536, 3, 320, 200); cut("grid", grid(320, 200, 32), 100, 0, 320, 200);
  cut("strips", strips(67, 5), 65536, 0, 67, 5); cut("strips", strips(67, 5), 80, 0, 67, 5);
  { auto t = grid(320, 200, 32); t.back().w = 0; cut("empty", t, 65536, 0, 320, 200); }
  { auto t = grid(320, 200, 32); t.back().x += 1; cut("right", t, 65536, 0, 320, 200); }
  { auto t = grid(320, 200, 32); t.back().y += 1; cut("bottom", t, 65536, 0, 320, 200); }
  return 0;
}
#endif
