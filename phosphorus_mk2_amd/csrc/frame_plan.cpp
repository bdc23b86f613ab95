// frame_plan.cpp — see frame_plan.h.
#include "frame_plan.h"

#include <algorithm>

namespace phx {

FilmLayout::FilmLayout(const phx_frame& f, bool adaptive_on) {
  const uint32_t normals = f.normals_channel ? 3u : 0u;
  xstride = f.primary_components + normals + (f.moments_channel ? 3u : 0u) + (adaptive_on ? 1u : 0u);
  normals_offset = f.normals_channel ? f.primary_components : 0;
  m2_offset = f.primary_components + normals;
  samples_offset = xstride - 1u;
  path_bytes = queue_bytes_per_path(f.normals_channel != 0) + (f.moments_channel ? 3 * sizeof(float) : 0) +
               (adaptive_on ? sizeof(float) + xstride * sizeof(float) + 3 * sizeof(uint32_t) : 0);
}

// A batch holds as many pixels as can carry ALL their samples in one pass (P x spp <= the path budget, at most 8 M pixels): path ids are
// pixel-major, so a pass with every sample of a pixel keeps the 64 lanes of a wave — and the 256 rays of a camera-ray packet — on ONE pixel.
// (Round 3 took 8 M pixels whatever the spp: the 3840x2160, 256-spp frame of BASELINE config 4 went through as 8 passes of 32 samples; as 8
// batches of 256 samples it is 6.8 % faster — camera rays 67.9 -> 36.0 ms, k_trace -4 %: profiles/r04_v_batch_probe.log.)
uint64_t pixel_cap(uint64_t budget_paths, const phx_options& opt, const phx_adaptive* adaptive) {
  // (divided by the samples a pass will really carry: with an explicit samples_in_flight only P x S paths are ever in flight; under adaptive
  // sampling a pass carries at most a round, and the longest round has max(min_samples, step) samples)
  const uint32_t frame_samples = adaptive ? std::min(opt.samples_per_pixel, std::max(adaptive->min_samples, adaptive->step)) : opt.samples_per_pixel;
  const uint32_t pass_samples = std::max(1u, std::min(opt.samples_per_pixel, opt.samples_in_flight ? opt.samples_in_flight : frame_samples));
  return std::min<uint64_t>(8u << 20, std::max<uint64_t>(budget_paths / pass_samples, 64u << 10));
}

// A batch never EXCEEDS the cap: its paths then fit the queues the first full batch allocated, whatever mix of whole and edge tiles it
// holds.  (Until round 5 a batch overshot by up to one tile; a 4 096-spp batch that grew from 131 072 to 131 584 pixels re-allocated 86 GB
// of queues — 2.6 s of hipFree — in the middle of a frame: profiles/r05_f_c5_batch_probe.log.)
int BatchCutter::next(std::vector<phx_tile>& tiles, std::string& err) {
  tiles.clear();
  uint64_t px = 0;
  while ((tiles_per_batch == 0 || tiles.size() < tiles_per_batch) && px < cap) {
    phx_tile t;
    if (have_held) { t = held; have_held = false; }
    else if (!next_tile(tiles_user, &t)) break;
    if (t.w == 0 || t.h == 0 || (uint64_t)t.x + t.w > width || (uint64_t)t.y + t.h > height) { err = "tile outside the film"; return PHX_ERR_ARG; }
    if (!tiles.empty() && px + (uint64_t)t.w * t.h > cap) { held = t; have_held = true; break; }
    tiles.push_back(t); px += (uint64_t)t.w * t.h;
  }
  // the batch's tiles in Morton order of their film position: path ids are pixel-major, so the batch's queue — and with it each
  // XCD's eighth of it (k_trace's segments) — covers a compact block of the film instead of a row of tiles 3840 pixels wide
  // (1 M soup + 2.3 % against queue order, 100 k soup and config 4 unchanged, films bit-identical: profiles/r04_y_morton.log)
  auto spread = [](uint32_t v) { v &= 0xffffu; v = (v | (v << 8)) & 0x00ff00ffu; v = (v | (v << 4)) & 0x0f0f0f0fu; v = (v | (v << 2)) & 0x33333333u; v = (v | (v << 1)) & 0x55555555u; return v; };
  auto key = [&](const phx_tile& t) { return spread(t.x >> 5) | (spread(t.y >> 5) << 1); };
  std::stable_sort(tiles.begin(), tiles.end(), [&](const phx_tile& a, const phx_tile& b) { return key(a) < key(b); });
  return PHX_OK;
}

uint32_t plan_passes(uint32_t P, uint32_t spp, uint32_t samples_in_flight, uint64_t budget_paths, const phx_adaptive* adaptive, uint32_t limit,
                     std::vector<Pass>& passes) {
  // paths in flight: the device's budget (up to 512 M paths).  Deep bounces keep only a few percent of the paths alive, so many paths per
  // pass are what keeps late launches full; a batch that cannot carry all its samples at once splits the spp range into equal passes.
  // (r: the samples to split — the frame's spp, or one round of adaptive sampling)
  auto pick_samples = [&](uint32_t r) -> uint32_t {
    if (samples_in_flight) return samples_in_flight;
    const uint64_t budget = std::max<uint64_t>(budget_paths, P);
    // (no slack: the frame driver never hands over a batch above its pixel cap = budget / samples of a pass, so P x spp <= budget holds for
    // every batch it sized; a caller's own tile list — or the cap's floor of 64 k pixels — may exceed it, and then the spp range is split)
    const uint32_t smax = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(budget / P, 0x7ffffff0ull / P));
    const uint32_t npasses = (r + smax - 1) / smax;
    return (r + npasses - 1) / npasses;
  };
  passes.clear();
  uint32_t S = 0;
  for (uint32_t begin = 0; begin < spp;) {
    const uint32_t end = !adaptive ? spp : (uint32_t)std::min<uint64_t>(spp, begin ? (uint64_t)begin + adaptive->step : adaptive->min_samples);
    const uint32_t Sr = std::min({pick_samples(end - begin), end - begin, limit});
    for (uint32_t s0 = begin; s0 < end; s0 += Sr) passes.push_back(Pass{s0, std::min(Sr, end - s0), adaptive && s0 + Sr >= end});
    S = std::max(S, Sr);
    begin = end;
  }
  return S;
}

}  // namespace phx
