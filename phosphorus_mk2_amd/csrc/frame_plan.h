// frame_plan.h — the host-only half of the frame driver: where a pixel's channels lie in the film, how many pixels a batch may hold, which
// tiles make the next batch, and the passes a batch is rendered in.
//
// Integer arithmetic on the ABI's structs and nothing else: no HIP call, no HIP header, no kernels.h, so the translation unit compiles with a
// plain host compiler (tests/native/host_frame_plan.cpp, tests/test_frame_plan.py).  The frame driver (frame_driver.cpp) asks the device how much memory is free
// (phx_device::path_budget), hands the answer in as a number of paths and drives the launches by what is decided here.
#pragma once
#include "../../include/phx_xpu.h"

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace phx {

// what the queues + state of one path in flight take (device_internal.h: PathQueues, whose static_assert holds the two to these figures)
constexpr size_t queue_bytes_per_path(bool normals) { return normals ? 192 : 176; }

// The floats of one pixel in the batch buffer and in every film sink: "primary", then "normals", "m2" and "samples" where the frame has them
// (phx_frame, phx_adaptive), and what a path in flight is counted as when the device's memory is divided into paths.
struct FilmLayout {
  uint32_t xstride = 0;         // floats per pixel
  uint32_t normals_offset = 0;  // 0 = the frame has no normals channel
  uint32_t m2_offset = 0;       // meaningful with phx_frame.moments_channel
  uint32_t samples_offset = 0;  // the last float: meaningful under adaptive sampling
  // Bytes per path: the queues' 176 / 192, and — counted once per path, as if every pixel carried one sample — the m2 channel's 3 floats of
  // the batch buffer (its other floats never were counted: 16 bytes a pixel against 176 a path) and, under adaptive sampling, the "samples"
  // float, the working copy of the pixel's row, its word of the working pixel table and its words of the two index lists.
  size_t path_bytes = 0;
  FilmLayout() = default;
  FilmLayout(const phx_frame& f, bool adaptive_on);
};

// Pixels a batch of this frame may hold: as many as can carry ALL the samples of a pass at once (pixels x samples <= budget_paths, the
// device's path budget), at least 64 k and at most 8 M.  adaptive: the device's setting, or nullptr when it is off.
uint64_t pixel_cap(uint64_t budget_paths, const phx_options& opt, const phx_adaptive* adaptive);

// Drains a tile queue in batches.  A batch takes tiles until it holds tiles_per_batch of them (0 = any number) or cap pixels; it never
// EXCEEDS the cap — the tile that would is held back and opens the next batch — except that its first tile is always taken.
struct BatchCutter {
  phx_next_tile_fn next_tile; void* tiles_user;
  uint64_t cap; uint32_t tiles_per_batch, width, height;  // width, height: the film's
  phx_tile held{}; bool have_held = false;
  // -> the next batch's tiles, in Morton order of their film position; none: the queue is drained.  A tile that is empty or not inside the
  // film: PHX_ERR_ARG, the reason in `err`.
  int next(std::vector<phx_tile>& tiles, std::string& err);
};

struct Pass { uint32_t s0, ns; bool round_end; };  // samples s0 .. s0 + ns - 1 of every pixel it carries; round_end: a decision of adaptive sampling follows

// The passes of a batch of P pixels at spp samples per pixel -> S, the most samples of a pixel any pass carries: what the queues are sized for.
// Without adaptive sampling the spp range is one "round"; with it the rounds end at e_0 = min(min_samples, spp), e_{j+1} = min(e_j + step, spp)
// (phx_adaptive), and a decision follows every round.  A round goes as one pass when P x its samples fit budget_paths (and 2^31); otherwise
// it is split into equal passes — or, with samples_in_flight set, into passes of that many samples whatever the budget.  No pass carries
// more than `limit` samples (the caller's back-off when the queues cannot be allocated; ~0u: none).
uint32_t plan_passes(uint32_t P, uint32_t spp, uint32_t samples_in_flight, uint64_t budget_paths, const phx_adaptive* adaptive, uint32_t limit,
                     std::vector<Pass>& passes);

}  // namespace phx
