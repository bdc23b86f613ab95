// display.hip — the display pass: a film's linear radiance to an RGBA8 sRGB image (phx_display in phx_xpu.h states the rule operation by
// operation).  No counterpart in the reference, which writes linear floats to a file.  A pass of its own: no frame launches these.
//
//   k_display_histogram   film -> 258 counts (the 256 luminance bins, invalid, unlit) in PHX_DISPLAY_SLOTS copies
//   k_display_exposure    the copies -> DisplayBlock: the histogram, the four counters, the scale (the exposure rule, one thread)
//   k_display_encode      film, the block's scale -> image, one 32-bit store a pixel
//
// The arithmetic is display_rule.h's, the one text the host tests compile too.  Both film kernels read a pixel's three floats with direct
// loads, a lane a pixel: lanes lie xstride floats apart, so the three loads of a wave touch the same 128-byte lines one after the other and
// every line of the film comes over the bus once, as it would through an LDS-staged span (accumulate.hip), without the barrier and the LDS.
// The histogram's grid does not grow with the film: a workgroup strides over spans, counts in LDS and ends with at most 258 global atomics
// (k_accumulate's 32 400 workgroups on one counter line took longer than the rest of that kernel).
// The counts are integers: the result does not depend on the order of the atomics.
#include "kernels.h"
#include "display_check.h"  // PHX_DISPLAY_HIST_MAX_GROUPS
#include "display_rule.h"

namespace phx {

namespace {
constexpr uint32_t SPAN = PHX_DISPLAY_SPAN;
static_assert((uint32_t)DISPLAY_COUNTS <= (uint32_t)PHX_DISPLAY_SLOT_WORDS && PHX_DISPLAY_SLOT_WORDS % 16 == 0, "a slot holds the 258 counts in whole 128-byte lines");
static_assert(SPAN == (uint32_t)DISPLAY_BINS, "thread k owns bin k when a workgroup flushes its counts and when k_display_exposure sums the slots");
}  // namespace

__global__ void __launch_bounds__(PHX_DISPLAY_SPAN) k_display_histogram(DisplayArgs A, const float* __restrict__ film, unsigned long long* __restrict__ slots) {
  __shared__ unsigned long long counts[DISPLAY_COUNTS];
  const uint32_t t = threadIdx.x;
  counts[t] = 0ull;
  if (t < (uint32_t)DISPLAY_COUNTS - SPAN) counts[SPAN + t] = 0ull;
  __syncthreads();
  const uint64_t spans = (A.num_pixels + SPAN - 1u) / SPAN;
  for (uint64_t s = blockIdx.x; s < spans; s += gridDim.x) {
    const uint64_t i = s * SPAN + t;
    if (i < A.num_pixels) {
      const float* v = film + i * A.xstride;
      atomicAdd(&counts[display_bin(v[0], v[1], v[2])], 1ull);
    }
  }
  __syncthreads();
  unsigned long long* slot = slots + (size_t)(blockIdx.x % PHX_DISPLAY_SLOTS) * PHX_DISPLAY_SLOT_WORDS;
  if (counts[t]) atomicAdd(slot + t, counts[t]);
  if (t < (uint32_t)DISPLAY_COUNTS - SPAN && counts[SPAN + t]) atomicAdd(slot + SPAN + t, counts[SPAN + t]);
}

__global__ void __launch_bounds__(PHX_DISPLAY_SPAN) k_display_exposure(DisplayArgs A, const unsigned long long* __restrict__ slots, DisplayBlock* __restrict__ block) {
  __shared__ uint64_t h[DISPLAY_COUNTS];
  const uint32_t t = threadIdx.x;
  for (uint32_t k = t; k < (uint32_t)DISPLAY_COUNTS; k += SPAN) {
    uint64_t sum = 0u;
    for (uint32_t s = 0; s < (uint32_t)PHX_DISPLAY_SLOTS; ++s) sum += slots[(size_t)s * PHX_DISPLAY_SLOT_WORDS + k];
    h[k] = sum;
    if (k < (uint32_t)DISPLAY_BINS) block->histogram[k] = sum;
  }
  __syncthreads();
  if (t == 0u) {
    uint64_t N = 0u;
    for (uint32_t k = 0; k < (uint32_t)DISPLAY_BINS; ++k) N += h[k];
    display_exposure_t e{A.scale, 0u};
    if (A.flags & PHX_DISPLAY_AUTO_EXPOSURE) e = display_exposure(h, N, A.scale, A.key, A.low_q16, A.high_q16, A.min_scale, A.max_scale);
    block->pixels = N + h[DISPLAY_BIN_INVALID] + h[DISPLAY_BIN_UNLIT]; block->invalid = h[DISPLAY_BIN_INVALID]; block->unlit = h[DISPLAY_BIN_UNLIT]; block->counted = N;
    block->scale = e.scale; block->from_histogram = e.from_histogram;
  }
}

__global__ void __launch_bounds__(PHX_DISPLAY_SPAN) k_display_encode(DisplayArgs A, const float* __restrict__ film, const DisplayBlock* __restrict__ block,
                                                                     uint32_t* __restrict__ image) {
  const uint64_t i = (uint64_t)blockIdx.x * SPAN + threadIdx.x;
  if (i >= A.num_pixels) return;
  const float scale = block ? block->scale : A.scale;
  // (uniform: only a film of 65536 x 65536 has an index that needs the 64-bit division)
  const uint32_t y = A.num_pixels <= 0xffffffffull ? (uint32_t)i / A.width : (uint32_t)(i / A.width), x = (uint32_t)(i - (uint64_t)y * A.width);
  const float* v = film + i * A.xstride;
  const float d = (A.flags & PHX_DISPLAY_DITHER) ? display_dither(x, y) : 0.5f;
  // consecutive lanes, consecutive words of a row
  image[(size_t)y * A.pitch_words + x] = display_pixel(v[0], v[1], v[2], scale, A.tone, A.white, d);
}

void launch_display_histogram(hipStream_t stream, const DisplayArgs& A, uint32_t num_cus, const float* film, unsigned long long* slots, DisplayBlock* block) {
  const uint64_t spans = (A.num_pixels + SPAN - 1u) / SPAN;
  uint64_t groups = (uint64_t)(num_cus ? num_cus : 1u) * 8u;  // eight workgroups of four waves a compute unit: every wave slot of the device
  if (groups > (uint64_t)PHX_DISPLAY_HIST_MAX_GROUPS) groups = PHX_DISPLAY_HIST_MAX_GROUPS;
  if (groups > spans) groups = spans;
  hipLaunchKernelGGL(k_display_histogram, dim3((uint32_t)groups), dim3(SPAN), 0, stream, A, film, slots);
  hipLaunchKernelGGL(k_display_exposure, dim3(1), dim3(SPAN), 0, stream, A, slots, block);
}

void launch_display_encode(hipStream_t stream, const DisplayArgs& A, const float* film, const DisplayBlock* block, uint32_t* image) {
  const uint32_t blocks = (uint32_t)((A.num_pixels + SPAN - 1u) / SPAN);  // <= 2^32 pixels: 2^24 workgroups
  hipLaunchKernelGGL(k_display_encode, dim3(blocks), dim3(SPAN), 0, stream, A, film, block, image);
}

}  // namespace phx
