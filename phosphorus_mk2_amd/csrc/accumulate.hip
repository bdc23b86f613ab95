// accumulate.hip — film accumulation across frames (phx_accumulate in phx_xpu.h states the rule operation by operation).
// No counterpart in the reference, which renders one frame and writes it out.  A pass of its own: no frame launches this kernel.
//
//   k_accumulate   frame film + accumulator -> accumulator ("primary", "normals", "m2", "samples"), and the four counters of the summary
//
// A pixel's floats lie xstride (6 .. 24) floats apart, so a lane per pixel would read 24 .. 96 byte strides.  Instead a workgroup owns a span of
// PHX_ACCUMULATE_SPAN consecutive pixels, whose floats are ONE contiguous range of each film: the workgroup moves both ranges into LDS with
// consecutive lanes on consecutive 16-byte words (4-byte words for a film that is not 16-byte aligned), one thread then pools one pixel out of
// LDS, and acc's range goes back the way it came.  LDS holds the floats as memory does, so the moves are 16-byte accesses on both sides with
// no index arithmetic; the price is paid where a thread reads its own pixel: lanes lie xstride floats apart, which is free of bank conflicts
// for an odd xstride (7, 11), 2-way for 6 and 10 and 8-way for 8, on some thirty 4-byte accesses a pixel (at strides 8 + 7 and 11 + 10 the kernel runs at a device copy's rate).
// An untouched pixel is written back with the bits it had.
// All arithmetic is binary64 in the rule's order (the file is compiled without contraction, as every other).
#include "film_pass.h"
#include "accumulate_check.h"  // PHX_ACCUMULATE_MAX_XSTRIDE

namespace phx {

namespace {

constexpr uint32_t SPAN = PHX_ACCUMULATE_SPAN;
// both spans and the waves' partial counts fit the 64 KB of LDS a launch gets without asking for more
static_assert(SPAN * 2u * PHX_ACCUMULATE_MAX_XSTRIDE * sizeof(float) + (SPAN / 64u) * 4u * sizeof(unsigned long long) <= 65536u, "k_accumulate's LDS");

// `count` floats from `from` to `to`, one of them global memory and the other LDS: 16 bytes a lane where the global side is 16-byte aligned
// (wave-uniform: a span starts a multiple of 1 KiB behind the film's first float, and behind LDS's), the rest, or all of it, float by float
__device__ __forceinline__ void move_span(const float* __restrict__ from, float* __restrict__ to, uint32_t count, bool aligned) {
  const uint32_t nvec = aligned ? count >> 2 : 0u;
  for (uint32_t v = threadIdx.x; v < nvec; v += SPAN) reinterpret_cast<float4*>(to)[v] = reinterpret_cast<const float4*>(from)[v];
  for (uint32_t i = (nvec << 2) + threadIdx.x; i < count; i += SPAN) to[i] = from[i];
}

}  // namespace

__global__ void __launch_bounds__(PHX_ACCUMULATE_SPAN) k_accumulate(AccumulateArgs A, float* __restrict__ acc, const float* __restrict__ frame,
                                                                    unsigned long long* __restrict__ counters) {
  extern __shared__ float4 lds4[];  // both spans as they lie in memory: acc's SPAN * xstride_a floats, then the frame film's
  float* lds = reinterpret_cast<float*>(lds4);
  __shared__ unsigned long long part[SPAN / 64u][4];
  float* sa = lds; float* sb = lds + SPAN * A.xstride_a;
  const uint64_t first = (uint64_t)blockIdx.x * SPAN;  // < num_pixels: the grid is ceil(num_pixels / SPAN)
  const uint32_t cnt = (uint32_t)(A.num_pixels - first < (uint64_t)SPAN ? A.num_pixels - first : (uint64_t)SPAN);
  float* ga = acc + first * A.xstride_a; const float* gb = frame + first * A.xstride_b;
  const uint32_t floats_a = cnt * A.xstride_a, floats_b = cnt * A.xstride_b;
  const bool aligned_a = (reinterpret_cast<uintptr_t>(ga) & 15u) == 0u, aligned_b = (reinterpret_cast<uintptr_t>(gb) & 15u) == 0u;
  move_span(ga, sa, floats_a, aligned_a);
  move_span(gb, sb, floats_b, aligned_b);
  __syncthreads();

  const uint32_t t = threadIdx.x;
  const bool live = t < cnt;
  bool valid = false, converged = false; unsigned long long ns = 0ull;
  if (live) {
    float* a = sa + t * A.xstride_a; const float* b = sb + t * A.xstride_b;
    float* am = a + A.m2_offset_a; const float* bm = b + A.m2_offset_b;
    const double na = (double)a[A.samples_offset_a];
    const double nb = A.samples_offset_b ? (double)b[A.samples_offset_b] : (double)A.spp_b;
    if (!(isfinite(na) && isfinite(nb) && na >= 0.0 && nb >= 0.0)) {
      const float nan = __builtin_nanf("");
      a[0] = a[1] = a[2] = nan; am[0] = am[1] = am[2] = nan; a[A.samples_offset_a] = nan;
    } else if (nb != 0.0) {
      if (na == 0.0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) { a[c] = b[c]; am[c] = bm[c]; }
        a[A.samples_offset_a] = (float)nb;
      } else {
        const double n = na + nb;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const double Va = (double)a[c], Vb = (double)b[c], m2a = (double)am[c], m2b = (double)bm[c];
          const double Qa = (m2a * na) * na, Qb = (m2b * nb) * nb;
          const double d = Vb - Va;
          const double Q = (Qa + Qb) + ((d * d) * (na * nb)) / n;
          a[c] = (float)(Va + (d * nb) / n);
          am[c] = (float)((Q / n) / n);
        }
        a[A.samples_offset_a] = (float)n;
      }
      if (A.normals_offset_a && A.normals_offset_b) {  // the last sample with a hit wins
        const float* bn = b + A.normals_offset_b;
        const float x = bn[0], y = bn[1], z = bn[2];
        if (x != 0.0f || y != 0.0f || z != 0.0f) { float* an = a + A.normals_offset_a; an[0] = x; an[1] = y; an[2] = z; }
      }
    }
    if (counters) {  // the summary, from the floats the pixel holds now
      const double n = (double)a[A.samples_offset_a];
      valid = accumulator_pixel_valid(a, am, n);
      if (valid) {
        const double q = n / (n - 1.0);
        converged = true;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const double L = (double)am[c] * q;
          const double bound = A.tau * (fabs((double)a[c]) + A.floor);
          converged = converged && L <= bound * bound;
        }
        ns = (unsigned long long)fmin(n, 9007199254740992.0);
      }
    }
  }
  if (counters) {  // (wave-uniform) ballots and one sum per wave, then one vector atomic of four lanes per workgroup
    const unsigned long long counts[4] = {wave_count(live), wave_count(live && !valid), wave_count(converged), wave_sum(ns)};  // pixels, invalid, converged, samples
    store_wave_counts(part, t, counts);
  }
  __syncthreads();  // the one barrier behind the pixels: for the span's way back and for the counts
  move_span(sa, ga, floats_a, aligned_a);
  if (counters) add_workgroup_counts(part, t, blockIdx.x, counters);
}

void launch_accumulate(hipStream_t stream, const AccumulateArgs& A, float* acc, const float* frame_film, unsigned long long* counters) {
  const uint32_t blocks = (uint32_t)((A.num_pixels + SPAN - 1u) / SPAN);  // <= 2^32 pixels: 2^24 workgroups
  const size_t lds_bytes = (size_t)SPAN * (A.xstride_a + A.xstride_b) * sizeof(float);
  hipLaunchKernelGGL(k_accumulate, dim3(blocks), dim3(SPAN), lds_bytes, stream, A, acc, frame_film, counters);
}

}  // namespace phx
