// film_pass.h — what the kernels of the film passes with a summary share on the device (accumulate.hip, reproject.hip, outlier_clamp.hip,
// tile_map.hip): the summary's counter path in two halves around the kernel's own barrier, and the test of a valid accumulator pixel.
// (display.hip counts 258 values a workgroup in LDS atomics: a scheme of its own.)
#pragma once
#include "kernels.h"

namespace phx {

// how many lanes of the wave hold a non-zero p, as __ballot reads it (wave-uniform)
__device__ __forceinline__ unsigned long long wave_count(int p) { return (unsigned long long)__popcll(__ballot(p)); }
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

// The counter path (kernels.h: summary slots), first half: lane 0 of every wave stores the wave's N counts (wave-uniform: ballots, wave_sum)
// into part[wave].  The kernel declares `part`, so its LDS is stated where its other LDS is.
template <uint32_t WAVES, uint32_t N>
__device__ __forceinline__ void store_wave_counts(unsigned long long (&part)[WAVES][N], uint32_t t, const unsigned long long (&counts)[N]) {
  if ((t & 63u) == 0u) {
#pragma unroll
    for (uint32_t k = 0; k < N; ++k) part[t >> 6][k] = counts[k];
  }
}
// Second half, behind a __syncthreads() of the kernel's (none in here: k_accumulate shares its barrier with the span's write-back): threads
// t < N sum the waves and do ONE vector atomic of N lanes into the slot of `workgroup`, the workgroup's linear id.
template <uint32_t WAVES, uint32_t N>
__device__ __forceinline__ void add_workgroup_counts(const unsigned long long (&part)[WAVES][N], uint32_t t, uint32_t workgroup, unsigned long long* counters) {
  if (t < N) {
    unsigned long long v = 0ull;
#pragma unroll
    for (uint32_t w = 0; w < WAVES; ++w) v += part[w][t];
    atomicAdd(counters + (size_t)(workgroup % PHX_SUMMARY_SLOTS) * PHX_SUMMARY_SLOT_WORDS + t, v);
  }
}

// An accumulator pixel that can be read: finite rgb (a), finite m2 >= 0 (am), a finite sample count n >= 2.  Comparisons only: the callers load.
__device__ __forceinline__ bool accumulator_pixel_valid(const float* a, const float* am, double n) {
  return isfinite(a[0]) && isfinite(a[1]) && isfinite(a[2]) && isfinite(am[0]) && isfinite(am[1]) && isfinite(am[2]) &&
         am[0] >= 0.0f && am[1] >= 0.0f && am[2] >= 0.0f && isfinite(n) && n >= 2.0;
}

}  // namespace phx
