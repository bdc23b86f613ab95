// tile_map.hip — the tile map (phx_tile_map in phx_xpu.h states the rule operation by operation).
// No counterpart in the reference, which renders one frame and writes it out.  A pass of its own: no frame launches this kernel.
//
//   k_tile_map   accumulator film -> one phx_tile_record per tile of a grid, and the six counters of the summary
//
// One workgroup per tile.  A tile's row is w * xstride contiguous floats of which 7 a pixel are read; consecutive threads take consecutive
// pixels of a row, so a wave's seven loads walk the same 64 * xstride floats and every 128-byte line they touch is fetched from memory once
// and met again in the vector cache by the later loads (DESIGN 26 has the measurement against a device copy and against an LDS-staged row).
// -DPHX_TILE_MAP_STAGED=1 builds that other way for the measurement: the rows of a chunk of pixels go through LDS as they lie in memory,
// as k_accumulate moves its span.
// A thread keeps its counts in registers over all its pixels; the waves' counts meet in LDS, and thread 0 writes the tile's record with
// ordinary stores: no word of `records` is written by two workgroups.  The summary goes the counter path of film_pass.h.
// All arithmetic is binary64 in the rule's order (the file is compiled without contraction, as every other).
#include "film_pass.h"
#include "tile_map_check.h"  // PHX_TILE_MAP_MAX_XSTRIDE

#ifndef PHX_TILE_MAP_STAGED
#define PHX_TILE_MAP_STAGED 0
#endif

namespace phx {

namespace {

constexpr uint32_t BLOCK = PHX_TILE_MAP_BLOCK, WAVES = BLOCK / 64u;

// what a thread, then a wave, then the workgroup knows of its pixels
struct TileCounts {
  uint32_t pixels = 0u, invalid = 0u, starved = 0u, converged = 0u, worst = 0u;  // worst: the bits of a non-negative float, which order as the floats do
  unsigned long long samples = 0ull;
};

// one pixel by the rule: a its first float, am its m2, n its sample count
__device__ __forceinline__ void count_pixel(const TileMapArgs& A, const float* a, const float* am, double n, TileCounts& c) {
  ++c.pixels;
  if (!accumulator_pixel_valid(a, am, n)) {
    ++c.invalid;
    if (isfinite(n) && n >= 0.0 && n < 2.0) ++c.starved;
    return;
  }
  const double q = n / (n - 1.0);
  bool converged = true; double r = 0.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double L = (double)am[k] * q;
    const double den = fabs((double)a[k]) + A.floor;
    const double b = A.tau * den;
    converged = converged && L <= b * b;
    const double rc = den > 0.0 ? sqrt(L) / den : (L == 0.0 ? 0.0 : (double)__builtin_inff());
    r = rc > r ? rc : r;
  }
  if (converged) ++c.converged;
  c.samples += (unsigned long long)fmin(n, 9007199254740992.0);
  const uint32_t bits = __float_as_uint((float)r);
  c.worst = bits > c.worst ? bits : c.worst;
}

__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)v, m); v = o > v ? o : v; }
  return v;
}

}  // namespace

__global__ void __launch_bounds__(PHX_TILE_MAP_BLOCK) k_tile_map(TileMapArgs A, const float* __restrict__ acc, phx_tile_record* __restrict__ records,
                                                                 unsigned long long* __restrict__ counters) {
  __shared__ unsigned long long part[WAVES][6];  // pixels, invalid, converged, samples, tiles, open: the summary's order
  __shared__ uint32_t more[WAVES][2];            // starved, worst
#if PHX_TILE_MAP_STAGED
  __shared__ float rows[BLOCK * PHX_TILE_MAP_MAX_XSTRIDE];  // a chunk's pixels as they lie in memory, row behind row
#endif
  const uint32_t t = threadIdx.x;
  const uint32_t ti = blockIdx.x % A.tiles_x, tj = blockIdx.x / A.tiles_x;  // the grid is tiles_x * tiles_y workgroups
  const uint32_t x0 = ti * A.tile_width, y0 = tj * A.tile_height;           // < width, < height
  const uint32_t w = A.width - x0 < A.tile_width ? A.width - x0 : A.tile_width, h = A.height - y0 < A.tile_height ? A.height - y0 : A.tile_height;
  TileCounts c;
#if PHX_TILE_MAP_STAGED
  // chunks of cw columns x cr rows, cw * cr <= BLOCK pixels: each row's cw * xstride floats are moved with consecutive lanes on consecutive words
  const uint32_t cw = w < BLOCK ? w : BLOCK, cr = BLOCK / cw, row_floats = cw * A.xstride;
  for (uint32_t yy = 0; yy < h; yy += cr)
    for (uint32_t xx = 0; xx < w; xx += cw) {
      const uint32_t nr = h - yy < cr ? h - yy : cr, nc = w - xx < cw ? w - xx : cw, nf = nc * A.xstride;
      for (uint32_t i = t; i < nr * nf; i += BLOCK) {
        const uint32_t r = i / nf, j = i - r * nf;
        rows[r * row_floats + j] = acc[((size_t)(y0 + yy + r) * A.width + x0 + xx) * A.xstride + j];
      }
      __syncthreads();
      const uint32_t r = t / nc, col = t - r * nc;
      if (r < nr) {
        const float* a = rows + r * row_floats + col * A.xstride;
        count_pixel(A, a, a + A.m2_offset, (double)a[A.samples_offset], c);
      }
      __syncthreads();
    }
#else
  const uint32_t count = w * h;  // <= 2^20
  for (uint32_t p = t; p < count; p += BLOCK) {
    const uint32_t r = p / w, col = p - r * w;
    const float* g = acc + ((size_t)(y0 + r) * A.width + x0 + col) * A.xstride;
    const float a[3] = {g[0], g[1], g[2]}, am[3] = {g[A.m2_offset], g[A.m2_offset + 1u], g[A.m2_offset + 2u]};
    count_pixel(A, a, am, (double)g[A.samples_offset], c);
  }
#endif
  {  // (wave-uniform) one sum per count and wave
    const unsigned long long counts[6] = {wave_sum(c.pixels), wave_sum(c.invalid), wave_sum(c.converged), wave_sum(c.samples), t == 0u ? 1ull : 0ull, 0ull};
    store_wave_counts(part, t, counts);
    const uint32_t starved = (uint32_t)wave_sum(c.starved), worst = wave_max(c.worst);
    if ((t & 63u) == 0u) { more[t >> 6][0] = starved; more[t >> 6][1] = worst; }
  }
  __syncthreads();
  if (t == 0u) {  // the tile's record, by the one thread of the one workgroup that owns it
    phx_tile_record rec;
    rec.tile = phx_tile{x0, y0, w, h};
    uint32_t invalid = 0u, starved = 0u, converged = 0u, worst = 0u; unsigned long long samples = 0ull;
#pragma unroll
    for (uint32_t k = 0; k < WAVES; ++k) {
      invalid += (uint32_t)part[k][1]; converged += (uint32_t)part[k][2]; samples += part[k][3];
      starved += more[k][0]; worst = more[k][1] > worst ? more[k][1] : worst;
    }
    rec.invalid = invalid; rec.starved = starved; rec.converged = converged; rec.worst = __uint_as_float(worst); rec.samples = samples;
    records[blockIdx.x] = rec;
    part[0][5] = (converged < w * h - invalid || starved > 0u) ? 1ull : 0ull;  // open
  }
  if (counters) {  // (workgroup-uniform)
    __syncthreads();  // part[0][5]
    add_workgroup_counts(part, t, blockIdx.x, counters);
  }
}

void launch_tile_map(hipStream_t stream, const TileMapArgs& A, uint32_t num_tiles, const float* acc, phx_tile_record* records, unsigned long long* counters) {
  hipLaunchKernelGGL(k_tile_map, dim3(num_tiles), dim3(BLOCK), 0, stream, A, acc, records, counters);
}

}  // namespace phx
