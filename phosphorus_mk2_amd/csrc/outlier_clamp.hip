// outlier_clamp.hip — the outlier clamp of a film against a reference film's neighbourhoods (phx_outlier_clamp in phx_xpu.h states the rule
// operation by operation).  No counterpart in the reference, which renders one frame and writes it out.  A pass of its own: no
// frame launches this kernel, and it reads no scene.
//
//   k_outlier_clamp   film (A) + ref (B) -> film_out (A's layout), and the six counters of the summary
//
// A workgroup owns a tile of TILE x TILE output pixels, one thread per pixel.  The rows of B that the tile and its halo of `radius` pixels
// cover (clipped to the film) are each ONE contiguous range of floats: a wave moves a row's range into LDS as it lies in memory,
// consecutive lanes on consecutive 16-byte words.  A row starts wherever its first pixel lies, so the row's place in LDS is shifted by the
// same 0 .. 3 floats by which its first float is off a 16-byte boundary in memory: both sides of every 16-byte move are then aligned, and at
// most three floats at either end go one by one.  Each float of B is read from memory once per workgroup, and the up to 49 taps of a pixel,
// three times over (the brightest taps, the means, the variances), come from LDS.  Where B is A (despeckle) the thread's own pixel comes from
// the tile too.  There is no grid stride and no workgroup waits on another; a thread whose pixel lies outside the film forms no address.
// The pixel's code is compiled once per radius, so the window's loops unroll and a tap's index is a constant; which taps count is one 64-bit
// mask, and the trimming keeps the three brightest taps' indices in named registers: nothing is indexed at run time.
// All arithmetic is binary64 in the rule's order (the file is compiled without contraction, as every other).
#include "film_pass.h"
#include "outlier_clamp_check.h"  // PHX_OUTLIER_MAX_XSTRIDE, PHX_OUTLIER_MAX_RADIUS

namespace phx {

namespace {

constexpr uint32_t TILE = PHX_OUTLIER_TILE, BLOCK = TILE * TILE, WAVES = BLOCK / 64u;
constexpr uint32_t MAX_SIDE = TILE + 2u * PHX_OUTLIER_MAX_RADIUS;

// floats between two rows of the tile in LDS: the widest row, rounded up to whole 16-byte words, and one word for the shift
__host__ __device__ constexpr uint32_t row_pitch(uint32_t radius, uint32_t xstride_b) { return (((TILE + 2u * radius) * xstride_b + 3u) & ~3u) + 4u; }
// the tile and the waves' partial counts fit the 64 KB of LDS a launch gets without asking for more
static_assert(MAX_SIDE * row_pitch(PHX_OUTLIER_MAX_RADIUS, PHX_OUTLIER_MAX_XSTRIDE) * sizeof(float) + WAVES * 6u * sizeof(unsigned long long) <= 65536u, "k_outlier_clamp's LDS");

struct Tile {
  const float* lds; uint64_t base_words;  // ref's address in 4-byte words
  uint32_t cx0, cy0, pitch, width, xstride_b;
  // by how many floats row y of the film is shifted in LDS: what its first float's address is off a 16-byte boundary
  __device__ __forceinline__ uint32_t shift(uint32_t y) const { return (uint32_t)((base_words + ((uint64_t)y * width + cx0) * xstride_b) & 3u); }
  // where pixel (x, y) of the tile begins in LDS, in floats (32-bit arithmetic that may wrap for a pixel outside the tile: such an index is never read through)
  __device__ __forceinline__ uint32_t index(uint32_t x, uint32_t y) const { return (y - cy0) * pitch + shift(y) + (x - cx0) * xstride_b; }
  __device__ __forceinline__ const float* pixel(uint32_t x, uint32_t y) const { return lds + index(x, y); }
};

// f(tap index, the tap's pixel of B in LDS) for every tap of the window around (px, py) whose bit in `taps` is set, in tap order.  R is the
// radius at compile time: both loops unroll, a tap's index and its bit are constants, and what is left per tap is a bit test and an add
template <int R, typename F>
__device__ __forceinline__ void for_each_tap(const Tile T, uint32_t px, uint32_t py, uint64_t taps, F&& f) {
#pragma unroll
  for (int dy = -R; dy <= R; ++dy) {
    const uint32_t row = T.index(px, py + (uint32_t)dy);
#pragma unroll
    for (int dx = -R; dx <= R; ++dx) {
      constexpr int side = 2 * R + 1;
      const int ti = (dy + R) * side + (dx + R);
      if (taps >> ti & 1ull) f(ti, T.lds + (row + (uint32_t)dx * T.xstride_b));
    }
  }
}

// the window's taps that lie inside the film (the centre left out under PHX_OUTLIER_EXCLUDE_CENTRE), a bit per tap index
template <int R>
__device__ __forceinline__ uint64_t taps_inside(const OutlierClampArgs& A, uint32_t px, uint32_t py) {
  constexpr int side = 2 * R + 1;
  uint64_t taps = 0ull;
#pragma unroll
  for (int dy = -R; dy <= R; ++dy) {
    const bool row_inside = py + (uint32_t)dy < A.height;  // (unsigned: a row above the film wraps past it)
#pragma unroll
    for (int dx = -R; dx <= R; ++dx) {
      const bool inside = row_inside && px + (uint32_t)dx < A.width && !(dx == 0 && dy == 0 && (A.flags & PHX_OUTLIER_EXCLUDE_CENTRE));
      taps |= (uint64_t)inside << ((dy + R) * side + (dx + R));
    }
  }
  return taps;
}

// one colour of a pixel behind the bounds' sums: the clamp and what it does to m2 (the rule's "bounds", "clamp" and "m2")
struct Colour { float value; bool clamped, scaled; double m2; };
__device__ __forceinline__ Colour clamp_colour(const OutlierClampArgs& A, double mu, double s, float a, float m2) {
  const double w = A.gamma * sqrt(s) + A.floor, hi = mu + w, lo = mu - w, av = (double)a;
  Colour c{a, false, false, (double)m2};
  if (av > hi) { c.value = (float)hi; c.clamped = true; }
  else if (!(A.flags & PHX_OUTLIER_UPPER_ONLY) && av < lo) { c.value = (float)lo; c.clamped = true; }
  if (A.m2_offset_a && c.clamped && av != 0.0) {
    const double f = (double)c.value / av;
    if (f >= 0.0 && f < 1.0) { c.m2 = (c.m2 * f) * f; c.scaled = true; }
  }
  return c;
}

// one pixel inside the film, radius R: the rule from "skipped" to "rounding".  cls: 0 skipped, 1 unbounded, 2 inside, 3 clamped
template <int R>
__device__ __forceinline__ void clamp_pixel(const OutlierClampArgs& A, const Tile T, uint32_t px, uint32_t py, const float* film, float* film_out, int& cls, bool& capped) {
  const uint64_t p = (uint64_t)py * A.width + px;
  const float* a = A.a_is_b ? T.pixel(px, py) : film + p * A.xstride_a;
  float* out = film_out + p * A.xstride_a;
  if (film_out != film) for (uint32_t c = 0; c < A.xstride_a; ++c) out[c] = a[c];
  const uint32_t mo = A.m2_offset_a, so = A.samples_offset_a;
  const float a0 = a[0], a1 = a[1], a2 = a[2];
  const double n = so ? (double)a[so] : 0.0;
  if (!(isfinite(a0) && isfinite(a1) && isfinite(a2)) || (so && !(isfinite(n) && n > 0.0))) cls = 0;
  else {
    // the three brightest counting taps, (l0, i0) first; a tap ranks before one seen earlier only if it is strictly brighter
    const double none = -__builtin_inf();
    double l0 = none, l1 = none, l2 = none; int i0 = -1, i1 = -1, i2 = -1;
    uint64_t taps = taps_inside<R>(A, px, py);  // from here on: the taps that count
    for_each_tap<R>(T, px, py, taps, [&](int ti, const float* b) {
      if (!(isfinite(b[0]) && isfinite(b[1]) && isfinite(b[2]))) { taps &= ~(1ull << ti); return; }
      const double l = (0.2126 * (double)b[0] + 0.7152 * (double)b[1]) + 0.0722 * (double)b[2];
      const bool g0 = l > l0, g1 = l > l1, g2 = l > l2;  // g0 implies g1 implies g2; selects, so that the six stay in registers
      l2 = g1 ? l1 : g2 ? l : l2; i2 = g1 ? i1 : g2 ? ti : i2;
      l1 = g0 ? l0 : g1 ? l : l1; i1 = g0 ? i0 : g1 ? ti : i1;
      l0 = g0 ? l : l0;           i0 = g0 ? ti : i0;
    });
    if (A.trim >= 1u && i0 >= 0) taps &= ~(1ull << i0);  // from here on: the taps left
    if (A.trim >= 2u && i1 >= 0) taps &= ~(1ull << i1);
    if (A.trim >= 3u && i2 >= 0) taps &= ~(1ull << i2);
    const uint32_t k = (uint32_t)__popcll(taps);
    if (k < A.min_taps) cls = 1;
    else {
      const double kd = (double)k;
      double sum0 = 0.0, sum1 = 0.0, sum2 = 0.0, ss0 = 0.0, ss1 = 0.0, ss2 = 0.0;
      for_each_tap<R>(T, px, py, taps, [&](int, const float* b) { sum0 += (double)b[0]; sum1 += (double)b[1]; sum2 += (double)b[2]; });
      const double mu0 = sum0 / kd, mu1 = sum1 / kd, mu2 = sum2 / kd;
      for_each_tap<R>(T, px, py, taps, [&](int, const float* b) {
        const double e0 = (double)b[0] - mu0, e1 = (double)b[1] - mu1, e2 = (double)b[2] - mu2;
        ss0 += e0 * e0; ss1 += e1 * e1; ss2 += e2 * e2;
      });
      Colour c0 = clamp_colour(A, mu0, ss0 / kd, a0, mo ? a[mo] : 0.0f), c1 = clamp_colour(A, mu1, ss1 / kd, a1, mo ? a[mo + 1u] : 0.0f),
             c2 = clamp_colour(A, mu2, ss2 / kd, a2, mo ? a[mo + 2u] : 0.0f);
      const bool any = c0.clamped || c1.clamped || c2.clamped;
      cls = any ? 3 : 2;
      if (A.clamped_history > 0.0 && any && n > A.clamped_history) {  // (the check: clamped_history > 0 only with a samples channel)
        capped = true;
        const double q = n / A.clamped_history;
        c0.m2 = c0.m2 * q; c1.m2 = c1.m2 * q; c2.m2 = c2.m2 * q;
        c0.scaled = c1.scaled = c2.scaled = true;
        out[so] = (float)A.clamped_history;
      }
      if (c0.clamped) out[0] = c0.value;
      if (c1.clamped) out[1] = c1.value;
      if (c2.clamped) out[2] = c2.value;
      if (mo) {
        if (c0.scaled) out[mo] = (float)c0.m2;
        if (c1.scaled) out[mo + 1u] = (float)c1.m2;
        if (c2.scaled) out[mo + 2u] = (float)c2.m2;
      }
    }
  }
}

}  // namespace

__global__ void __launch_bounds__(PHX_OUTLIER_TILE * PHX_OUTLIER_TILE) k_outlier_clamp(OutlierClampArgs A, const float* film, const float* __restrict__ ref, float* film_out,
                                                                                      unsigned long long* __restrict__ counters) {
  extern __shared__ float4 lds4[];  // the tile's rows of B as they lie in memory, row_pitch floats apart, each shifted by 0 .. 3 floats
  float* lds = reinterpret_cast<float*>(lds4);
  __shared__ unsigned long long part[WAVES][6];
  const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6, r = A.radius;
  const uint32_t x0 = blockIdx.x * TILE, y0 = blockIdx.y * TILE;  // inside the film: the grid is ceil(width / TILE) x ceil(height / TILE)
  Tile T;
  T.lds = lds; T.base_words = (uint64_t)(reinterpret_cast<uintptr_t>(ref) >> 2); T.width = A.width; T.xstride_b = A.xstride_b;
  T.cx0 = x0 > r ? x0 - r : 0u; T.cy0 = y0 > r ? y0 - r : 0u; T.pitch = row_pitch(r, A.xstride_b);
  const uint32_t cx1 = x0 + TILE + r < A.width ? x0 + TILE + r : A.width, cy1 = y0 + TILE + r < A.height ? y0 + TILE + r : A.height;
  const uint32_t rows = cy1 - T.cy0, count = (cx1 - T.cx0) * A.xstride_b;  // count <= pitch - 4
  const bool words = (reinterpret_cast<uintptr_t>(ref) & 3u) == 0u;
  for (uint32_t row = wave; row < rows; row += WAVES) {  // (wave-uniform) a wave per row: [cx0, cx1) of film row cy0 + row, inside the film
    const uint32_t y = T.cy0 + row, shift = T.shift(y);
    const float* g = ref + ((uint64_t)y * A.width + T.cx0) * A.xstride_b;
    float* s = lds + row * T.pitch + shift;
    const uint32_t to_boundary = (4u - shift) & 3u;
    const uint32_t head = words && to_boundary < count ? to_boundary : count, nvec = (count - head) >> 2;  // (a film off a 4-byte boundary: all head)
    for (uint32_t i = lane; i < head; i += 64u) s[i] = g[i];
    for (uint32_t v = lane; v < nvec; v += 64u) reinterpret_cast<float4*>(s + head)[v] = reinterpret_cast<const float4*>(g + head)[v];
    for (uint32_t i = head + (nvec << 2) + lane; i < count; i += 64u) s[i] = g[i];
  }
  __syncthreads();

  const uint32_t px = x0 + (t & (TILE - 1u)), py = y0 + t / TILE;
  const bool live = px < A.width && py < A.height;
  int cls = -1; bool capped = false;
  if (live) {  // (the radius is wave-uniform)
    if (r == 1u) clamp_pixel<1>(A, T, px, py, film, film_out, cls, capped);
    else if (r == 2u) clamp_pixel<2>(A, T, px, py, film, film_out, cls, capped);
    else clamp_pixel<3>(A, T, px, py, film, film_out, cls, capped);
  }
  if (counters) {  // (wave-uniform) ballots, then one vector atomic of six lanes per workgroup
    // pixels, skipped, unbounded, inside, clamped, capped
    const unsigned long long counts[6] = {wave_count(live), wave_count(cls == 0), wave_count(cls == 1), wave_count(cls == 2), wave_count(cls == 3), wave_count(capped)};
    store_wave_counts(part, t, counts);
    __syncthreads();
    add_workgroup_counts(part, t, blockIdx.y * gridDim.x + blockIdx.x, counters);
  }
}

void launch_outlier_clamp(hipStream_t stream, const OutlierClampArgs& A, const float* film, const float* ref, float* film_out, unsigned long long* counters) {
  const dim3 grid((A.width + TILE - 1u) / TILE, (A.height + TILE - 1u) / TILE);  // <= 4096 x 4096 workgroups
  const size_t lds_bytes = (size_t)(TILE + 2u * A.radius) * row_pitch(A.radius, A.xstride_b) * sizeof(float);
  hipLaunchKernelGGL(k_outlier_clamp, grid, dim3(BLOCK), lds_bytes, stream, A, film, ref, film_out, counters);
}

}  // namespace phx
