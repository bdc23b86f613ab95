// reproject.hip — carrying an accumulator film from one camera to another (phx_reproject in phx_xpu.h states the rule operation by
// operation).  No counterpart in the reference, which renders one frame from one camera.  A pass of its own: no frame launches
// this kernel, and it reads no scene.
//
//   k_reproject   acc_from + guides_from + guides_to + two cameras -> acc_to (every float), and the five counters of the summary
//
// One thread per OUTPUT pixel, workgroups of PHX_REPROJECT_BLOCK consecutive pixels.  A thread reads its 8 guide floats, projects the first
// hit through both cameras and gathers the four taps around the sampling point straight from memory: under a small camera move neighbouring
// threads sample neighbouring points, so a wave's taps are a few rows of consecutive pixels that L1 / L2 serve (DESIGN 22 has the measured
// rate beside a device copy's); there is no LDS staging.  Every index is tested against the film before it is formed.
// All arithmetic is binary64 in the rule's order (the file is compiled without contraction, as every other).
#include "film_pass.h"

namespace phx {

namespace {

constexpr uint32_t BLOCK = PHX_REPROJECT_BLOCK;

// project(K, X) of the rule: false for a point behind the camera (a NaN is behind it)
__device__ __forceinline__ bool project(const ReprojectCamera& K, double X, double Y, double Z, double& fx, double& fy) {
  const double dx = X - K.o[0], dy = Y - K.o[1], dz = Z - K.o[2];
  const double cx = (dx * K.inv[0] + dy * K.inv[3]) + dz * K.inv[6];
  const double cy = (dx * K.inv[1] + dy * K.inv[4]) + dz * K.inv[7];
  const double cz = (dx * K.inv[2] + dy * K.inv[5]) + dz * K.inv[8];
  if (!(cz < 0.0)) return false;
  const double t = -cz;
  fx = ((cx / t) / (K.ratio * K.zoom) + 0.5) * K.w;
  fy = (0.5 - (cy / t) / K.zoom) * K.h;
  return true;
}

}  // namespace

__global__ void __launch_bounds__(PHX_REPROJECT_BLOCK) k_reproject(ReprojectArgs A, const float* __restrict__ acc_from, const float* __restrict__ guides_from,
                                                                   const float* __restrict__ guides_to, float* __restrict__ acc_to,
                                                                   unsigned long long* __restrict__ counters) {
  __shared__ unsigned long long part[BLOCK / 64u][5];
  const uint32_t t = threadIdx.x;
  const uint64_t p = (uint64_t)blockIdx.x * BLOCK + t;
  const bool live = p < A.num_pixels;
  bool reused = false, no_geometry = false; unsigned long long ns = 0ull;
  if (live) {
    float* out = acc_to + p * A.xstride_a;
    const float* G = guides_to + p * A.xstride_g;
    const uint32_t x = (uint32_t)(p % A.width), y = (uint32_t)(p / A.width);
    // the four taps by their place in tap order: pixel index, and weight (0: the tap does not count); static indices, so they stay in registers
    uint64_t tap_q[4] = {0ull, 0ull, 0ull, 0ull}; double tap_w[4] = {0.0, 0.0, 0.0, 0.0};
    if (!(G[3] > 0.0f)) no_geometry = true;
    else {
      const double X = (double)G[4], Y = (double)G[5], Z = (double)G[6];
      double fxa, fya, fxb, fyb;
      if (project(A.from, X, Y, Z, fxa, fya) && project(A.to, X, Y, Z, fxb, fyb)) {
        const double sx = (double)x + (fxa - fxb), sy = (double)y + (fya - fyb);
        if (sx > -1.0 && sx < (double)A.width && sy > -1.0 && sy < (double)A.height) {
          const double x0 = floor(sx), y0 = floor(sy), tx = sx - x0, ty = sy - y0;
          const double plane_scale = A.from.zoom / A.from.h;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const double qx = x0 + (double)(k & 1), qy = y0 + (double)(k >> 1);
            const double w = ((k & 1) ? tx : 1.0 - tx) * ((k >> 1) ? ty : 1.0 - ty);
            if (!(w > 0.0)) continue;
            if (qx < 0.0 || qx >= (double)A.width || qy < 0.0 || qy >= (double)A.height) continue;
            const uint64_t q = (uint64_t)qy * A.width + (uint64_t)qx;  // < num_pixels
            const float* a = acc_from + q * A.xstride_a;
            const float* am = a + A.m2_offset_a; const float* an = a + A.normals_offset_a;
            const double n = (double)a[A.samples_offset_a];
            if (!(accumulator_pixel_valid(a, am, n) && isfinite(an[0]) && isfinite(an[1]) && isfinite(an[2]))) continue;
            const float* g = guides_from + q * A.xstride_g;
            bool finite = true;
#pragma unroll
            for (int c = 0; c < 8; ++c) finite = finite && isfinite(g[c]);
            if (!finite || !(g[3] > 0.0f)) continue;
            const double ddx = X - (double)g[4], ddy = Y - (double)g[5], ddz = Z - (double)g[6];
            const double tol = plane_scale * (double)g[7];
            const double r = ((double)an[0] * ddx + (double)an[1] * ddy) + (double)an[2] * ddz;
            if (!(fabs(r) <= A.sigma_plane * tol)) continue;
            const double dd = (ddx * ddx + ddy * ddy) + ddz * ddz, lim = A.sigma_dist * tol;
            if (!(dd <= lim * lim)) continue;
            tap_q[k] = q; tap_w[k] = w;
          }
        }
      }
    }
    double wsum = 0.0, wbest = 0.0; uint64_t qb = 0ull;  // (0.0 + w == w bit for bit for w > 0: the sum starts at its first term); ties to the first
#pragma unroll
    for (int k = 0; k < 4; ++k) if (tap_w[k] > 0.0) { wsum += tap_w[k]; if (tap_w[k] > wbest) { wbest = tap_w[k]; qb = tap_q[k]; } }
    if (!(wbest > 0.0)) {
      for (uint32_t c = 0; c < A.xstride_a; ++c) out[c] = 0.0f;
    } else {
      const float* b = acc_from + qb * A.xstride_a;
      for (uint32_t c = 0; c < A.xstride_a; ++c) out[c] = b[c];
      double n = 0.0, V[3] = {0.0, 0.0, 0.0}, m[3] = {0.0, 0.0, 0.0};
      bool started = false;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (!(tap_w[k] > 0.0)) continue;
        const float* a = acc_from + tap_q[k] * A.xstride_a; const float* am = a + A.m2_offset_a;
        const double u = tap_w[k] / wsum, uu = u * u;
        const double tn = u * (double)a[A.samples_offset_a];
        n = started ? n + tn : tn;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const double tv = u * (double)a[c], tm = uu * (double)am[c];
          V[c] = started ? V[c] + tv : tv;
          m[c] = started ? m[c] + tm : tm;
        }
        started = true;
      }
      const double n_out = n < A.max_history ? n : A.max_history;
      if (n > n_out) {
        const double s = n / n_out;
#pragma unroll
        for (int c = 0; c < 3; ++c) m[c] = m[c] * s;
      }
      const float nf = (float)n_out;
#pragma unroll
      for (int c = 0; c < 3; ++c) { out[c] = (float)V[c]; out[A.m2_offset_a + c] = (float)m[c]; }
      out[A.samples_offset_a] = nf;
      reused = true;
      ns = (unsigned long long)nf;  // finite and >= 0: a convex mix of valid counts, capped
    }
  }
  if (counters) {  // (wave-uniform) ballots and one sum per wave, then one vector atomic of five lanes per workgroup
    // pixels, reused, no_geometry, disoccluded, samples
    const unsigned long long counts[5] = {wave_count(live), wave_count(reused), wave_count(no_geometry), wave_count(live && !reused && !no_geometry), wave_sum(ns)};
    store_wave_counts(part, t, counts);
    __syncthreads();
    add_workgroup_counts(part, t, blockIdx.x, counters);
  }
}

void launch_reproject(hipStream_t stream, const ReprojectArgs& A, const float* acc_from, const float* guides_from, const float* guides_to, float* acc_to,
                      unsigned long long* counters) {
  const uint32_t blocks = (uint32_t)((A.num_pixels + BLOCK - 1u) / BLOCK);  // <= 2^32 pixels: 2^24 workgroups
  hipLaunchKernelGGL(k_reproject, dim3(blocks), dim3(BLOCK), 0, stream, A, acc_from, guides_from, guides_to, acc_to, counters);
}

}  // namespace phx
