// denoise.hip — the film denoiser (phx_denoise in phx_xpu.h states the rule operation by operation; kernels.h has the state's layout).
// No counterpart in the reference, whose film code asks for one (src/xpu/cpu.cpp:173-174).  A post-process: no frame launches these kernels.
//
//   k_denoise_pack       film -> state 0: V from m2 and the pixel's sample count, valid, e
//   k_denoise_iteration  one a-trous iteration: a valid pixel gathers its 3 x 3 (the yardstick) and its 25 taps from one state, writes the other
//   k_denoise_unpack     state -> "primary" and "m2" of the valid pixels
//
// One thread owns one pixel; the grid is 2-D over the film; no workgroup waits on another.  An edge is a skipped tap: a coordinate is tested
// before it becomes an address.  All arithmetic is binary64 in the rule's order (the file is compiled without contraction, as every other).
//
// Each kernel is a template over GUIDE, the PHX_GUIDE_* flags of phx_denoise_guides.  GUIDE == 0 is the filter above and reads nothing
// of its last argument; DEMODULATE divides the first hit's albedo out in the pack stage and multiplies it back in the unpack stage (both read the
// guide film; nothing is kept per pixel); PLANE keeps x = (position, distance) per pixel, marks a valid pixel of coverage 0 with n.w = 2, and
// multiplies a tap's weight by the biweight of its distance from p's tangent plane.
#include "kernels.h"
#include "../../include/phx_xpu.h"  // PHX_GUIDE_*

#include <type_traits>

namespace phx {

namespace {

__device__ __forceinline__ double luminance(double r, double g, double b) { return (0.2126 * r + 0.7152 * g) + 0.0722 * b; }
// e_x of the rule from the fp32 variances
__device__ __forceinline__ double deviation(float vr, float vg, float vb) { return luminance(sqrt((double)vr), sqrt((double)vg), sqrt((double)vb)); }
// this thread's pixel -> false past the film's edge
__device__ __forceinline__ bool own_pixel(const DenoiseArgs& A, int& x, int& y, size_t& p) {
  x = (int)(blockIdx.x * PHX_DENOISE_BX + threadIdx.x); y = (int)(blockIdx.y * PHX_DENOISE_BY + threadIdx.y);
  p = (size_t)y * A.width + (size_t)x;
  return x < (int)A.width && y < (int)A.height;
}
// n of the rule: the pixel's own sample count where the film says it
__device__ __forceinline__ double samples_of(const DenoiseArgs& A, const float* px) { return A.samples_offset ? (double)px[A.samples_offset] : (double)A.spp; }

}  // namespace

template <uint32_t GUIDE>
__global__ void __launch_bounds__(PHX_DENOISE_BX * PHX_DENOISE_BY) k_denoise_pack(DenoiseArgs A, const float* __restrict__ film, DenoiseGuideArgs G) {
  int x, y; size_t p;
  if (!own_pixel(A, x, y, p)) return;
  const float* px = film + p * A.xstride;
  float c0 = px[0], c1 = px[1], c2 = px[2];
  const float m0 = px[A.m2_offset], m1 = px[A.m2_offset + 1], m2 = px[A.m2_offset + 2];
  float nx = 0.0f, ny = 0.0f, nz = 0.0f;
  if (A.normals_offset) { nx = px[A.normals_offset]; ny = px[A.normals_offset + 1]; nz = px[A.normals_offset + 2]; }
  const double n = samples_of(A, px);
  bool valid = isfinite(c0) && isfinite(c1) && isfinite(c2) && isfinite(m0) && isfinite(m1) && isfinite(m2) && isfinite(nx) && isfinite(ny) && isfinite(nz) &&
               m0 >= 0.0f && m1 >= 0.0f && m2 >= 0.0f && isfinite(n) && n >= 2.0;
  float g[8] = {};  // GUIDE: the pixel's guide floats (albedo, coverage, position, distance)
  if constexpr (GUIDE != 0u) {
    const float* gp = G.guides + p * G.xstride;
#pragma unroll
    for (int k = 0; k < 8; ++k) { g[k] = gp[k]; valid = valid && isfinite(g[k]); }
  }
  float v0 = 0.0f, v1 = 0.0f, v2 = 0.0f; double e = 0.0;
  if (valid) {
    const double q = n / (n - 1.0);
    if constexpr ((GUIDE & PHX_GUIDE_DEMODULATE) != 0u) {
      const double d0 = fmax((double)g[0], G.albedo_floor), d1 = fmax((double)g[1], G.albedo_floor), d2 = fmax((double)g[2], G.albedo_floor);
      c0 = (float)((double)c0 / d0); c1 = (float)((double)c1 / d1); c2 = (float)((double)c2 / d2);
      v0 = (float)(((double)m0 * q) / (d0 * d0)); v1 = (float)(((double)m1 * q) / (d1 * d1)); v2 = (float)(((double)m2 * q) / (d2 * d2));
    } else {
      v0 = (float)((double)m0 * q); v1 = (float)((double)m1 * q); v2 = (float)((double)m2 * q);
    }
    e = deviation(v0, v1, v2);
  }
  A.c[0][p] = make_float4(c0, c1, c2, 0.0f);
  A.v[0][p] = make_float4(v0, v1, v2, 0.0f);
  A.e[0][p] = e;
  float flag = valid ? 1.0f : 0.0f;
  if constexpr ((GUIDE & PHX_GUIDE_PLANE) != 0u) {
    if (valid && g[3] == 0.0f) flag = 2.0f;  // no camera ray of the pixel hit anything
    G.x[p] = make_float4(g[4], g[5], g[6], g[7]);
  }
  A.n[p] = make_float4(nx, ny, nz, flag);
}

template <uint32_t GUIDE>
__global__ void __launch_bounds__(PHX_DENOISE_BX * PHX_DENOISE_BY) k_denoise_iteration(DenoiseArgs A, int from, int step, DenoiseGuideArgs G) {
  int x, y; size_t p;
  if (!own_pixel(A, x, y, p)) return;
  const float4 Np = A.n[p];
  if (Np.w == 0.0f) return;  // an invalid pixel has no state
  const float4* __restrict__ C = A.c[from]; const float4* __restrict__ V = A.v[from]; const double* __restrict__ E = A.e[from];
  const float4* __restrict__ N = A.n;
  const int W_ = (int)A.width, H_ = (int)A.height;
  const float4 Cp = C[p];
  const double cr = (double)Cp.x, cg = (double)Cp.y, cb = (double)Cp.z;
  const double lp = luminance(cr, cg, cb);

  // the yardstick: the 3 x 3 mean of e * e, one pixel apart whatever the step
  constexpr double k3[3] = {0.25, 0.5, 0.25};
  double sum_g = 0.0, sum_gee = 0.0;
#pragma unroll
  for (int dy = -1; dy <= 1; ++dy) {
    const int yy = y + dy;
    if (yy < 0 || yy >= H_) continue;
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx) {
      const int xx = x + dx;
      if (xx < 0 || xx >= W_) continue;
      const size_t q = (size_t)yy * A.width + (size_t)xx;
      if (N[q].w == 0.0f) continue;
      const double g = k3[dy + 1] * k3[dx + 1], e = E[q];
      sum_gee = sum_gee + (g * e) * e;
      sum_g = sum_g + g;
    }
  }
  const double sig = A.sigma_l * sqrt(sum_gee / sum_g);

  const bool p_missed = Np.x == 0.0f && Np.y == 0.0f && Np.z == 0.0f;
  constexpr bool PLANE = (GUIDE & PHX_GUIDE_PLANE) != 0u;
  float4 Xp = make_float4(0.0f, 0.0f, 0.0f, 0.0f); double tol = 0.0;  // PLANE: p's position and the plane tolerance at its distance
  if constexpr (PLANE) { Xp = G.x[p]; tol = G.tol_scale * (double)Xp.w; }
  constexpr double k5[5] = {0.0625, 0.25, 0.375, 0.25, 0.0625};
  double W = 0.0, a0 = 0.0, a1 = 0.0, a2 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0;
#pragma unroll
  for (int dy = -2; dy <= 2; ++dy) {
    const int yy = y + step * dy;
    if (yy < 0 || yy >= H_) continue;
#pragma unroll
    for (int dx = -2; dx <= 2; ++dx) {
      const int xx = x + step * dx;
      if (xx < 0 || xx >= W_) continue;
      const size_t q = (size_t)yy * A.width + (size_t)xx;
      const float4 Nq = N[q];
      if (Nq.w == 0.0f) continue;
      const float4 Cq = C[q], Vq = V[q];
      const double h = k5[dy + 2] * k5[dx + 2];
      double w = h;
      if (dx != 0 || dy != 0) {
        double wn = 1.0;
        if (!(p_missed && Nq.x == 0.0f && Nq.y == 0.0f && Nq.z == 0.0f)) {
          double d = ((double)Np.x * (double)Nq.x + (double)Np.y * (double)Nq.y) + (double)Np.z * (double)Nq.z;
          d = d > 0.0 ? d : 0.0;
          for (uint32_t k = 0; k < A.normal_power_log2; ++k) d = d * d;
          wn = d;
        }
        const double lq = luminance((double)Cq.x, (double)Cq.y, (double)Cq.z);
        double wl;
        if (sig == 0.0) wl = lq == lp ? 1.0 : 0.0;
        else {
          const double u = fabs(lq - lp) / sig, t = 1.0 - u * u;
          wl = u < 1.0 ? t * t : 0.0;
        }
        w = (h * wn) * wl;
        if constexpr (PLANE) {
          double wx;
          const bool p_open = Np.w == 2.0f, q_open = Nq.w == 2.0f;
          if (p_open || q_open) wx = p_open && q_open ? 1.0 : 0.0;
          else {
            const float4 Xq = G.x[q];
            const double r = ((double)Np.x * ((double)Xq.x - (double)Xp.x) + (double)Np.y * ((double)Xq.y - (double)Xp.y)) + (double)Np.z * ((double)Xq.z - (double)Xp.z);
            if (tol == 0.0) wx = r == 0.0 ? 1.0 : 0.0;
            else {
              const double u = fabs(r) / tol, t = 1.0 - u * u;
              wx = u < 1.0 ? t * t : 0.0;
            }
          }
          w = w * wx;
        }
      }
      W = W + w;
      a0 = a0 + w * ((double)Cq.x - cr); a1 = a1 + w * ((double)Cq.y - cg); a2 = a2 + w * ((double)Cq.z - cb);
      const double ww = w * w;
      b0 = b0 + ww * (double)Vq.x; b1 = b1 + ww * (double)Vq.y; b2 = b2 + ww * (double)Vq.z;
    }
  }
  const double WW = W * W;
  const float v0 = (float)(b0 / WW), v1 = (float)(b1 / WW), v2 = (float)(b2 / WW);
  const int to = from ^ 1;
  A.c[to][p] = make_float4((float)(cr + a0 / W), (float)(cg + a1 / W), (float)(cb + a2 / W), 0.0f);
  A.v[to][p] = make_float4(v0, v1, v2, 0.0f);
  A.e[to][p] = deviation(v0, v1, v2);
}

template <uint32_t GUIDE>
__global__ void __launch_bounds__(PHX_DENOISE_BX * PHX_DENOISE_BY) k_denoise_unpack(DenoiseArgs A, int from, float* __restrict__ film, DenoiseGuideArgs G) {
  int x, y; size_t p;
  if (!own_pixel(A, x, y, p)) return;
  if (A.n[p].w == 0.0f) return;  // an invalid pixel keeps its input floats
  float* px = film + p * A.xstride;
  const double n = samples_of(A, px);
  const double r = (n - 1.0) / n;
  const float4 Cp = A.c[from][p], Vp = A.v[from][p];
  if constexpr ((GUIDE & PHX_GUIDE_DEMODULATE) != 0u) {
    const float* gp = G.guides + p * G.xstride;
    const double d0 = fmax((double)gp[0], G.albedo_floor), d1 = fmax((double)gp[1], G.albedo_floor), d2 = fmax((double)gp[2], G.albedo_floor);
    px[0] = (float)((double)Cp.x * d0); px[1] = (float)((double)Cp.y * d1); px[2] = (float)((double)Cp.z * d2);
    px[A.m2_offset] = (float)((((double)Vp.x * d0) * d0) * r); px[A.m2_offset + 1] = (float)((((double)Vp.y * d1) * d1) * r);
    px[A.m2_offset + 2] = (float)((((double)Vp.z * d2) * d2) * r);
  } else {
  px[0] = Cp.x; px[1] = Cp.y; px[2] = Cp.z;
  px[A.m2_offset] = (float)((double)Vp.x * r); px[A.m2_offset + 1] = (float)((double)Vp.y * r); px[A.m2_offset + 2] = (float)((double)Vp.z * r);
  }
}

// ---- launches ---------------------------------------------------------------------------------------
namespace {
dim3 denoise_grid(const DenoiseArgs& A) { return dim3((A.width + PHX_DENOISE_BX - 1) / PHX_DENOISE_BX, (A.height + PHX_DENOISE_BY - 1) / PHX_DENOISE_BY); }
const dim3 denoise_block(PHX_DENOISE_BX, PHX_DENOISE_BY);
}  // namespace

void launch_denoise_pack(hipStream_t stream, const DenoiseArgs& A, const float* film) {
  hipLaunchKernelGGL(k_denoise_pack<0u>, denoise_grid(A), denoise_block, 0, stream, A, film, DenoiseGuideArgs{});
}
void launch_denoise_iteration(hipStream_t stream, const DenoiseArgs& A, int from, uint32_t step) {
  hipLaunchKernelGGL(k_denoise_iteration<0u>, denoise_grid(A), denoise_block, 0, stream, A, from, (int)step, DenoiseGuideArgs{});
}
void launch_denoise_unpack(hipStream_t stream, const DenoiseArgs& A, int from, float* film) {
  hipLaunchKernelGGL(k_denoise_unpack<0u>, denoise_grid(A), denoise_block, 0, stream, A, from, film, DenoiseGuideArgs{});
}

// the guided instantiations: G.flags is 1, 2 or 3
namespace {
template <typename F> void with_guide_flags(uint32_t flags, F&& f) {
  if (flags == 1u) f(std::integral_constant<uint32_t, 1u>{}); else if (flags == 2u) f(std::integral_constant<uint32_t, 2u>{}); else f(std::integral_constant<uint32_t, 3u>{});
}
}  // namespace
void launch_denoise_pack_guided(hipStream_t stream, const DenoiseArgs& A, const DenoiseGuideArgs& G, const float* film) {
  with_guide_flags(G.flags, [&](auto F) { hipLaunchKernelGGL(k_denoise_pack<decltype(F)::value>, denoise_grid(A), denoise_block, 0, stream, A, film, G); });
}
void launch_denoise_iteration_guided(hipStream_t stream, const DenoiseArgs& A, const DenoiseGuideArgs& G, int from, uint32_t step) {
  // DEMODULATE alone filters the demodulated state by the unguided rule
  with_guide_flags(G.flags, [&](auto F) { hipLaunchKernelGGL(k_denoise_iteration<(decltype(F)::value & PHX_GUIDE_PLANE)>, denoise_grid(A), denoise_block, 0, stream, A, from, (int)step, G); });
}
void launch_denoise_unpack_guided(hipStream_t stream, const DenoiseArgs& A, const DenoiseGuideArgs& G, int from, float* film) {
  with_guide_flags(G.flags, [&](auto F) { hipLaunchKernelGGL(k_denoise_unpack<(decltype(F)::value & PHX_GUIDE_DEMODULATE)>, denoise_grid(A), denoise_block, 0, stream, A, from, film, G); });
}

}  // namespace phx
