// film_hooks.hip — the small kernels around a pass and their launches (see kernels.h for the HBM layout and the map of kernels
// to files): the start of a pass and the film, the hook kernels of the parity tests (phx_dev_*: one device function per lane,
// exactly as the shade kernels call it), and the preprocess kernels that lay the scene's tables out in pool order.
//
//   k_film      the per-sample film add of tile_renderer_t::render_tile (reference src/xpu/cpu.cpp:175-198), in sample order
//   k_adaptive_*    adaptive sampling: the decision behind a round, the stable compaction of the pixels that go on, the rows' moves (no counterpart in the reference)
//   k_film_moments  the same add, and beside it the centred second moment of a pixel's samples (phx_frame.moments_channel; no counterpart in the reference)
#include "shade_common.h"

namespace phx {

// ---- pass ---------------------------------------------------------------------------------------------
// start of a pass: queue 0 "holds" the num_pixels x num_samples camera rays (state_t::reset, spt.hpp:39-49, is implicit:
// the first k_shade writes beta, depth and radiance of every path without reading them)
__global__ void k_begin_pass(PassBuffers pb, uint32_t num_samples) {
  const uint32_t npaths = pb.num_pixels * num_samples;
  pb.counters[0] = npaths; pb.counters[CNT_STRIDE] = 0; pb.counters[CNT_SHADOW] = 0; pb.counters[CNT_SHADOW + CNT_STRIDE] = 0;
  zero_cursors(pb.counters);
  atomicAdd(&pb.stats->camera_samples, (unsigned long long)npaths);
}

// ---- film -------------------------------------------------------------------------------------------
// channels.primary->add(x, y, r * (1.0f / (spp * pps))) per sample, IN SAMPLE ORDER (cpu.cpp:175-198): the sum of a pixel is
// a serial chain, so it cannot be a lane-parallel reduction.  Radiance is stored pixel-major (pix * S + s): a 256-thread
// block moves 64 pixels x 16 samples at a time through LDS — read as 256-B runs of one pixel's samples, summed by the 64
// threads that own a pixel each (row pitch 17 float4: conflict-free) — instead of every thread striding 16*S bytes.
#define PHX_FILM_PIX 64
#define PHX_FILM_SMP 16
__global__ void __launch_bounds__(256) k_film(PassBuffers pb, uint32_t num_samples, float inv) {
  __shared__ float4 tile[PHX_FILM_PIX * (PHX_FILM_SMP + 1)];
  const uint32_t pix0 = blockIdx.x * PHX_FILM_PIX;
  const uint32_t my_pix = pix0 + threadIdx.x;
  const bool owner = threadIdx.x < PHX_FILM_PIX && my_pix < pb.num_pixels;
  float r = 0.0f, g = 0.0f, b = 0.0f;
  float* out = pb.acc + (size_t)my_pix * pb.xstride;
  if (owner) { r = out[0]; g = out[1]; b = out[2]; }
  float nx = 0.0f, ny = 0.0f, nz = 0.0f; bool have_n = false;
  const int nsrc = pb.pn ? 2 : 1;
  for (uint32_t s0 = 0; s0 < num_samples; s0 += PHX_FILM_SMP) {
    for (int src = 0; src < nsrc; ++src) {
      const float4* __restrict__ in = src ? pb.pn : pb.pr;
      __syncthreads();  // the previous tile has been consumed
#pragma unroll
      for (int k = 0; k < PHX_FILM_PIX * PHX_FILM_SMP / 256; ++k) {
        const uint32_t e = k * 256 + threadIdx.x, p = e / PHX_FILM_SMP, sm = e % PHX_FILM_SMP;
        if (pix0 + p < pb.num_pixels && s0 + sm < num_samples) tile[p * (PHX_FILM_SMP + 1) + sm] = in[(size_t)(pix0 + p) * num_samples + s0 + sm];
      }
      __syncthreads();
      if (owner) {
        const uint32_t cnt = min((uint32_t)PHX_FILM_SMP, num_samples - s0);
        for (uint32_t sm = 0; sm < cnt; ++sm) {
          const float4 c = tile[threadIdx.x * (PHX_FILM_SMP + 1) + sm];
          if (src == 0) { r += c.x * inv; g += c.y * inv; b += c.z * inv; }
          else if (c.w != 0.0f) { nx = c.x; ny = c.y; nz = c.z; have_n = true; }  // the last sample with a primary hit wins
        }
      }
    }
  }
  if (owner) {
    out[0] = r; out[1] = g; out[2] = b;
    if (have_n) { out[pb.normals_offset] = nx; out[pb.normals_offset + 1] = ny; out[pb.normals_offset + 2] = nz; }
  }
}

// ---- film with the moments channel ---------------------------------------------------------------------
// phx_frame.moments_channel (phx_xpu.h states the rule): k_film's walk — the same staging, the same fp32 chain of `primary`, the same
// normals — and beside it, per colour, the centred second moment of the pixel's samples y_s = x_s * inv by Welford's update in binary64.  The
// three colours' chains are independent, so a pixel has three owner threads, one per colour (thread = colour * 64 + pixel: waves 0-2 of the
// block; colour 0's also keeps the normals), and the block's fourth wave makes what is uniform over pixels: r_n = 1 / n, one IEEE division
// per sample index of the tile, handed over through LDS.  `samples_done` = the samples earlier passes have added to the batch buffer (s0).
__global__ void __launch_bounds__(256) k_film_moments(PassBuffers pb, uint32_t num_samples, float inv, uint32_t samples_done, uint32_t m2_offset) {
  __shared__ float4 tile[PHX_FILM_PIX * (PHX_FILM_SMP + 1)];
  __shared__ double rn[PHX_FILM_SMP];
  const uint32_t pix0 = blockIdx.x * PHX_FILM_PIX;
  const uint32_t lp = threadIdx.x % PHX_FILM_PIX, col = threadIdx.x / PHX_FILM_PIX;  // col 3: the wave of r_n
  const uint32_t my_pix = pix0 + lp;
  const bool owner = col < 3u && my_pix < pb.num_pixels;
  float f = 0.0f, m2 = 0.0f;
  float* out = pb.acc + (size_t)my_pix * pb.xstride;
  if (owner) { f = out[col]; m2 = out[m2_offset + col]; }
  double mean = samples_done ? (double)f / (double)samples_done : 0.0, M2 = (double)m2;
  float nx = 0.0f, ny = 0.0f, nz = 0.0f; bool have_n = false;
  const int nsrc = pb.pn ? 2 : 1;
  for (uint32_t s0 = 0; s0 < num_samples; s0 += PHX_FILM_SMP) {
    for (int src = 0; src < nsrc; ++src) {
      const float4* __restrict__ in = src ? pb.pn : pb.pr;
      __syncthreads();  // the previous tile has been consumed
#pragma unroll
      for (int k = 0; k < PHX_FILM_PIX * PHX_FILM_SMP / 256; ++k) {
        const uint32_t e = k * 256 + threadIdx.x, p = e / PHX_FILM_SMP, sm = e % PHX_FILM_SMP;
        if (pix0 + p < pb.num_pixels && s0 + sm < num_samples) tile[p * (PHX_FILM_SMP + 1) + sm] = in[(size_t)(pix0 + p) * num_samples + s0 + sm];
      }
      if (src == 0 && col == 3u && lp < PHX_FILM_SMP) rn[lp] = 1.0 / (double)(samples_done + s0 + lp + 1u);
      __syncthreads();
      if (owner) {
        const uint32_t cnt = min((uint32_t)PHX_FILM_SMP, num_samples - s0);
        for (uint32_t sm = 0; sm < cnt; ++sm) {
          const float4 c = tile[lp * (PHX_FILM_SMP + 1) + sm];
          if (src == 0) {
            const float y = (col == 0u ? c.x : col == 1u ? c.y : c.z) * inv;
            f += y;  // k_film's chain
            const double d = (double)y - mean;
            mean = mean + d * rn[sm];
            M2 = M2 + d * ((double)y - mean);
          } else if (col == 0u && c.w != 0.0f) { nx = c.x; ny = c.y; nz = c.z; have_n = true; }  // the last sample with a primary hit wins
        }
      }
    }
  }
  if (owner) {
    out[col] = f; out[m2_offset + col] = (float)M2;
    if (have_n) { out[pb.normals_offset] = nx; out[pb.normals_offset + 1] = ny; out[pb.normals_offset + 2] = nz; }
  }
}

// batch render buffer -> full-frame device film (film_t::add_tile for a device-resident sink)
__global__ void __launch_bounds__(PHX_BLOCK) k_scatter_film(PassBuffers pb, float* film, uint32_t film_width) {
  const uint32_t pix = blockIdx.x * PHX_BLOCK + threadIdx.x;
  if (pix >= pb.num_pixels) return;
  const uint32_t xy = pb.pix_xy[pix];
  const float* src = pb.acc + (size_t)pix * pb.xstride;
  float* dst = film + ((size_t)(xy >> 16) * film_width + (xy & 0xffffu)) * pb.xstride;
  for (uint32_t c = 0; c < pb.xstride; ++c) dst[c] = src[c];
}

// ---- adaptive sampling: the selection behind a round (phx_adaptive in phx_xpu.h states the rule) -----------------------------------
// A STABLE compaction of the rows that go on, as three launches with no waiting between workgroups: k_adaptive_count decides per row and
// counts each block's survivors, k_adaptive_scan (one workgroup) turns the counts into offsets and publishes the total, k_adaptive_write
// decides again — the same expression on the same floats — writes every survivor's row index at its place and rescales the rows that stop.
// A row belongs to ONE thread, and a row that goes on is not written: the second decision reads what the first one read.
// q, g and k are uniform over the rows and come from the host (adaptive_args in device.cpp: IEEE binary64 divisions).
#define PHX_SEL_BLOCK 256
static_assert(PHX_SEL_BLOCK == PHX_ADAPTIVE_BLOCK, "the host sizes the block-count scratch by it");
// the decision for row `row`: true = it stops.  A NaN compares false: such a pixel never stops.
__device__ __forceinline__ bool adaptive_stops(const AdaptiveArgs& A, const float* row) {
  bool stop = true;
#pragma unroll
  for (uint32_t c = 0; c < 3u; ++c) {
    const double L = (double)row[A.m2_offset + c] * A.q;
    const double b = A.tau * (fabs((double)row[c]) + A.g);
    stop = stop && (L <= b * b);
  }
  return stop;
}
// -> this thread's row goes on (false for threads past num_active); `row` = its index
__device__ __forceinline__ bool adaptive_survives(const AdaptiveArgs& A, uint32_t i, uint32_t& row) {
  if (i >= A.num_active) { row = 0u; return false; }
  row = A.active ? A.active[i] : i;
  return !adaptive_stops(A, A.acc + (size_t)row * A.xstride);
}
// survivors among the block's threads before this one (exclusive) and in the whole block: a ballot per wave, a 4-entry scan in LDS
__device__ __forceinline__ uint32_t block_rank(bool alive, uint32_t& block_total) {
  __shared__ uint32_t wave_count[PHX_SEL_BLOCK / 64];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const unsigned long long m = __ballot(alive);
  if (lane == 0u) wave_count[wave] = (uint32_t)__popcll(m);
  __syncthreads();
  uint32_t before = 0u, total = 0u;
#pragma unroll
  for (uint32_t w = 0; w < PHX_SEL_BLOCK / 64; ++w) { const uint32_t c = wave_count[w]; before += w < wave ? c : 0u; total += c; }
  block_total = total;
  return before + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
}
__global__ void __launch_bounds__(PHX_SEL_BLOCK) k_adaptive_count(AdaptiveArgs A, uint32_t* __restrict__ block_counts) {
  uint32_t row, total;
  const bool alive = adaptive_survives(A, blockIdx.x * PHX_SEL_BLOCK + threadIdx.x, row);
  (void)block_rank(alive, total);
  if (threadIdx.x == 0u) block_counts[blockIdx.x] = total;
}
// one workgroup: counts[0 .. n) -> their exclusive prefix sums in place, the total to *total_out.  Thread t owns a run of ceil(n / 256) counts.
__global__ void __launch_bounds__(PHX_SEL_BLOCK) k_adaptive_scan(uint32_t* __restrict__ counts, uint32_t n, uint32_t* __restrict__ total_out) {
  __shared__ uint32_t run_sum[PHX_SEL_BLOCK];
  const uint32_t per = (n + PHX_SEL_BLOCK - 1) / PHX_SEL_BLOCK;
  const uint32_t i0 = min(threadIdx.x * per, n), i1 = min(i0 + per, n);
  uint32_t s = 0u;
  for (uint32_t i = i0; i < i1; ++i) s += counts[i];
  run_sum[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0u) {
    uint32_t t = 0u;
    for (uint32_t w = 0; w < PHX_SEL_BLOCK; ++w) { const uint32_t c = run_sum[w]; run_sum[w] = t; t += c; }
    *total_out = t;
  }
  __syncthreads();
  uint32_t t = run_sum[threadIdx.x];
  for (uint32_t i = i0; i < i1; ++i) { const uint32_t c = counts[i]; counts[i] = t; t += c; }
}
__global__ void __launch_bounds__(PHX_SEL_BLOCK) k_adaptive_write(AdaptiveArgs A, const uint32_t* __restrict__ block_offsets, uint32_t* __restrict__ survivors) {
  const uint32_t i = blockIdx.x * PHX_SEL_BLOCK + threadIdx.x;
  uint32_t row, total;
  const bool alive = adaptive_survives(A, i, row);
  const uint32_t rank = block_rank(alive, total);
  if (alive) survivors[block_offsets[blockIdx.x] + rank] = row;  // < the total of the scan <= num_active
  else if (i < A.num_active) {  // the row stops: rescaled once, and it says how many samples it took
    float* r = A.acc + (size_t)row * A.xstride;
#pragma unroll
    for (uint32_t c = 0; c < 3u; ++c) {
      r[c] = (float)((double)r[c] * A.k);
      r[A.m2_offset + c] = (float)(((double)r[A.m2_offset + c] * A.k) * A.k);
    }
    r[A.samples_offset] = A.n;
  }
}
// Rows between home order and working order, a thread per float so that the working side coalesces: working row w is home row idx[w].
// to_home == 0: home -> working, the pixel words (pix_xy) with them; 1: working -> home (the pixel words never change).
__global__ void __launch_bounds__(PHX_SEL_BLOCK) k_adaptive_move(float* __restrict__ home, float* __restrict__ work, const uint32_t* __restrict__ home_xy,
                                                                 uint32_t* __restrict__ work_xy, const uint32_t* __restrict__ idx, uint32_t n, uint32_t xstride, int to_home) {
  const size_t t = (size_t)blockIdx.x * PHX_SEL_BLOCK + threadIdx.x;
  const size_t w = t / xstride; const uint32_t c = (uint32_t)(t % xstride);
  if (w >= n) return;
  const size_t h = idx[w];
  if (to_home) home[h * xstride + c] = work[w * xstride + c];
  else {
    work[w * xstride + c] = home[h * xstride + c];
    if (c == 0u) work_xy[w] = home_xy[h];
  }
}
// channel "samples" of the rows idx[0 .. n) (nullptr: rows 0 .. n - 1): the pixels that took every sample of the frame
__global__ void __launch_bounds__(PHX_SEL_BLOCK) k_adaptive_mark(float* __restrict__ acc, uint32_t xstride, uint32_t samples_offset, const uint32_t* __restrict__ idx,
                                                                 uint32_t n, float value) {
  const uint32_t i = blockIdx.x * PHX_SEL_BLOCK + threadIdx.x;
  if (i >= n) return;
  acc[(size_t)(idx ? idx[i] : i) * xstride + samples_offset] = value;
}

// ---- KAT kernels ------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) k_bsdf_f(const DevMaterial* mat, uint32_t n, const float* n3, const float* wi3, const float* wo3, float* f3) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const v3 nn(n3[3 * i], n3[3 * i + 1], n3[3 * i + 2]), view(wo3[3 * i], wo3[3 * i + 1], wo3[3 * i + 2]);  // f(wi = to the light, wo = hits.wi)
  const v3 f = bsdf_f<false, 8, true>(*mat, nn, v3(wi3[3 * i], wi3[3 * i + 1], wi3[3 * i + 2]), view);
  f3[3 * i] = f.x; f3[3 * i + 1] = f.y; f3[3 * i + 2] = f.z;
}
__global__ void __launch_bounds__(64) k_bsdf_sample(const DevMaterial* mat, uint32_t n, const float* n3, const float* wi3, const float* u2,
                              float* wo3, float* f3, float* pdf, uint32_t* flags) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  v3 wo; float p; uint32_t fl;
  const v3 nn(n3[3 * i], n3[3 * i + 1], n3[3 * i + 2]), view(wi3[3 * i], wi3[3 * i + 1], wi3[3 * i + 2]);  // sample(u, wi = hits.wi)
  v3 f = bsdf_sample<false, 8, true>(*mat, nn, u2[2 * i], u2[2 * i + 1], view, wo, p, fl);
  if (p == 0.0f) { wo = v3(0.0f); f = v3(0.0f); fl = 0; }
  wo3[3 * i] = wo.x; wo3[3 * i + 1] = wo.y; wo3[3 * i + 2] = wo.z;
  f3[3 * i] = f.x; f3[3 * i + 1] = f.y; f3[3 * i + 2] = f.z; pdf[i] = p; flags[i] = fl;
}

__global__ void __launch_bounds__(64) k_environment_lookup(const DevTexture* textures, const float4* texels, uint32_t tex, uint32_t mapping, float ex, float ey,
                                                           float ez, uint32_t n, const float* dirs, float* rgb) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const v3 c = env_emission(textures, texels, tex, mapping, v3(dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]), v3(ex, ey, ez));
  rgb[3 * i] = c.x; rgb[3 * i + 1] = c.y; rgb[3 * i + 2] = c.z;
}

__global__ void __launch_bounds__(64) k_texture_lookup(const DevTexture* textures, const float4* texels, uint32_t tex, uint32_t n, const float* st, float* rgb) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const v3 c = tex_lookup(textures, texels, tex, st[2 * i], st[2 * i + 1]);
  rgb[3 * i] = c.x; rgb[3 * i + 1] = c.y; rgb[3 * i + 2] = c.z;
}

// phx_dev_light_sample: the light sample of k_shade_g's next-event block (light_pick_env, triangle_t::sample, P).  On a scene with SC_LIGHTS_ENV
// the pick is over num_lights + 1 entries: an environment pick answers light = num_lights, tri = 0xffffffff and zeros, and reads no light record.
__global__ void __launch_bounds__(64) k_light_sample(DevScene sc, uint32_t n, const float* u3, uint32_t* light, uint32_t* tri, float* bary, float* P3, float* pdf) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float pick = u3[3 * i], lu = u3[3 * i + 1], lv = u3[3 * i + 2];
  uint32_t l, ti, lt; float remapped;
  light_pick_env(sc, pick, lu, l, ti, lt, remapped);
  const bool env = l == sc.num_lights;
  float bu = 0.0f, bv = 0.0f; v3 P(0.0f);
  if (!env) {
    const float x = sqrtf(remapped);
    bu = 1 - x; bv = lv * x;                 // triangle_t::sample, mesh.cpp:318-324
    const DevLightTri& LT = sc.light_tris[lt];
    const v3 la(LT.ax, LT.ay, LT.az), lb(LT.bx, LT.by, LT.bz), lc(LT.cx, LT.cy, LT.cz);
    P = bu * la + bv * lb + (1 - bu - bv) * lc;
  }
  light[i] = l; tri[i] = env ? 0xffffffffu : ti; bary[2 * i] = bu; bary[2 * i + 1] = bv;
  P3[3 * i] = P.x; P3[3 * i + 1] = P.y; P3[3 * i + 2] = P.z;
  pdf[i] = env ? 0.0f : sc.lights[l].lpdf;
}

// phx_dev_light_emission: the same light sample, then light_emission as k_shade_g<.., TEX>'s next-event block runs it (an environment pick: zeros)
__global__ void __launch_bounds__(64) k_light_emission(DevScene sc, uint32_t n, const float* u3, float* st2, float* e3) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float pick = u3[3 * i], lu = u3[3 * i + 1], lv = u3[3 * i + 2];
  uint32_t l, ti, lt; float remapped;
  light_pick_env(sc, pick, lu, l, ti, lt, remapped);
  v3 le(0.0f); float2 st = make_float2(0.0f, 0.0f);
  if (l != sc.num_lights) {
    const float x = sqrtf(remapped);
    const float bu = 1 - x, bv = lv * x;
    const DevLight& L = sc.lights[l];
    le = v3(L.ex, L.ey, L.ez);
    if (sc.tex && sc.tex->any_emit_tex) le = light_emission(sc.tex->elem_uv, sc.tex->textures, sc.tex->texels, emit_tex_table(sc), L, sc.light_tris[lt], bu, bv, st);
  }
  st2[2 * i] = st.x; st2[2 * i + 1] = st.y;
  e3[3 * i] = le.x; e3[3 * i + 1] = le.y; e3[3 * i + 2] = le.z;
}
// phx_dev_environment_sample: light_pick, env_sample and env_emission as k_shade_g<.., ENV>'s next-event block runs them
__global__ void __launch_bounds__(64) k_environment_sample(DevScene sc, float ex, float ey, float ez, uint32_t n, const float* u3, uint32_t* light, uint32_t* texel,
                                                           float* st2, float* dir3, float* pdf, float* e3) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const float pick = u3[3 * k], lu = u3[3 * k + 1], lv = u3[3 * k + 2];
  uint32_t l, ti, lt; float remapped;
  light_pick_env(sc, pick, lu, l, ti, lt, remapped);
  uint32_t i = 0u, j = 0u; float s = 0.0f, t = 0.0f, p = 0.0f; v3 d(0.0f), le(0.0f);
  if (l == sc.num_lights) {
    const DevTexScene& tx = *sc.tex;
    const DevTexture ET = tx.textures[tx.env_tex];
    if (env_sample(tx.env_cdf, ET.width, ET.height, tx.env_mapping, tx.env_p, lu, lv, i, j, s, t, d, p))
      le = env_emission(tx.textures, tx.texels, tx.env_tex, tx.env_mapping, d, v3(ex, ey, ez));
  }
  light[k] = l; texel[2 * k] = i; texel[2 * k + 1] = j; st2[2 * k] = s; st2[2 * k + 1] = t;
  dir3[3 * k] = d.x; dir3[3 * k + 1] = d.y; dir3[3 * k + 2] = d.z; pdf[k] = p;
  e3[3 * k] = le.x; e3[3 * k + 1] = le.y; e3[3 * k + 2] = le.z;
}

// phx_dev_lobe_weights: lobe_weight_of as k_shade_g<.., TEX, ., MASK> (TEXTURED) or k_shade_g<PERHIT> (scenes without a texture table) resolves it
template <bool TEXTURED>
__global__ void __launch_bounds__(64) k_lobe_weights(const DevMaterial* mat, const DevTexture* textures, const float4* texels, const uint32_t* lobe_tex, uint32_t n,
                                                     const float* n3, const float* wi3, const float* st, float* w, uint32_t* kept) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const DevMaterial& m = *mat;
  const v3 nn(n3[3 * i], n3[3 * i + 1], n3[3 * i + 2]), view(wi3[3 * i], wi3[3 * i + 1], wi3[3 * i + 2]);
  TexHit th{};
  if constexpr (TEXTURED) th = TexHit{textures, texels, lobe_tex, st[2 * i], st[2 * i + 1]};
  uint32_t keep = 0u;
  for (uint32_t k = 0; k < 8u; ++k) {
    v3 lw(0.0f);
    if (k < m.num_lobes && lobe_weight_of<true, TEXTURED, TEXTURED>(m, k, m.lobes[k], nn, view, lw, th)) keep |= 1u << k;
    float* o = w + 3 * (8 * (size_t)i + k);
    o[0] = lw.x; o[1] = lw.y; o[2] = lw.z;
  }
  kept[i] = keep;
}

namespace {
__global__ void k_build_shade_recs(const TriRec* __restrict__ tris, const uint32_t* __restrict__ elem_of_prim, float4* __restrict__ elem_shade, uint32_t n) {
  const uint32_t p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const uint32_t e = elem_of_prim[p];
  if (e == 0xffffffffu) return;
  const TriRec T = tris[e];
  const v3 gn = shading_normal(DevScene{}, e, false, v3(T.e0x, T.e0y, T.e0z), v3(T.e1x, T.e1y, T.e1z), 0.0f, 0.0f);  // the flat face's normal, by the expression the shade kernels used per hit
  elem_shade[e] = make_float4(gn.x, gn.y, gn.z, u2f(T.material));
}
__global__ void k_permute_normals(const float* __restrict__ prim_normals, const uint32_t* __restrict__ elem_of_prim, float* __restrict__ elem_normals, uint32_t n) {
  const uint32_t p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const uint32_t e = elem_of_prim[p];
  if (e == 0xffffffffu) return;
#pragma unroll
  for (int k = 0; k < 9; ++k) elem_normals[9 * (size_t)e + k] = prim_normals[9 * (size_t)p + k];
}
__global__ void k_permute_uvs(const float2* __restrict__ prim_uv, const uint32_t* __restrict__ elem_of_prim, float2* __restrict__ elem_uv, uint32_t n) {
  const uint32_t p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const uint32_t e = elem_of_prim[p];
  if (e == 0xffffffffu) return;
#pragma unroll
  for (int k = 0; k < 3; ++k) elem_uv[3 * (size_t)e + k] = prim_uv[3 * (size_t)p + k];
}
__global__ void k_remap_light_tris(DevLightTri* __restrict__ lt, uint32_t n, const uint32_t* __restrict__ elem_of_prim) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i < n && lt[i].smooth) lt[i].prim = elem_of_prim[lt[i].prim];
}
// (every primitive has a record: both builders make each of the n primitives, zero-area ones included, the one triangle of a leaf and write
// elem_of_prim[p] with it -- bvh_build.cpp: the collapse's leaf children, bvh_gpu.hip: k_collapse -- which k_remap_light_tris relies on too)
__global__ void k_remap_flat_light_tris(DevLightTri* __restrict__ lt, uint32_t n, const uint32_t* __restrict__ elem_of_prim) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i < n && !lt[i].smooth) lt[i].prim = elem_of_prim[lt[i].prim];
}
}  // namespace

// ---- launches ---------------------------------------------------------------------------------------
void launch_begin_pass(hipStream_t stream, const PassBuffers& pb, uint32_t num_samples) {
  hipLaunchKernelGGL(k_begin_pass, dim3(1), dim3(1), 0, stream, pb, num_samples);
}
void launch_build_shade_recs(hipStream_t stream, const TriRec* tris, const uint32_t* elem_of_prim, float4* elem_shade, uint32_t num_prims) {
  if (num_prims) hipLaunchKernelGGL(k_build_shade_recs, dim3((num_prims + 255) / 256), dim3(256), 0, stream, tris, elem_of_prim, elem_shade, num_prims);
}
void launch_permute_normals(hipStream_t stream, const float* prim_normals, const uint32_t* elem_of_prim, float* elem_normals, uint32_t num_prims) {
  if (num_prims) hipLaunchKernelGGL(k_permute_normals, dim3((num_prims + 255) / 256), dim3(256), 0, stream, prim_normals, elem_of_prim, elem_normals, num_prims);
}
void launch_permute_uvs(hipStream_t stream, const float2* prim_uv, const uint32_t* elem_of_prim, float2* elem_uv, uint32_t num_prims) {
  if (num_prims) hipLaunchKernelGGL(k_permute_uvs, dim3((num_prims + 255) / 256), dim3(256), 0, stream, prim_uv, elem_of_prim, elem_uv, num_prims);
}
void launch_remap_light_tris(hipStream_t stream, DevLightTri* light_tris, uint32_t num_light_tris, const uint32_t* elem_of_prim) {
  if (num_light_tris) hipLaunchKernelGGL(k_remap_light_tris, dim3((num_light_tris + 255) / 256), dim3(256), 0, stream, light_tris, num_light_tris, elem_of_prim);
}
void launch_remap_flat_light_tris(hipStream_t stream, DevLightTri* light_tris, uint32_t num_light_tris, const uint32_t* elem_of_prim) {
  if (num_light_tris) hipLaunchKernelGGL(k_remap_flat_light_tris, dim3((num_light_tris + 255) / 256), dim3(256), 0, stream, light_tris, num_light_tris, elem_of_prim);
}
void launch_film(hipStream_t stream, const PassBuffers& pb, uint32_t num_samples, float inv) {
  hipLaunchKernelGGL(k_film, dim3((pb.num_pixels + PHX_FILM_PIX - 1) / PHX_FILM_PIX), dim3(256), 0, stream, pb, num_samples, inv);
}
void launch_film_moments(hipStream_t stream, const PassBuffers& pb, uint32_t num_samples, float inv, uint32_t samples_done, uint32_t m2_offset) {
  hipLaunchKernelGGL(k_film_moments, dim3((pb.num_pixels + PHX_FILM_PIX - 1) / PHX_FILM_PIX), dim3(256), 0, stream, pb, num_samples, inv, samples_done, m2_offset);
}
void launch_scatter_film(hipStream_t stream, const PassBuffers& pb, float* device_film, uint32_t film_width) {
  hipLaunchKernelGGL(k_scatter_film, dim3(blocks_for(pb.num_pixels)), dim3(PHX_BLOCK), 0, stream, pb, device_film, film_width);
}
void launch_adaptive_select(hipStream_t stream, const AdaptiveArgs& A, uint32_t* block_scratch, uint32_t* survivors, uint32_t* total_out) {
  const uint32_t nblocks = (A.num_active + PHX_SEL_BLOCK - 1) / PHX_SEL_BLOCK;
  hipLaunchKernelGGL(k_adaptive_count, dim3(nblocks), dim3(PHX_SEL_BLOCK), 0, stream, A, block_scratch);
  hipLaunchKernelGGL(k_adaptive_scan, dim3(1), dim3(PHX_SEL_BLOCK), 0, stream, block_scratch, nblocks, total_out);
  hipLaunchKernelGGL(k_adaptive_write, dim3(nblocks), dim3(PHX_SEL_BLOCK), 0, stream, A, block_scratch, survivors);
}
void launch_adaptive_move(hipStream_t stream, float* home, float* work, const uint32_t* home_xy, uint32_t* work_xy, const uint32_t* idx, uint32_t n,
                          uint32_t xstride, int to_home) {
  const size_t nfl = (size_t)n * xstride;
  if (nfl) hipLaunchKernelGGL(k_adaptive_move, dim3((uint32_t)((nfl + PHX_SEL_BLOCK - 1) / PHX_SEL_BLOCK)), dim3(PHX_SEL_BLOCK), 0, stream, home, work, home_xy, work_xy, idx, n, xstride, to_home);
}
void launch_adaptive_mark(hipStream_t stream, float* acc, uint32_t xstride, uint32_t samples_offset, const uint32_t* idx, uint32_t n, float value) {
  if (n) hipLaunchKernelGGL(k_adaptive_mark, dim3((n + PHX_SEL_BLOCK - 1) / PHX_SEL_BLOCK), dim3(PHX_SEL_BLOCK), 0, stream, acc, xstride, samples_offset, idx, n, value);
}
void launch_bsdf_f(hipStream_t stream, const DevMaterial* mat, uint32_t n, const float* n3, const float* wi3, const float* wo3, float* f3) {
  hipLaunchKernelGGL(k_bsdf_f, dim3((n + 63) / 64), dim3(64), 0, stream, mat, n, n3, wi3, wo3, f3);
}
void launch_bsdf_sample(hipStream_t stream, const DevMaterial* mat, uint32_t n, const float* n3, const float* wi3, const float* u2,
                        float* wo3, float* f3, float* pdf, uint32_t* flags) {
  hipLaunchKernelGGL(k_bsdf_sample, dim3((n + 63) / 64), dim3(64), 0, stream, mat, n, n3, wi3, u2, wo3, f3, pdf, flags);
}
void launch_environment_lookup(hipStream_t stream, const DevTexture* textures, const float4* texels, uint32_t tex, uint32_t mapping, float ex, float ey, float ez,
                               uint32_t n, const float* dirs, float* rgb) {
  hipLaunchKernelGGL(k_environment_lookup, dim3((n + 63) / 64), dim3(64), 0, stream, textures, texels, tex, mapping, ex, ey, ez, n, dirs, rgb);
}
void launch_lobe_weights(hipStream_t stream, const DevMaterial* mat, const DevTexture* textures, const float4* texels, const uint32_t* lobe_tex, uint32_t n,
                         const float* n3, const float* wi3, const float* st, float* w, uint32_t* kept) {
  if (textures) hipLaunchKernelGGL(k_lobe_weights<true>, dim3((n + 63) / 64), dim3(64), 0, stream, mat, textures, texels, lobe_tex, n, n3, wi3, st, w, kept);
  else hipLaunchKernelGGL(k_lobe_weights<false>, dim3((n + 63) / 64), dim3(64), 0, stream, mat, textures, texels, lobe_tex, n, n3, wi3, st, w, kept);
}
void launch_light_sample(hipStream_t stream, const DevScene& sc, uint32_t n, const float* u3, uint32_t* light, uint32_t* tri, float* bary, float* P, float* pdf) {
  hipLaunchKernelGGL(k_light_sample, dim3((n + 63) / 64), dim3(64), 0, stream, sc, n, u3, light, tri, bary, P, pdf);
}
void launch_light_emission(hipStream_t stream, const DevScene& sc, uint32_t n, const float* u3, float* st, float* e) {
  hipLaunchKernelGGL(k_light_emission, dim3((n + 63) / 64), dim3(64), 0, stream, sc, n, u3, st, e);
}
void launch_environment_sample(hipStream_t stream, const DevScene& sc, float ex, float ey, float ez, uint32_t n, const float* u3, uint32_t* light, uint32_t* texel,
                               float* st, float* dir, float* pdf, float* e) {
  hipLaunchKernelGGL(k_environment_sample, dim3((n + 63) / 64), dim3(64), 0, stream, sc, ex, ey, ez, n, u3, light, texel, st, dir, pdf, e);
}
void launch_texture_lookup(hipStream_t stream, const DevTexture* textures, const float4* texels, uint32_t tex, uint32_t n, const float* st, float* rgb) {
  hipLaunchKernelGGL(k_texture_lookup, dim3((n + 63) / 64), dim3(64), 0, stream, textures, texels, tex, n, st, rgb);
}

}  // namespace phx
