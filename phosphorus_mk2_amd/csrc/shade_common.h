// shade_common.h — the device functions that two or more kernel families share (trace.hip, shade_lambert.hip, shade_general.hip,
// film_hooks.hip; kernels.h has the map of kernels to files).  Included by those four only: everything here is __device__ __forceinline__
// (host helpers static inline), so each translation unit inlines its own copy and a kernel's code does not depend on what else shares
// its file.  A change here can move every family's instruction stream: prove with scripts/asm_compare.py that it did not.
//
//   camera_ray  camera::perspective_kernel_t (reference src/kernels/cpu/camera.hpp:80-159) + spt::state_t::reset: a device
//               function — primary rays are rebuilt on the fly by k_trace_primary and the first k_shade of a pass, never stored
#pragma once
#include "kernels.h"
#include "../../include/phx_xpu.h"  // PHX_SHADE_*: the bits of phx_stats::shade_kernels

#include <algorithm>
#include <cstddef>
#include <cstdlib>
#include <type_traits>

namespace phx {

#define PHX_BLOCK 256
#define PHX_UNI(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))  /* wave-uniform by construction: keep it in an SGPR */

__device__ __forceinline__ uint32_t f2u(float f) { return __float_as_uint(f); }
__device__ __forceinline__ float u2f(uint32_t u) { return __uint_as_float(u); }

// ---- camera rays ------------------------------------------------------------------------------------
// camera::perspective_kernel_t (kernels/cpu/camera.hpp:80-159).  Primary rays are never stored: the first
// k_trace of a pass and the first k_shade both rebuild the ray of path `path` from the pixel table and the jitter table
// (about 40 instructions) instead of writing and re-reading 32 B per path.
// LENS (camera_t::aperture_radius != 0, set by the Blender importer when depth of field is on): camera.hpp:140-147 and
// simd::concentric_sample_disc (math/simd/sampling.hpp:8-32) AS WRITTEN (SURVEY A-21): the raw samples in [0, 1) are mapped, not 2 u - 1;
// the constants named pi_o_2 / pi_o_4 hold 2 / pi and 4 / pi; select(m, l, r) returns r where m is set (float8.hpp:103-105).  The two lens
// samples are the spare dimensions 6 and 7 of the path's step 0 (the reference: a table of 1024 per sample index, sampling.cpp:108-109).
// A sample with a zero coordinate gives a non-finite angle and a NaN ray, which hits nothing, there and here.
template <bool LENS>
__device__ __forceinline__ void camera_ray(const DevScene& sc, const PassBuffers& pb, uint32_t path, uint32_t sample0, v3& p, v3& w) {
  const uint32_t pix = path / pb.num_samples, s = path - pix * pb.num_samples;  // pixel-major: a wave = 64 samples of one pixel
  const uint32_t xy = pb.pix_xy[pix];
  const float sx = (float)(xy & 0xffffu), sy = (float)(xy >> 16);
  const float2 jit = pb.jitter[sample0 + s];
  const float ndcy = 0.5f - (-0.5f + sy) * sc.stepy;
  const float ndcx = (-0.5f + sx) * sc.stepx - 0.5f;
  v3 d(jit.x, jit.y, -1.0f);
  d.x = (ndcx + d.x * sc.stepx) * sc.ratio * sc.zoom;
  d.y = (ndcy + d.y * sc.stepy) * sc.zoom;
  const float ool = 1.0f / sqrtf(sdot(d, d));
  d = v3(d.x * ool, d.y * ool, d.z * ool);
  const float* M = sc.cam_m;
  if constexpr (LENS) {
    const uint32_t key = path_key(pb.seed, (xy >> 16) * sc.width + (xy & 0xffffu), sample0 + s);
    const float ux = draw_f32(key, DIM_LENS_U), uy = draw_f32(key, DIM_LENS_V);
    const float c2 = (float)(2.0f / M_PI), c4 = (float)(4.0f / M_PI);
    const bool x_gt_y = fabsf(ux) > fabsf(uy);
    const float r = x_gt_y ? uy : ux;
    const float theta1 = c4 * (uy / ux), theta2 = c2 - c4 * (ux / uy);
    const sincosf_t sc_t = sincosf_(x_gt_y ? theta2 : theta1);
    const float lx = (r * sc_t.c) * sc.aperture_radius, ly = (r * sc_t.s) * sc.aperture_radius;
    const float ft = fabsf(sc.focal_distance / d.z);
    d = v3(d.x * ft - lx, d.y * ft - ly, d.z * ft - 0.0f);
    const float ool2 = 1.0f / sqrtf(sdot(d, d));
    d = v3(d.x * ool2, d.y * ool2, d.z * ool2);
    { float t = lx * M[0]; t = fmaf(ly, M[4], t); t = fmaf(0.0f, M[8], t); p.x = t + M[12]; }
    { float t = lx * M[1]; t = fmaf(ly, M[5], t); t = fmaf(0.0f, M[9], t); p.y = t + M[13]; }
    { float t = lx * M[2]; t = fmaf(ly, M[6], t); t = fmaf(0.0f, M[10], t); p.z = t + M[14]; }
  } else {
  { float t = 0.0f * M[0]; t = fmaf(0.0f, M[4], t); t = fmaf(0.0f, M[8], t); p.x = t + M[12]; }
  { float t = 0.0f * M[1]; t = fmaf(0.0f, M[5], t); t = fmaf(0.0f, M[9], t); p.y = t + M[13]; }
  { float t = 0.0f * M[2]; t = fmaf(0.0f, M[6], t); t = fmaf(0.0f, M[10], t); p.z = t + M[14]; }
  }
  { float t = d.x * M[0]; t = fmaf(d.y, M[4], t); w.x = fmaf(d.z, M[8], t); }
  { float t = d.x * M[1]; t = fmaf(d.y, M[5], t); w.y = fmaf(d.z, M[9], t); }
  { float t = d.x * M[2]; t = fmaf(d.y, M[6], t); w.z = fmaf(d.z, M[10], t); }
}

__device__ __forceinline__ void zero_cursors(uint32_t* counters) {
#pragma unroll
  for (uint32_t k = 0; k < 2u * CNT_SEGS; ++k) counters[CNT_CURSOR + k * CNT_STRIDE] = 0;
}

// ---- shade + next-event estimation + integrate ------------------------------------------------------
__device__ __forceinline__ v3 shading_normal(const DevScene& sc, uint32_t elem /* pool index of the triangle record */, bool smooth, const v3& e0, const v3& e1, float u, float v) {
  if (smooth) {  // mesh_t::shading_parameters, src/mesh.cpp:187-199
    const float w = 1 - u - v;
    const float* pn = sc.elem_normals + 9 * (size_t)elem;
    const v3 n0(pn[0], pn[1], pn[2]), n1(pn[3], pn[4], pn[5]), n2(pn[6], pn[7], pn[8]);
    return normalize_inplace(w * n0 + u * n1 + v * n2);
  }
  return normalize_inplace(cross(e0, e1));  // (v1-v0) x (v2-v0), never flipped (mesh.cpp:201-215)
}
// k_shade_g: the three vertex normals of the hit's pool element are requested TOGETHER WITH its shade record — whether the face is smooth
// is a bit of that record — and used or dropped when it has landed (flat faces of a scene with smooth ones pay a 36-byte gather for nothing;
// scenes without smooth faces have no table and no request)
struct VertexNormals { v3 n0, n1, n2; };
__device__ __forceinline__ VertexNormals request_vertex_normals(const DevScene& sc, uint32_t elem) {
  VertexNormals N{v3(0.0f), v3(0.0f), v3(0.0f)};
  if (sc.elem_normals) {
    const float* pn = sc.elem_normals + 9 * (size_t)elem;
    N.n0 = v3(pn[0], pn[1], pn[2]); N.n1 = v3(pn[3], pn[4], pn[5]); N.n2 = v3(pn[6], pn[7], pn[8]);
  }
  return N;
}
__device__ __forceinline__ v3 shading_normal(const VertexNormals& N, bool smooth, const v3& geometric /* DevScene::elem_shade */, float u, float v) {
  if (smooth) { const float w = 1 - u - v; return normalize_inplace(w * N.n0 + u * N.n1 + v * N.n2); }  // the same expression as above
  return geometric;
}

// k_shade_g<.., TEX>: the three corner UVs of the hit's pool element, requested with its shade record like the vertex normals, and the hit's
// (s, t) by mesh_t::shading_parameters (src/mesh.cpp:177-181,239-257): w = (1 - u) - v, st = (w * uv0 + u * uv1) + v * uv2
struct CornerUVs { float2 a, b, c; };
__device__ __forceinline__ CornerUVs request_corner_uvs(const float2* elem_uv, uint32_t elem) {
  const float2* p = elem_uv + 3 * (size_t)elem;
  return CornerUVs{p[0], p[1], p[2]};
}
__device__ __forceinline__ float2 hit_st(const CornerUVs& C, float u, float v) {
  const float w = (1 - u) - v;
  return make_float2((w * C.a.x + u * C.b.x) + v * C.c.x, (w * C.a.y + u * C.b.y) + v * C.c.y);
}

__device__ __forceinline__ float luminance(const v3& c) {  // color::y, src/utils/color.hpp:13-16
  return (float)0.212671 * c.x + (float)0.715160 * c.y + (float)0.072169 * c.z;
}

// ---- next-event estimation's pick (light_sampler_t, spt.hpp:95-149; area_light_t::sample, light.cpp:55-67) ---------------------------------
// The light uniformly, then a triangle inside it and the draw remapped into that triangle.  PHX_LIGHTS_REFERENCE: the triangle by index, as
// the reference does with its search commented out (light.cpp:30-53) -- the pdf 1/area it reports is then the true density only for lights of
// equal triangles.  PHX_LIGHTS_BY_AREA (SC_LIGHTS_BY_AREA, a wave-uniform branch on a kernel argument): by the area CDF that follows the light
// table, the rule of include/phx_xpu.h.  Used by k_shade_g and by phx_dev_light_sample; k_shade<1/2> keep their own copy of the reference
// pick (a BY_AREA scene never runs them).
// PHX_LIGHT_SELECT_BY_POWER (SC_LIGHTS_BY_POWER, wave-uniform likewise): the light itself by the selection table pcdf, which sits between the
// light records and the area CDF (num_lights floats, padded to whole records); DevLight::lpdf then holds (1 / area) * p_l.
__device__ __forceinline__ const float* light_pcdf(const DevScene& sc) { return reinterpret_cast<const float*>(sc.lights + sc.num_lights); }
__device__ __forceinline__ const float* light_cdf(const DevScene& sc) {
  const uint32_t pcdf_records = (sc.any_tex & SC_LIGHTS_BY_POWER) ? (sc.num_lights + 7u) >> 3 : 0u;  // 8 floats per 32-byte record
  return reinterpret_cast<const float*>(sc.lights + sc.num_lights + pcdf_records);
}
// the smallest i in [0, last] with u < cdf[i], or last: reads cdf[0 .. last - 1] only.  (The four searches of light_pick / light_pick_env; every
// k_shade_g body is the same with it as with the loops written out, profiles/r14_asm_per_symbol.txt.  env_cdf_search is not folded in: its 17-step bound is its contract.)
__device__ __forceinline__ uint32_t cdf_search(const float* cdf, uint32_t last, float u) {
  uint32_t lo = 0, hi = last;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (u < cdf[mid]) hi = mid; else lo = mid + 1;
  }
  return lo;
}
__device__ __forceinline__ void light_pick(const DevScene& sc, float pick, float lu, uint32_t& l, uint32_t& ti, uint32_t& lt, float& remapped) {
  if (sc.any_tex & SC_LIGHTS_BY_POWER) {
    l = cdf_search(light_pcdf(sc), sc.num_lights - 1, pick);  // monotone, pcdf[num_lights - 1] == 1
  } else {
    const float nlf = (float)sc.num_lights;
    l = (uint32_t)floorf(pick * nlf);
    if (l > sc.num_lights - 1) l = sc.num_lights - 1;
  }
  const uint32_t ltris = sc.lights[l].num_tris;
  if (sc.any_tex & SC_LIGHTS_BY_AREA) {
    const float* cdf = light_cdf(sc) + sc.lights[l].first_tri;  // cdf[i] = (area_0 + ... + area_i) / area, monotone, cdf[ltris - 1] == 1
    ti = cdf_search(cdf, ltris - 1, lu);
    const float below = ti ? cdf[ti - 1] : 0.0f;
    remapped = fminf((lu - below) / (cdf[ti] - below), 1.0f - FLT_EPSILON);
  } else {
    const float numf = (float)ltris;
    ti = (uint32_t)floorf(lu * numf);  // uniform by index (light.cpp:55), pdf = 1/area
    if (ti > ltris - 1) ti = ltris - 1;
    remapped = fminf(lu * numf - (float)ti, 1.0f - FLT_EPSILON);
  }
  lt = sc.lights[l].first_tri + ti;
}

// light_pick where the scene may have PHX_LIGHT_INCLUDE_ENVIRONMENT (SC_LIGHTS_ENV, a wave-uniform branch; always with SC_LIGHTS_BY_POWER and
// SC_LIGHTS_BY_AREA): pcdf has one more entry, the environment's, so the area CDF starts one entry's padding later, and a pick that lands there
// returns l == num_lights with ti = lt = 0 and remapped = 0 and reads no light record (there is none: the caller samples the image, env_sample).
// Used by the ENV instantiations of k_shade_g and by the hooks' kernels (for every scene: the fall-back below); light_pick and its callers are as they were.
__device__ __forceinline__ void light_pick_env(const DevScene& sc, float pick, float lu, uint32_t& l, uint32_t& ti, uint32_t& lt, float& remapped) {
  if (!(sc.any_tex & SC_LIGHTS_ENV)) { light_pick(sc, pick, lu, l, ti, lt, remapped); return; }
  l = cdf_search(light_pcdf(sc), sc.num_lights, pick);  // monotone, pcdf[num_lights] == 1
  if (l == sc.num_lights) { ti = 0u; lt = 0u; remapped = 0.0f; return; }
  const float* cdf = reinterpret_cast<const float*>(sc.lights + sc.num_lights + ((sc.num_lights + 8u) >> 3)) + sc.lights[l].first_tri;
  ti = cdf_search(cdf, sc.lights[l].num_tris - 1, lu);  // as light_pick searches it
  const float below = ti ? cdf[ti - 1] : 0.0f;
  remapped = fminf((lu - below) / (cdf[ti] - below), 1.0f - FLT_EPSILON);
  lt = sc.lights[l].first_tri + ti;
}

// ---- the environment's sample (PHX_LIGHT_INCLUDE_ENVIRONMENT; the rule is stated in include/phx_xpu.h) ---------------------------------------
// The smallest i with u < cdf[i], or n - 1: a binary search of at most 17 steps (n <= 65536 needs 16) that reads cdf[0 .. n - 2] only; a NaN
// draw compares false everywhere and ends at n - 1.
__device__ __forceinline__ uint32_t env_cdf_search(const float* cdf, uint32_t n, float u) {
  uint32_t lo = 0u, hi = n - 1u;
  for (int step = 0; step < 17 && lo < hi; ++step) {
    const uint32_t mid = (lo + hi) >> 1;
    if (u < cdf[mid]) hi = mid; else lo = mid + 1u;
  }
  return min(lo, n - 1u);
}
// The texel (i, j) of the W x H image by the tables env_cdf = mcdf[H], ccdf[H][W], the point (s, t) inside it, its direction d and
// pdf = p_env * pdf_omega.  -> false: no shadow ray (sin(pi t) <= 0, or pdf not finite and positive; pdf is then 0).  Used by k_shade_g<.., ENV>
// and by phx_dev_environment_sample.  sin(pi t) = cos(pi (0.5 - t)) is the Taylor polynomial of the header, Horner in binary64, rounded once: no
// library function enters the density, so the tests restate it bit for bit; d goes through sinf / cosf and is held to a tolerance.
__device__ __forceinline__ float env_sin_pi_t(float t) {
  const double y = kPiD * (0.5 - (double)t), y2 = y * y;
  double c = 1.0 / 2432902008176640000.0;  // 1 / 20!
  c = 1.0 / 6402373705728000.0 - y2 * c;   // 1 / 18! ...
  c = 1.0 / 20922789888000.0 - y2 * c;
  c = 1.0 / 87178291200.0 - y2 * c;
  c = 1.0 / 479001600.0 - y2 * c;
  c = 1.0 / 3628800.0 - y2 * c;
  c = 1.0 / 40320.0 - y2 * c;
  c = 1.0 / 720.0 - y2 * c;
  c = 1.0 / 24.0 - y2 * c;
  c = 1.0 / 2.0 - y2 * c;
  c = 1.0 - y2 * c;
  return (float)c;
}
__device__ __forceinline__ bool env_sample(const float* env_cdf, uint32_t W, uint32_t H, uint32_t mapping, float p_env, float lu, float lv, uint32_t& i, uint32_t& j,
                                           float& s, float& t, v3& d, float& pdf) {
  j = env_cdf_search(env_cdf, H, lu);
  const float rlo = j ? env_cdf[j - 1u] : 0.0f;
  const float prow = env_cdf[j] - rlo;
  const float ru = fminf((lu - rlo) / prow, 1.0f - FLT_EPSILON);
  const float* row = env_cdf + H + (size_t)j * W;
  i = env_cdf_search(row, W, lv);
  const float clo = i ? row[i - 1u] : 0.0f;
  const float pcol = row[i] - clo;
  const float rv = fminf((lv - clo) / pcol, 1.0f - FLT_EPSILON);
  s = ((float)i + rv) / (float)W;
  t = ((float)j + ru) / (float)H;
  const float phi = (s - 0.5f) * (float)(2.0 * kPiD), lam = (0.5f - t) * (float)kPiD;
  const float cl = cosf(lam), sl = sinf(lam), cp = cosf(phi), sp = sinf(phi);
  d = mapping == ENV_LATLONG_Z_UP ? v3(cl * cp, cl * sp, sl) : v3(-(cl * sp), sl, cl * cp);
  const float sin_t = env_sin_pi_t(t);
  pdf = p_env * (((prow * pcol) * (float)(W * H)) / ((float)(2.0 * kPiD * kPiD) * sin_t));
  const bool ok = sin_t > 0.0f && pdf > 0.0f && pdf <= FLT_MAX;
  if (!ok) pdf = 0.0f;
  return ok;
}

// ---- textured surface emission (phx_material.emission_uv_texture; the rule is stated in include/phx_xpu.h) -----------------------------------
// Both run only in a scene with DevTexScene::any_emit_tex, behind a wave-uniform branch on that word; `emit_tex` is DevTexScene::mat_emit_tex.
// At a hit: e * texel at the hit's own (s, t), for a material that names an image.
__device__ __forceinline__ v3 hit_emission(const DevTexture* textures, const float4* texels, const uint32_t* emit_tex, uint32_t mat, const v3& e, const float2& st) {
  const uint32_t k = emit_tex[mat];
  if (!k) return e;
  const v3 c = tex_lookup(textures, texels, k - 1u, st.x, st.y);
  return v3(e.x * c.x, e.y * c.y, e.z * c.z);
}
// At a light sample (bu, bv) of triangle_t::sample on light triangle LT of light L: the UV of the sampled point itself, st = (bu * uv_a +
// bv * uv_b) + (1 - bu - bv) * uv_c with the weights P is built with -- NOT the reference's rotated reading of (bu, bv) as Moeller-Trumbore
// barycentrics (DESIGN: light_st_rotated) -- and e * texel there.  LT.prim is a pool element in such a scene (launch_remap_flat_light_tris).
// A light without an image: its constant e, st = (0, 0).  Used by k_shade_g<.., TEX> and by phx_dev_light_emission.
__device__ __forceinline__ v3 light_emission(const float2* elem_uv, const DevTexture* textures, const float4* texels, const uint32_t* emit_tex, const DevLight& L,
                                             const DevLightTri& LT, float bu, float bv, float2& st) {
  const v3 e(L.ex, L.ey, L.ez);
  st = make_float2(0.0f, 0.0f);
  const uint32_t k = emit_tex[L.material];
  if (!k) return e;
  const CornerUVs C = request_corner_uvs(elem_uv, LT.prim);
  const float w = 1 - bu - bv;
  st = make_float2((bu * C.a.x + bv * C.b.x) + w * C.c.x, (bu * C.a.y + bv * C.b.y) + w * C.c.y);
  const v3 c = tex_lookup(textures, texels, k - 1u, st.x, st.y);
  return v3(e.x * c.x, e.y * c.y, e.z * c.z);
}
// DevTexScene::mat_emit_tex through the scalar cache, read where it is used (inside the any_emit_tex branch) so that no register holds it elsewhere
__device__ __forceinline__ const uint32_t* emit_tex_table(const DevScene& sc) {
  return ((const __attribute__((address_space(4))) DevTexScene*)sc.tex)->mat_emit_tex;
}

// ---- host helpers of the launches -------------------------------------------------------------------
static inline uint32_t blocks_for(uint32_t n) { return (n + PHX_BLOCK - 1) / PHX_BLOCK; }
// A run-time flag becomes a template argument in ONE place: f is called with std::true_type or std::false_type.
template <typename F> static auto with_flag(bool v, F&& f) { if (v) return f(std::true_type{}); else return f(std::false_type{}); }

}  // namespace phx
