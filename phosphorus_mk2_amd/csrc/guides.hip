// guides.hip — the first-hit guide film (phx_guides in phx_xpu.h states the rule operation by operation).
// No counterpart in the reference.  A pass of its own: no frame launches this kernel, and it launches none of the frame's.
//
//   k_guides<LENS, TEXTURED>  one thread owns one film pixel and loops over its G samples: camera_ray (shade_common.h) rebuilds the ray of
//                             (seed, pixel, sample), traverse8 (bvh8.h) finds the hit k_trace_rays finds, lobe_weight_of (bsdf.h) resolves the
//                             material's lobes there as phx_dev_lobe_weights does, and the sums stay in registers.  No per-path buffers, no atomics,
//                             no workgroup waits on another.
//
// A wave owns an 8 x 8 block of pixels, so its 64 rays at sample s are neighbours on the film and walk the same nodes.  The per-lane traversal
// stack is dynamic LDS sized by the tree's depth, as in k_trace_rays.  A pixel past the film's edge returns before it forms an address.
#include "shade_common.h"

namespace phx {

namespace {
// k_trace_rays' stack: entry k of a lane at base[k * PHX_BLOCK], conflict-free 8-byte accesses
struct GuideStack {
  uint2* base; int sp;
  __device__ __forceinline__ void push(uint32_t b, uint32_t h) { base[sp * PHX_BLOCK] = make_uint2(b, h); ++sp; }
  __device__ __forceinline__ void pop(uint32_t& b, uint32_t& h) { --sp; const uint2 e = base[sp * PHX_BLOCK]; b = e.x; h = e.y; }
  __device__ __forceinline__ bool empty() const { return sp == 0; }
};
enum { GUIDE_TILE = 8, GUIDE_WAVES = PHX_BLOCK / 64 };
}  // namespace

template <bool LENS, bool TEXTURED>
__global__ void __launch_bounds__(PHX_BLOCK) k_guides(DevScene sc, PassBuffers pb, float* __restrict__ film) {
  extern __shared__ uint2 guide_stack[];
  const uint32_t tiles_x = (sc.width + GUIDE_TILE - 1u) / GUIDE_TILE, tiles_y = (sc.height + GUIDE_TILE - 1u) / GUIDE_TILE;
  const uint32_t tile = blockIdx.x * GUIDE_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (tile >= tiles_x * tiles_y) return;
  const uint32_t tile_y = tile / tiles_x, tile_x = tile - tile_y * tiles_x;
  const uint32_t x = tile_x * GUIDE_TILE + (lane & 7u), y = tile_y * GUIDE_TILE + (lane >> 3);
  if (x >= sc.width || y >= sc.height) return;
  const uint32_t pix = y * sc.width + x, G = pb.num_samples;

  v3 albedo_sum(0.0f), x_sum(0.0f);
  float t_sum = 0.0f; uint32_t hits = 0u;
  for (uint32_t s = 0; s < G; ++s) {
    v3 o, d;
    camera_ray<LENS>(sc, pb, pix * G + s, 0u, o, d);
    GuideStack stack{guide_stack + threadIdx.x, 0};
    Hit h;
    traverse8<false>(sc.pool, sc.grid, o, d, FLT_MAX, h, stack);
    v3 albedo(1.0f);  // a miss, an emitter
    if (h.tri != 0xffffffffu) {
      const float4 S = sc.elem_shade[h.tri];  // (geometric normal, material | smooth << 31)
      const uint32_t pm = f2u(S.w), mat = pm & 0x7fffffffu;
      const DevMaterial& m = sc.materials[mat];
      if (!m.is_emitter) {
        const VertexNormals VN = request_vertex_normals(sc, h.tri);
        const v3 n = shading_normal(VN, (pm >> 31) != 0, v3(S.x, S.y, S.z), h.u, h.v);
        const v3 wo = -d;  // hits.wi
        TexHit th{};
        if constexpr (TEXTURED) {
          const DevTexScene& tx = *sc.tex;
          const float2 st = hit_st(request_corner_uvs(tx.elem_uv, h.tri), h.u, h.v);
          th = TexHit{tx.textures, tx.texels, tx.lobe_tex + 8 * (size_t)mat, st.x, st.y};
        }
        albedo = v3(0.0f);
        for (uint32_t k = 0; k < 8u; ++k) {
          v3 lw(0.0f);
          if (k < m.num_lobes && lobe_weight_of<true, TEXTURED, TEXTURED>(m, k, m.lobes[k], n, wo, lw, th)) albedo = albedo + lw;
        }
      }
      const v3 X = o + d * h.t;
      x_sum = x_sum + X; t_sum = t_sum + h.t; ++hits;
    }
    albedo_sum = albedo_sum + albedo;
  }
  const float inv_g = 1.0f / (float)G, fh = (float)hits;
  float* px = film + (size_t)pix * 8u;
  px[0] = albedo_sum.x * inv_g; px[1] = albedo_sum.y * inv_g; px[2] = albedo_sum.z * inv_g;
  px[3] = fh * inv_g;
  px[4] = hits ? x_sum.x / fh : 0.0f; px[5] = hits ? x_sum.y / fh : 0.0f; px[6] = hits ? x_sum.z / fh : 0.0f;
  px[7] = hits ? t_sum / fh : 0.0f;
}

uint32_t guides_kernels(const void** out) {
  out[0] = reinterpret_cast<const void*>(&k_guides<false, false>); out[1] = reinterpret_cast<const void*>(&k_guides<false, true>);
  out[2] = reinterpret_cast<const void*>(&k_guides<true, false>); out[3] = reinterpret_cast<const void*>(&k_guides<true, true>);
  return 4u;
}

void launch_guides(hipStream_t stream, const DevScene& sc, const PassBuffers& pb, float* film) {
  const uint32_t tiles = ((sc.width + GUIDE_TILE - 1u) / GUIDE_TILE) * ((sc.height + GUIDE_TILE - 1u) / GUIDE_TILE);
  const dim3 g((tiles + GUIDE_WAVES - 1u) / GUIDE_WAVES), b(PHX_BLOCK);
  const size_t lds = (size_t)std::max(2u, std::min(sc.stack_levels, (uint32_t)PHX_MAX_BVH_DEPTH)) * PHX_BLOCK * sizeof(uint2);  // launch_trace_rays' sizing
  with_flag(sc.aperture_radius != 0.0f, [&](auto LENS) {
    with_flag((sc.any_tex & SC_TEX_LOBES) != 0u, [&](auto TEXTURED) {
      hipLaunchKernelGGL((k_guides<decltype(LENS)::value, decltype(TEXTURED)::value>), g, b, lds, stream, sc, pb, film);
    });
  });
}

}  // namespace phx
