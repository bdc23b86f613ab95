// shade_lambert.hip — the shade kernel of the Lambert-only scenes and its launch (see kernels.h for the HBM layout and the map of
// kernels to files).  One path per lane, 64-lane wavefronts.
//
//   k_shade     deferred_shading_kernel_t (reference src/kernels/cpu/deferred_shading_kernel.hpp:20-72) + light_sampler_t
//               (spt.hpp:95-149) + integrator_t (spt.hpp:161-328) fused; survivors and shadow rays are appended to their
//               queues with __ballot/__popcll compaction (one global atomic per 1024-thread workgroup)
#include "shade_common.h"
#include "shade_launch.h"

namespace phx {

// Stream compaction: append-slot allocation for the threads of a workgroup that `want` one.
// __ballot/__popcll give the rank inside the wave, the waves' counts are summed through LDS, and ONE
// global atomic per workgroup reserves the slots (a returning atomic on one address sustains only
// ~90 ops/us chip-wide — per-wave atomics made k_shade atomic-bound).  All threads of the block must call.
#ifndef PHX_SHADE_BLOCK_D
#define PHX_SHADE_BLOCK_D 1024  /* Lambert-only k_shade: threads per workgroup.  The kernel is bound by the atomics on the two queue counters (one per
                                    workgroup and queue): 256 threads 28.3 ms, 512 16.0 ms, 1024 11.3 ms per frame (profiles/README.md) */
#endif
// Both queues of a workgroup are appended in ONE round: the wave counts of the two predicates go to LDS, the first lanes of
// waves 0 and 1 each prefix one of them and issue its atomic — the two round trips to the counters overlap instead of following
// each other (two barriers and one atomic latency per workgroup instead of four and two).
template <int SHADE_BLOCK>
__device__ __forceinline__ void block_append2(bool want_a, uint32_t* counter_a, bool want_b, uint32_t* counter_b, uint32_t* lds /* [2 * (waves + 1)] */,
                                              uint32_t& at_a, uint32_t& at_b) {
  static_assert(SHADE_BLOCK >= 128 && SHADE_BLOCK % 64 == 0, "block_append2: wave 0 sums queue A, wave 1 queue B");
  const uint32_t lane = __lane_id(), wave = threadIdx.x >> 6, nwaves = SHADE_BLOCK >> 6;
  const unsigned long long mask_a = __ballot(want_a), mask_b = __ballot(want_b);
  uint32_t* cnt_a = lds; uint32_t* cnt_b = lds + nwaves + 1;
  if (lane == 0) { cnt_a[wave] = (uint32_t)__popcll(mask_a); cnt_b[wave] = (uint32_t)__popcll(mask_b); }
  __syncthreads();
  if (lane == 0 && wave < 2) {
    uint32_t* cnt = wave == 0 ? cnt_a : cnt_b;
    uint32_t total = 0;
#pragma nounroll
    for (uint32_t w = 0; w < nwaves; ++w) { const uint32_t c = cnt[w]; cnt[w] = total; total += c; }
    cnt[nwaves] = total ? atomicAdd(wave == 0 ? counter_a : counter_b, total) : 0u;
  }
  __syncthreads();
  const unsigned long long below = (1ull << lane) - 1ull;
  at_a = cnt_a[nwaves] + cnt_a[wave] + (uint32_t)__popcll(mask_a & below);
  at_b = cnt_b[nwaves] + cnt_b[wave] + (uint32_t)__popcll(mask_b & below);
}

// The Lambert-only scenes (the soups, the Cornell box): shade + NEE + integrate of one path per thread in one go; HBM-stream bound.
// Scenes with other closures go through k_shade_g below.
template <int MATS /* 1 Lambert lobes only; 2 at most one Lambert lobe per material (DevScene::diffuse_only) */,
          bool FIRST /* queue q = the camera rays of this pass: nothing to read but the hit */, bool LENS = false /* FIRST: thin-lens camera */>
__global__ void __launch_bounds__(PHX_SHADE_BLOCK_D) __attribute__((amdgpu_waves_per_eu(4, 8))) k_shade(DevScene sc, PassBuffers pb, int q, int sq, uint32_t sample0) {
  static_assert(MATS == 1 || MATS == 2, "general closures: k_shade_g");
  constexpr bool DIFFUSE_ONLY = true;
  constexpr int MAXL = MATS == 2 ? 1 : 8;
  constexpr int PHX_SHADE_BLOCK = PHX_SHADE_BLOCK_D;
  __shared__ uint32_t lds_cnt[2 * ((PHX_SHADE_BLOCK >> 6) + 1)];
  // a k_trace wave that hit its watchdog left rays untraced: their hit records are whatever the buffer held (an earlier step's, an earlier
  // scene's) — the frame is reported as failed anyway (device.cpp), so nothing is shaded, nothing appended, and the queues of the following
  // steps are empty
  if (pb.stats->watchdog | pb.stats->ring_watchdog) return;
  const uint32_t count = pb.counters[q * CNT_STRIDE];
  const uint32_t i = blockIdx.x * PHX_SHADE_BLOCK + threadIdx.x;
  if (i == 0) zero_cursors(pb.counters);  // the next k_trace pulls its chunks from here
  // One block per workgroup, grid sized for the queue's capacity.  (A fixed grid walking the queue in a loop — what k_shade_g does —
  // costs this kernel its occupancy: whatever is loop-invariant gets hoisted and held in registers, 51-61 VGPRs become 73-82, and
  // 1024-thread workgroups need <= 64 to run two per CU.)
  if (blockIdx.x * PHX_SHADE_BLOCK >= count) return;
  const bool live = i < count;
  bool alive = false, want_shadow = false, masked = false;
  uint32_t path = 0, next_specular = 0;
  v3 nxt_o, nxt_d, sh_o, sh_d, contrib, nxt_beta;
  uint32_t nxt_depth = 0, key = 0;
  float sh_t = 0.0f;
  if (live) {
    float4 a, b, bd;
    const uint2 h = pb.hit_tt[i];  // (t, pool index): 8 bytes; the barycentrics are a stream of their own, read for smooth faces only (below)
    if (FIRST) {
      v3 co, cd;
      camera_ray<LENS>(sc, pb, i, sample0, co, cd);
      a = make_float4(co.x, co.y, co.z, u2f(i)); b = make_float4(cd.x, cd.y, cd.z, FLT_MAX);
      bd = make_float4(1.0f, 1.0f, 1.0f, u2f(0u));  // state_t::reset: beta = 1, depth = 0
    } else {
      a = pb.ro[q][i]; b = pb.rd[q][i]; bd = pb.qs[q][i];
    }
    const uint32_t pbits = f2u(a.w);
    path = pbits & 0x7fffffffu;
    const bool specular = (pbits >> 31) != 0;
    v3 beta(bd.x, bd.y, bd.z);
    // radiance is only read-modified-written when this step adds something: out += beta * e with e == 0 and a
    // finite beta leaves `out` unchanged bit for bit (out is never -0), so the 32 B of traffic are skipped
    v3 add_e(0.0f); bool add_rad = false;
    const bool beta_finite = isfinite(bd.x) && isfinite(bd.y) && isfinite(bd.z);
    uint32_t depth = f2u(bd.w);
    // the path's RNG key: computed once, by the first shade of the pass, then carried in the ray record's fourth word (a closest-hit ray's
    // tmax is always FLT_MAX) — a dependent gather (pixel table), an integer division and four hash rounds less per later step
    if (FIRST) {
      const uint32_t pix = path / pb.num_samples, s = path - pix * pb.num_samples;
      const uint32_t xy = pb.pix_xy[pix];
      key = path_key(pb.seed, (xy >> 16) * sc.width + (xy & 0xffffu), sample0 + s);
    } else {
      key = f2u(b.w);
    }
    const uint32_t tri = h.y;
    const v3 o(a.x, a.y, a.z), d(b.x, b.y, b.z);
    if (tri != 0xffffffffu) {
      const float4 S = sc.elem_shade[tri];  // (geometric normal, material | smooth << 31): 16 bytes of the hit triangle instead of its 64-byte record
      const uint32_t pm = f2u(S.w);
      const v3 p = o + d * u2f(h.x);       // hits.p = p + wi*d
      const v3 wo = -d;                    // hits.wi = -wi
      v3 n(S.x, S.y, S.z);
      if ((pm >> 31) != 0) {  // a smooth face: the scene has one, so the trace kernels wrote pb.hit_uv (scene_commit.cpp: the scene's hit_uv flag)
        const float2 uv = pb.hit_uv[i];
        n = shading_normal(sc, tri, true, v3(0.0f), v3(0.0f), uv.x, uv.y);
      }
      // material_t::evaluate (material.cpp:419-458): the closure list at this hit.  A constant recipe is read from the table; a
      // material with a hit-dependent weight (glass: Fresnel-driven mix) gets its weights resolved for (n, hits.wi) first.
      const DevMaterial* mp = &sc.materials[pm & 0x7fffffffu];
      DevMaterial mh;
      if (MATS == 2) {  // the whole material in two 16-byte loads; only the fields named here are ever read (bsdf_f / bsdf_sample <true, 1>)
        const DevMatLite ml = sc.mat_lite[pm & 0x7fffffffu];
        mh.num_lobes = ml.lobes_flags & 0xffu; mh.lobes[0].flags = ml.lobes_flags >> 8; mh.lobes[0].type = L_DIFFUSE;
        mh.lobes[0].wx = ml.wx; mh.lobes[0].wy = ml.wy; mh.lobes[0].wz = ml.wz;
        mh.ex = ml.ex; mh.ey = ml.ey; mh.ez = ml.ez; mh.sheen_L5 = 0.0f;
        mp = &mh;
      }
      const DevMaterial& m = *mp;
      if (pb.pn && (FIRST || depth == 0)) pb.pn[path] = make_float4(n.x, n.y, n.z, 1.0f);
      const v3 e(m.ex, m.ey, m.ez);
      if (depth == 0 || specular) { add_e = e; add_rad = true; }  // spt.hpp:177-179
      // ---- next-event estimation: sampler_t::fresh_light_samples + light_sampler_t (sampling.cpp:160-179, spt.hpp:95-149)
      {
        const uint32_t b0 = depth * DIMS_PER_STEP;
        const float pick = draw_f32(key, b0 + DIM_LIGHT_PICK), lu = draw_f32(key, b0 + DIM_LIGHT_U), lv = draw_f32(key, b0 + DIM_LIGHT_V);
        const float nlf = (float)sc.num_lights;
        uint32_t l = (uint32_t)floorf(pick * nlf);
        if (l > sc.num_lights - 1) l = sc.num_lights - 1;
        const DevLight L = sc.lights[l];
        const float numf = (float)L.num_tris;
        uint32_t ti = (uint32_t)floorf(lu * numf);  // uniform by index (light.cpp:55), pdf = 1/area
        if (ti > L.num_tris - 1) ti = L.num_tris - 1;
        const float remapped = fminf(lu * numf - (float)ti, 1.0f - FLT_EPSILON);
        const DevLightTri LT = sc.light_tris[L.first_tri + ti];
        const float x = sqrtf(remapped);
        const float bu = 1 - x, bv = lv * x;     // triangle_t::sample, mesh.cpp:318-324
        const v3 la(LT.ax, LT.ay, LT.az), lb(LT.bx, LT.by, LT.bz), lc(LT.cx, LT.cy, LT.cz);
        const v3 P = bu * la + bv * lb + (1 - bu - bv) * lc;
        const float lpdf = L.lpdf;  // (1.0f / L.area) / nlf, evaluated at preprocess
        sh_o = v3(p.x + n.x * 0.0001f, p.y + n.y * 0.0001f, p.z + n.z * 0.0001f);
        v3 wl = P - sh_o;
        const float l2 = sdot(wl, wl);
        const float dist = sqrtf(l2) - 0.0001f;
        const float oolen = 1.0f / sqrtf(l2);
        wl = v3(wl.x * oolen, wl.y * oolen, wl.z * oolen);
        if (sdot(n, wl) >= 0.0f) {
          // li(), spt.hpp:212-255 — evaluated before the occlusion test; added by k_trace_shadow if unoccluded
          const v3 f = bsdf_f<DIFFUSE_ONLY, MAXL>(m, n, wl, wo);
          // the light's normal at the sampled point (mesh_t::shading_parameters on the light triangle) and its emission
          const v3 ln = LT.smooth ? shading_normal(sc, LT.prim, true, lb - la, lc - la, bu, bv) : v3(LT.nx, LT.ny, LT.nz);
          const v3 le(L.ex, L.ey, L.ez);
          const float pdf = lpdf * dist * dist / fabsf(dot(ln, -wl));
          const v3 li = ((le * 4.0f) * f) * (1.0f / pdf);
          contrib = beta * li;
          sh_d = wl; sh_t = dist;
          want_shadow = true;
        } else {
          masked = true;
        }
      }
      // ---- integrate: ++depth, russian roulette, bsdf sampling (spt.hpp:188-190, 257-328)
      depth += 1;
      float wgt = 1.0f;
      alive = depth < sc.max_depth;
      if (alive && depth >= 3) {
        const float qq = fmaxf(0.05f, 1.0f - luminance(beta));
        const float xi = draw_f32(key, (depth - 1u) * DIMS_PER_STEP + DIM_RR);
        alive = xi >= qq;
        if (alive) wgt = (1.0f / (1.0f - qq));
      }
      beta = beta * wgt;
      if (alive) {
        const uint32_t b1 = (depth - 1u) * DIMS_PER_STEP;
        v3 sampled; float pdf; uint32_t fl;
        const v3 f = bsdf_sample<DIFFUSE_ONLY, MAXL>(m, n, draw_f32(key, b1 + DIM_BSDF_U), draw_f32(key, b1 + DIM_BSDF_V), wo, sampled, pdf, fl);
        if ((f.x == 0.0f && f.y == 0.0f && f.z == 0.0f) || pdf == 0.0f) {
          alive = false;
        } else {
          const float weight = dot(n, sampled);
          beta = beta * (f * (fabsf(weight) / pdf));
          const float off = (weight < 0.0f) ? -0.0001f : 0.0001f;
          nxt_o = p + n * off;
          nxt_d = sampled;
          next_specular = (fl & B_SPECULAR) ? 1u : 0u;
        }
      }
    } else {
      // miss: environment lighting (deferred_shading_kernel.hpp:65-70, spt.hpp:199-202)
      v3 e(0.0f);
      if (sc.env_material >= 0) { const DevMaterial& m = sc.materials[sc.env_material]; e = v3(m.ex, m.ey, m.ez); }
      add_e = e; add_rad = true;
      if (FIRST && pb.pn) pb.pn[path] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      masked = true;  // a miss still occupies a (MASKED|SHADOW) slot in the reference's shadow stream (spt.hpp:138-141)
    }
    nxt_beta = beta; nxt_depth = depth;  // only the next k_shade of a surviving path reads them: they leave with the ray below
    if (FIRST) {  // r = 0 + beta * e: every path's radiance is written here, nothing is read
      const v3 rad = v3(0.0f) + v3(bd.x, bd.y, bd.z) * add_e;
      pb.pr[path] = make_float4(rad.x, rad.y, rad.z, 0.0f);
    } else if (add_rad && !(beta_finite && add_e.x == 0.0f && add_e.y == 0.0f && add_e.z == 0.0f)) {
      const float4 rr = pb.pr[path];
      const v3 rad = v3(rr.x, rr.y, rr.z) + v3(bd.x, bd.y, bd.z) * add_e;  // beta as it was when the ray arrived
      pb.pr[path] = make_float4(rad.x, rad.y, rad.z, 0.0f);
    }
  }
  // ---- stream compaction: survivors -> next ray queue, unmasked NEE rays -> shadow queue
  uint32_t no, ns;
  // (the rays leave in thread order.  Sorting the workgroup's survivors by direction octant and / or the Morton cell of their origin
  // before the append — 64 or 512 bins through LDS — bought k_trace 0.5 ms of 60 and cost this kernel 0.8-1.8 ms of 10 on every
  // workload, config 4 included: profiles/r03_g_bin_octant_ab.log, r03_i_bin_morton_ab.log; removed after commit "Ray-coherence experiments")
  block_append2<PHX_SHADE_BLOCK>(alive, &pb.counters[(q ^ 1) * CNT_STRIDE], want_shadow, &pb.counters[CNT_SHADOW + sq * CNT_STRIDE], lds_cnt, no, ns);
  if (alive) {
    pb.ro[q ^ 1][no] = make_float4(nxt_o.x, nxt_o.y, nxt_o.z, u2f(path | (next_specular << 31)));
    pb.rd[q ^ 1][no] = make_float4(nxt_d.x, nxt_d.y, nxt_d.z, u2f(key));  // (d, the path's RNG key)
    pb.qs[q ^ 1][no] = make_float4(nxt_beta.x, nxt_beta.y, nxt_beta.z, u2f(nxt_depth));  // the path's state travels with its ray
  }
  if (want_shadow) {
    pb.so[ns] = make_float4(sh_o.x, sh_o.y, sh_o.z, u2f(path));
    pb.sd[ns] = make_float4(sh_d.x, sh_d.y, sh_d.z, sh_t);
    pb.sc[ns] = make_float4(contrib.x, contrib.y, contrib.z, 0.0f);
  }
  (void)masked;  // rays_masked = rays_closest - rays_shadow: every shaded slot yields a shadow ray or a masked slot
}

template <int MATS, bool FIRST, bool LENS>
static uint64_t shade_d(dim3 g, dim3 b, hipStream_t stream, const DevScene& sc, const PassBuffers& pb, int q, int sq, uint32_t sample0) {
  constexpr uint32_t bit = (MATS == 2 ? PHX_SHADE_FAMILY_LAMBERT1 : PHX_SHADE_FAMILY_LAMBERT) * PHX_SHADE_PASSES + shade_pass<FIRST, LENS>();
  static_assert(bit < PHX_SHADE_KERNELS, "phx_stats::shade_kernels: a kernel without a bit");
  hipLaunchKernelGGL((k_shade<MATS, FIRST, LENS>), g, b, 0, stream, sc, pb, q, sq, sample0);
  return 1ull << bit;
}
// launch_shade's branch for a sc.diffuse_only scene (shade_general.hip; declared in shade_launch.h)
uint64_t launch_shade_lambert(hipStream_t stream, const DevScene& sc, const PassBuffers& pb, int q, int sq, uint32_t capacity, uint32_t sample0, int camera_rays, bool lens) {
  const dim3 g((capacity + PHX_SHADE_BLOCK_D - 1) / PHX_SHADE_BLOCK_D), b(PHX_SHADE_BLOCK_D);
  return with_flag(sc.diffuse_only == 2, [&](auto ONE_LOBE) {
    return with_pass(camera_rays != 0, lens, [&](auto FIRST, auto LENS) { return shade_d<decltype(ONE_LOBE)::value ? 2 : 1, decltype(FIRST)::value, decltype(LENS)::value>(g, b, stream, sc, pb, q, sq, sample0); });
  });
}

}  // namespace phx
