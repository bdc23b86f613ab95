// kernels.h — device-side data layout of the wavefront path tracer and the launch entry points
// implemented by the kernel families below.  One "pass" carries P pixels x S samples = npaths paths through
// generate -> [trace closest -> shade/NEE/integrate -> trace shadow] x depth -> film.
//
// One translation unit per kernel family (the head of each file maps its kernels to the reference's sources):
//   trace.hip          k_trace, k_trace_primary, k_trace_rays; trace_plan, init_kernels_on_current_device, launch_trace*
//   shade_lambert.hip  k_shade<MATS, FIRST, LENS> (Lambert-only scenes), block_append2
//   shade_general.hip  k_shade_g and its append ring; launch_shade (which reaches k_shade through shade_launch.h)
//   film_hooks.hip     k_begin_pass, k_film, k_film_moments, k_scatter_film; k_adaptive_* (the selection of adaptive sampling); the hook kernels of the parity tests (phx_dev_*); the preprocess kernels
//   denoise.hip        k_denoise_pack, k_denoise_iteration, k_denoise_unpack: the film denoiser, a post-process no frame launches
//   guides.hip         k_guides: the first-hit guide film (albedo, coverage, position, distance), a pass of its own no frame launches
//   accumulate.hip     k_accumulate: pools a finished film into an accumulator film and counts its summary, a pass of its own no frame launches
//   tile_map.hip       k_tile_map: an accumulator film's convergence, one record per tile of a grid, and its summary, a pass of its own no frame launches
//   reproject.hip      k_reproject: carries an accumulator film from one camera to another by the guide films' first hits, a pass of its own no frame launches
//   outlier_clamp.hip  k_outlier_clamp: clamps a film's pixels to bounds taken from a reference film's neighbourhoods (despeckle, history clamp), a pass of its own no frame launches
//   display.hip        k_display_histogram, k_display_exposure, k_display_encode: a film's radiance to an RGBA8 sRGB image, a pass of its own no frame launches
//   film_pass.h        what the film passes with a summary share: the counter path (wave_count, wave_sum, store_wave_counts, add_workgroup_counts), accumulator_pixel_valid
//   shade_common.h     the device functions two or more of them share: camera_ray, shading_normal, light_pick, env_sample, light_emission, ...
// A family's code can change another's only through a shared header.
//
// HBM layout (records of 16 B, so that a wave reads/writes 1 KiB per instruction, except the hit records, which are two streams of 8 B):
//   ray queue (x2, ping-pong)  ro[i] = (o.xyz, path | SPECULAR<<31)   rd[i] = (d.xyz, tmax)
//   hit records                hit_tt[i] = (t, triangle-record index)   always
//                              hit_uv[i] = (u, v)                       only when the committed scene reads barycentrics: a smooth face, a UV
//                                                                       consumer (TEX / MASK / emitter images) or a per-hit material
//   shadow queue               so[i] = (o.xyz, path)  sd[i] = (d.xyz, tmax)  sc[i] = (beta*Li rgb, 0)
//   path state (by path id)    pb[path] = (beta.rgb, depth)   pr[path] = (radiance.rgb, 0)
//   path id = sample_in_pass * P + pixel_in_batch  (neighbouring lanes = neighbouring pixels)
// These take the place of ray_t<1024> / interaction_t<1024> / active_t<1024> / spt::state_t<1024>
// (reference src/state.hpp:40-282, src/kernels/cpu/spt.hpp:23-64): the interaction record is never
// materialised — shade, NEE and integrate are one kernel.
#pragma once
#include "bsdf.h"
#include "bvh8.h"
#include "reproject_check.h"  // ReprojectCamera (host-only)

#include <hip/hip_runtime.h>

namespace phx {

// Light table (light_t::make_area, src/light.cpp:10-45).  What k_shade would otherwise fetch through three more dependent loads per
// shaded hit is resolved once at preprocess, with the same fp32 operations the kernel would use: the pick pdf (1/area)/nlights
// (spt.hpp:95-149; under PHX_LIGHT_SELECT_BY_POWER (1/area) * p_l, p_l the light's interval of the selection table), the light material's emission (material_t::evaluate's e) and, per triangle, the geometric normal of a flat face.
struct DevLight { uint32_t first_tri, num_tris; float area; uint32_t material; float lpdf, ex, ey, ez; };                 // 32 B
struct DevLightTri { float ax, ay, az, bx, by, bz, cx, cy, cz, nx, ny, nz; uint32_t prim, smooth, mesh_mat, face; };   // 64 B
// A material of a scene in which every material is at most ONE Lambert lobe (the soups, the Cornell box): 32 B instead of 544
struct DevMatLite { float wx, wy, wz; uint32_t lobes_flags /* num_lobes | flags << 8 */; float ex, ey, ez; uint32_t pad; };

// The image textures of a scene as k_shade_g<., ., ., TEX> reads them (one record in device memory, read through the scalar cache)
struct DevTexScene {
  const float2* elem_uv;          // 3 x (s, t) per POOL ELEMENT, indexed like `tris` (the triangle's corner UVs, mesh_t::shading_parameters)
  const DevTexture* textures;     // per texture: offset into `texels`, width, height, filter / wrap modes
  const float4* texels;           // every texture's texels, RGB + 0, row-major, one 16-byte load per texel
  const uint32_t* lobe_tex;       // 8 per material: texture + 1 of lobe k (DevMaterial::tex_lobes says which are textured)
  uint32_t env_tex;               // k_shade_g<.., ENV>: the environment's image (0-based index into `textures`)
  uint32_t env_mapping;           // and its lat-long mapping (ENV_LATLONG_*)
  // textured surface emission (phx_material.emission_uv_texture; bsdf.h: hit_emission, shade_common.h: light_emission)
  uint32_t any_emit_tex;          // some emitter's emission is multiplied by an image: the wave-uniform branch of the TEX kernels
  float env_p;                    // SC_LIGHTS_ENV: the environment's interval of the selection table, p_env (this word was padding)
  const uint32_t* mat_emit_tex;   // per material: its emission image + 1 (0 = none), indexed by the hit's material and by DevLight::material
  const float* env_cdf;           // SC_LIGHTS_ENV: the environment's direction tables, mcdf (H floats) then ccdf (H rows of W floats); nullptr otherwise
};
// DevScene::any_tex bits: which image lookups the shade kernels compile in
enum { SC_TEX_LOBES = 1u /* some lobe is textured or masked: TEX */, SC_TEX_ENV = 2u /* the environment has an image: ENV */,
       SC_TEX_MASK = 4u /* some lobe's mix factor is an image (PHX_FAC_TEX_*): MASK, always with SC_TEX_LOBES and any_per_hit */,
       SC_TEX_ANY = 7u,
       // not an image bit: PHX_LIGHTS_BY_AREA.  k_shade_g picks a light's triangle by the area CDF (light_pick); the scene then runs k_shade_g
       // (diffuse_only = 0) and `lights` has the CDF behind it
       SC_LIGHTS_BY_AREA = 8u,
       // PHX_LIGHT_SELECT_BY_POWER, always with SC_LIGHTS_BY_AREA: light_pick searches the selection table pcdf, which sits between the light
       // records and the area CDF: num_lights floats, padded to whole records of the light table
       SC_LIGHTS_BY_POWER = 16u,
       // PHX_LIGHT_INCLUDE_ENVIRONMENT, always with SC_LIGHTS_BY_POWER and SC_TEX_ENV: pcdf has num_lights + 1 entries, the last one the environment's,
       // and k_shade_g<.., ENV> samples the image by DevTexScene::env_cdf when the pick lands there (shade_common.h: env_sample)
       SC_LIGHTS_ENV = 32u };

struct DevScene {
  const uint32_t* pool;           // the BVH8 pool: 16 words per element, element 0 = root nodelet (bvh8.h)
  const TriRec* tris;             // the same pool seen as triangle records (hit records carry pool indices)
  SceneGrid grid;                 // grid of the nodelets' origins
  const DevTexScene* tex;         // image textures of the scene (device memory), or nullptr when no lobe is textured and the environment has no image
  const float4* elem_shade;       // per POOL ELEMENT (indexed like `tris`): what shading needs of a hit triangle in 16 bytes — its geometric normal
                                  // normalize((v1-v0) x (v2-v0)) (mesh.cpp:201-215, computed once at preprocess by the shade kernels' own expression) and
                                  // material | smooth << 31 — instead of the 64-byte triangle record (round 6)
  const float* elem_normals;      // 9 floats (n0,n1,n2) per POOL ELEMENT — indexed like `tris`, by the hit's pool index, so that the normals are requested
                                  // WITH the triangle record, not after it (round 6; entries of nodelets are never read) — or nullptr when no face is smooth
  const DevMaterial* materials;
  const DevMatLite* mat_lite;     // diffuse_only == 2: the same table, 32 B per material
  const DevLight* lights;         // num_lights records; under SC_LIGHTS_BY_AREA the area CDF follows them in the same allocation: one float per light
                                  // triangle, indexed like light_tris (light_cdf); under SC_LIGHTS_BY_POWER the selection table comes first (light_pcdf)
  const DevLightTri* light_tris;
  uint32_t num_lights;
  int32_t env_material;
  float cam_m[16];
  float zoom, stepx, stepy, ratio;
  uint32_t width, height;
  uint32_t max_depth;
  uint32_t stack_levels;          // BVH depth
  uint32_t num_elems;             // pool elements (stored breadth first: a prefix of the pool is the top of the tree)
  uint32_t num_cus;               // compute units of the device (persistent grid sizing)
  uint32_t diffuse_only;          // 1: every lobe of every material is Lambert (k_shade<1>); 2: and no material has more than one (k_shade<2>)
  uint32_t any_per_hit;           // some material's closure weights depend on the hit (glass): k_shade<0>; none: k_shade<3>
  uint2* stack_spill;             // k_trace<., SPILL>: stack entries below the levels kept in LDS, [level - lds_levels][thread of the grid]
  uint32_t spill_stride;          // threads of the largest k_trace grid (0 = every level is in LDS)
  float aperture_radius, focal_distance;  // camera_t (entities/camera.hpp:24-29): thin lens when aperture_radius != 0 (camera.hpp:140-147)
  uint32_t any_tex;               // SC_TEX_* bits: some lobe is textured (k_shade_g<., ., ., TEX>) / the environment has an image (k_shade_g<.., ENV>);
                                  // either one: k_shade_g shades every step and sc.tex is set.  (This word and `tex` take
                                  // the struct's tail padding and the slot of a pointer no kernel read: DevScene keeps its size and layout, so
                                  // the kernels that take it by value compile to the same code as before textures existed)
};
static_assert(sizeof(DevScene) == 240, "DevScene is every kernel's first argument: its size fixes the offsets of the ones behind it");

// counters (x CNT_STRIDE words): [0],[1] ray-queue lengths (ping-pong); [2],[3] shadow-queue lengths (by step parity); [4],[5] chunk cursors
// every counter on its own 128-byte line: the queue-length counters take one atomic per k_shade workgroup and one address (line)
// sustains ~90 atomics/us — two counters on one line halve what each gets
// [4 + p * CNT_SEGS + s]: the range cursor of queue p (0 shadow, 1 closest) for SEGMENT s of the queue — the queue is cut in CNT_SEGS equal
// parts, one per XCD (workgroup ids go round the XCDs: id & 7), so that an XCD's L2 serves one part of the image
enum { CNT_STRIDE = 32, CNT_SHADOW = 2 * CNT_STRIDE, CNT_CURSOR = 4 * CNT_STRIDE, CNT_SEGS = 8, CNT_WORDS = (4 + 2 * CNT_SEGS) * CNT_STRIDE };
struct DevStats {
  unsigned long long rays_closest, rays_shadow, rays_masked, camera_samples;
  // instrumented build only (-DPHX_COUNT=1, `make variant NAME=count`): traversal work, [0] closest-hit rays, [1] shadow rays
  unsigned long long node_visits_lds[2], node_visits_mem[2], tri_tests[2];
  // wave-level: loop iterations, executions of the node block / the triangle block (a block runs when ANY lane needs it)
  unsigned long long wave_iters, node_block_execs, tri_block_execs, refills;
  unsigned long long idle_lane_iters, tri_pending_lane_iters;
  // k_trace_primary (instrumented build): packets walked, packets that fell back to the per-lane walk, node tests and triangle tests
  // per PACKET (one test serves the 64 rays), and lanes whose ray was improved by a triangle test (of 64 per test)
  unsigned long long primary_packets, primary_fallbacks, primary_node_tests, primary_tri_tests, primary_tri_lanes_hit;
  unsigned long long watchdog;         // k_trace waves that gave up after PHX_TRACE_WATCHDOG iterations: 0, or the frame is reported as failed
  unsigned long long stack_pushes[8];  // instrumented: pushes onto the per-lane group stack by the depth they land at (7 = 7 and deeper)
  // instrumented: pending (ray, triangle) pairs of the wave at its triangle-block executions — their sum, and executions by the number of
  // pairs: <= 8, <= 16, <= 24, <= 32, <= 48, <= 64, <= 96, more
  unsigned long long tri_pairs_pending, tri_pairs_hist[8];
  unsigned long long ring_watchdog;    // k_shade_g waves whose wait on the append ring timed out (PHX_RING_SPINS): 0, or the frame is reported as failed
};

struct PassBuffers {
  float4* ro[2]; float4* rd[2];
  uint2* hit_tt;              // (t as bits, pool index of the hit triangle | 0xffffffff = miss): written by every closest-hit trace, read by every shade
  float2* hit_uv;             // the hit's barycentrics, or nullptr: the trace kernels are instantiated without them (UV = false) and no shade kernel asks
  float4* so; float4* sd; float4* sc;
  float4* qs[2];              // path state (beta, depth) of the queue entry: it travels WITH the ray (round 6; before: an array by path id, a dependent gather)
  float4* pr;
  float4* pn;                 // primary normal + hit flag per path (only when the normals channel is on)
  uint32_t* counters;         // CNT_WORDS
  DevStats* stats;
  const uint32_t* pix_xy;     // per pixel of the batch: x | y << 16 (film coordinates)
  const float2* jitter;       // per spp index: film jitter shared by all pixels (src/sampling.cpp:98-112)
  float* acc;                 // batch render buffer: tile after tile, interleaved xstride floats per pixel
  uint32_t num_pixels;        // P
  uint32_t num_samples;       // samples of this pass; path id = pixel_in_batch * num_samples + sample_in_pass
  uint32_t xstride;           // floats per pixel (frame_plan.h: FilmLayout, which states the pixel's layout once)
  uint32_t normals_offset;    // offset of channel "normals" inside a pixel, 0 = off
  uint64_t seed;
  uint32_t* qlen_out;         // k_trace: host-visible word that receives the length of the ray queue it traces (frame_driver.cpp: enqueue_batch reads it with device_word and sizes the next shade grids by it), or nullptr
};

// shape of a k_trace launch on a scene (reported through phx_stats so that tests can assert which plan a tree ran with)
struct TracePlan { uint32_t block, ntop, levels, lds_bytes, wg_per_cu, lds_levels, spill_threads, packed /* 5-byte stack entries in LDS */; };
TracePlan trace_plan(const DevScene& sc);
// per device, once: lets the traversal kernels use the CU's full 160 KB of LDS as dynamic shared memory
hipError_t init_kernels_on_current_device();

bool launch_counts_traversal_work();  // true in the instrumented build (PHX_COUNT)

// launches (all asynchronous on `stream`)
// start of a pass: queue 0 stands for the num_pixels x num_samples camera rays, which are rebuilt on the fly (camera_ray)
void launch_begin_pass(hipStream_t stream, const PassBuffers& pb, uint32_t num_samples);
// one persistent launch: closest-hit rays of queue q (do_closest) + any-hit rays of shadow queue sq (do_shadow)
void launch_trace(hipStream_t stream, const DevScene& sc, const PassBuffers& pb, int q, int sq, int do_closest, int do_shadow, uint32_t capacity);
// step 0 of a pass: the npaths camera rays (never stored: rebuilt from the pixel and jitter tables), walked as packets by k_trace_primary;
// writes the hit records of queue q and does k_trace's start-of-step bookkeeping
void launch_trace_primary(hipStream_t stream, const DevScene& sc, const PassBuffers& pb, uint32_t npaths, uint32_t sample0, int q, int sq);
// shades queue q, appends survivors to queue q^1 and NEE rays to shadow queue sq
// -> the launched kernel's bit of phx_stats::shade_kernels
uint64_t launch_shade(hipStream_t stream, const DevScene& sc, const PassBuffers& pb, int q, int sq, uint32_t capacity, uint32_t sample0, int camera_rays);
void launch_film(hipStream_t stream, const PassBuffers& pb, uint32_t num_samples, float inv_spp_pps);
// launch_film for a frame with phx_frame.moments_channel: the same film add, and the channel m2 (3 floats at m2_offset of a pixel) by the rule of
// phx_xpu.h; samples_done = the samples of every pixel that earlier passes of the batch have added.  They are arguments of this launch and not
// fields of PassBuffers, which every kernel takes by value: a new field would move the kernel-argument offsets of all of them
void launch_film_moments(hipStream_t stream, const PassBuffers& pb, uint32_t num_samples, float inv_spp_pps, uint32_t samples_done, uint32_t m2_offset);
// preprocess: vertex normals from scene_t::triangles() order to pool-element order (elem_of_prim: the builders' map), and the smooth light
// triangles' `prim` from primitive to pool element (they look their normals up in the same table)
void launch_build_shade_recs(hipStream_t stream, const TriRec* tris, const uint32_t* elem_of_prim, float4* elem_shade, uint32_t num_prims);
void launch_permute_normals(hipStream_t stream, const float* prim_normals, const uint32_t* elem_of_prim, float* elem_normals, uint32_t num_prims);
void launch_permute_uvs(hipStream_t stream, const float2* prim_uv, const uint32_t* elem_of_prim, float2* elem_uv, uint32_t num_prims);
void launch_remap_light_tris(hipStream_t stream, DevLightTri* light_tris, uint32_t num_light_tris, const uint32_t* elem_of_prim);
// a scene with emitter images: the FLAT light triangles' `prim` becomes a pool element too (light_emission gathers the corner UVs by it; the
// smooth ones are remapped by launch_remap_light_tris, whose kernel and whose readers are as they were)
void launch_remap_flat_light_tris(hipStream_t stream, DevLightTri* light_tris, uint32_t num_light_tris, const uint32_t* elem_of_prim);
void launch_scatter_film(hipStream_t stream, const PassBuffers& pb, float* device_film, uint32_t film_width);

// Adaptive sampling (phx_adaptive in phx_xpu.h): the selection behind a round that ended at n samples of spp.  PassBuffers has no
// field for it; a pass over the rows that go on is the same kernels with other values in pix_xy, acc and num_pixels.
struct AdaptiveArgs {
  float* acc; uint32_t xstride, m2_offset, samples_offset;  // rows of the batch buffer: primary at 0, m2 and samples at their offsets
  const uint32_t* active; uint32_t num_active;              // the rows to decide, ascending; nullptr: 0 .. num_active - 1
  double q, g, tau, k; float n;                             // n / (n - 1), (a * n) / spp, the threshold, spp / n, (float)n
};
enum { PHX_ADAPTIVE_BLOCK = 256 };  // rows per workgroup of the selection
// Decides every active row, rescales those that stop and writes the indices of those that go on to `survivors` in the order of `active`
// (k_adaptive_count, k_adaptive_scan, k_adaptive_write).  block_scratch: ceil(num_active / PHX_ADAPTIVE_BLOCK) words; *total_out receives
// the number of survivors (a device word, or a host word the device can write).  num_active >= 1.
void launch_adaptive_select(hipStream_t stream, const AdaptiveArgs& A, uint32_t* block_scratch, uint32_t* survivors, uint32_t* total_out);
// n rows of xstride floats between home order and working order (working row w = home row idx[w]); to_home == 0 also carries pix_xy along
void launch_adaptive_move(hipStream_t stream, float* home, float* work, const uint32_t* home_xy, uint32_t* work_xy, const uint32_t* idx, uint32_t n,
                          uint32_t xstride, int to_home);
// channel "samples" = value in rows idx[0 .. n) of acc (idx == nullptr: rows 0 .. n - 1)
void launch_adaptive_mark(hipStream_t stream, float* acc, uint32_t xstride, uint32_t samples_offset, const uint32_t* idx, uint32_t n, float value);

// The film denoiser (phx_denoise in phx_xpu.h states the rule; denoise.hip).  Its state lives in working memory of the call, one
// record per pixel and array, so that a tap is three 16-byte loads: c = (C.rgb, 0) and v = (V.rgb, 0), both ping-pong; e = the luminance
// deviation e_x as the binary64 it is computed in (made once by the stage that writes V, read by the 3 x 3 of nine pixels), ping-pong;
// n = (N.xyz, valid ? 1 : 0), constant.  96 bytes a pixel.
struct DenoiseArgs {
  uint32_t width, height, xstride, normals_offset, m2_offset, samples_offset, spp, normal_power_log2;
  double sigma_l;
  float4* c[2]; float4* v[2]; double* e[2]; float4* n;
};
enum { PHX_DENOISE_BX = 64, PHX_DENOISE_BY = 4 };  // a workgroup's pixels: 4 rows of 64, a wave per row
// film -> state 0 (V from m2, valid, e)
void launch_denoise_pack(hipStream_t stream, const DenoiseArgs& A, const float* film);
// one iteration at step `step`: state `from` -> state `from ^ 1` (valid pixels only; the others' records are never read)
void launch_denoise_iteration(hipStream_t stream, const DenoiseArgs& A, int from, uint32_t step);
// state `from` -> "primary" and "m2" of the valid pixels of `film`, which holds the input film's floats
void launch_denoise_unpack(hipStream_t stream, const DenoiseArgs& A, int from, float* film);
// The guided filter (phx_denoise_guides in phx_xpu.h): the same three stages, instantiated with the guides.  flags = PHX_GUIDE_* (never
// 0 here: the launches above serve that).  DEMODULATE keeps nothing per pixel (the pack and unpack stages read the albedo from the guide film);
// PLANE keeps x = (position.xyz, distance), constant, and n.w = 2 instead of 1 for a valid pixel of coverage 0: 112 bytes a pixel.
struct DenoiseGuideArgs {
  const float* guides; uint32_t xstride, flags;
  double albedo_floor, tol_scale /* sigma_x * plane_scale */;
  float4* x;
};
void launch_denoise_pack_guided(hipStream_t stream, const DenoiseArgs& A, const DenoiseGuideArgs& G, const float* film);
void launch_denoise_iteration_guided(hipStream_t stream, const DenoiseArgs& A, const DenoiseGuideArgs& G, int from, uint32_t step);
void launch_denoise_unpack_guided(hipStream_t stream, const DenoiseArgs& A, const DenoiseGuideArgs& G, int from, float* film);

// The first-hit guide pass (phx_guides in phx_xpu.h; guides.hip): one launch, one thread per film pixel, 8 floats a pixel into `film`.
// pb carries what camera_ray reads and nothing else: pix_xy (row-major over the film), jitter, num_samples = G, seed.
void launch_guides(hipStream_t stream, const DevScene& sc, const PassBuffers& pb, float* film);
// its instantiations, for init_kernels_on_current_device (the per-lane traversal stack is dynamic LDS): -> how many were written to out[0 .. 3]
uint32_t guides_kernels(const void** out);

// Summary slots: the `counters` of launch_accumulate, launch_tile_map, launch_reproject and launch_outlier_clamp (film_pass.h has the device's side,
// film_calls.cpp's SummarySlots the host's).  nullptr, or PHX_SUMMARY_SLOTS zeroed slots of PHX_SUMMARY_SLOT_WORDS 64-bit words, a 128-byte
// line each: a workgroup adds its counts, in the order of the call's summary struct, to the first words of slot (workgroup id % SLOTS), and
// the caller sums the slots.  One line sustains some 90 atomics a microsecond, and a 2160p film has 32 400 workgroups.
enum { PHX_SUMMARY_SLOTS = 64, PHX_SUMMARY_SLOT_WORDS = 16 };

// Film accumulation (phx_accumulate in phx_xpu.h states the rule; accumulate.hip): one launch, a workgroup per span of
// PHX_ACCUMULATE_SPAN consecutive pixels.  The workgroup moves the span's floats of both films into LDS with coalesced 16-byte loads, a thread
// pools one pixel, and the span of acc goes back the same way.  xstride_* <= PHX_ACCUMULATE_MAX_XSTRIDE (accumulate_check.h: the check
// refuses more), which bounds the LDS of a launch: SPAN * 2 * MAX_XSTRIDE floats = 48 KB (accumulate.hip asserts it).
struct AccumulateArgs {
  uint64_t num_pixels;
  uint32_t xstride_a, normals_offset_a, m2_offset_a, samples_offset_a;
  uint32_t xstride_b, normals_offset_b, m2_offset_b, samples_offset_b;
  uint32_t spp_b;
  double tau, floor;
};
enum { PHX_ACCUMULATE_SPAN = 256 };
// counters: summary slots (above); pixels, invalid, converged, samples (phx_accumulate_summary)
void launch_accumulate(hipStream_t stream, const AccumulateArgs& A, float* acc, const float* frame_film, unsigned long long* counters);

// The tile map (phx_tile_map in phx_xpu.h states the rule; tile_map.hip): one launch, a workgroup of PHX_TILE_MAP_BLOCK threads
// per tile of the grid, tiles_x tiles a row.  Consecutive threads take consecutive pixels of a tile's row and read their 7 floats straight
// from memory; the workgroup reduces its counts and writes its own record, so no two workgroups write the same word but in the summary.
struct TileMapArgs {
  uint32_t width, height, xstride, m2_offset, samples_offset, tile_width, tile_height, tiles_x;
  double tau, floor;
};
enum { PHX_TILE_MAP_BLOCK = 256 };
// counters: summary slots (above); pixels, invalid, converged, samples, tiles, open (phx_tile_map_summary)
void launch_tile_map(hipStream_t stream, const TileMapArgs& A, uint32_t num_tiles, const float* acc, phx_tile_record* records, unsigned long long* counters);

// The display pass (phx_display in phx_xpu.h states the rule; display.hip, over display_rule.h): up to three launches on one stream
// with no host round trip between them.
//   launch_display_histogram  k_display_histogram: a grid sized by the device's compute units (at most PHX_DISPLAY_HIST_MAX_GROUPS workgroups,
//                             display_check.h) strides over spans of PHX_DISPLAY_SPAN pixels, counts into 258 LDS counters (the 256 bins,
//                             invalid, unlit) and adds the non-zero ones to slot (workgroup id % PHX_DISPLAY_SLOTS) of `slots`;
//                             k_display_exposure: one workgroup sums the slots and runs the exposure rule into `block`
//   launch_display_encode     k_display_encode: a thread per pixel, one 32-bit store per pixel, the scale read from `block` (nullptr: A.scale)
struct DisplayArgs {
  uint64_t num_pixels;
  uint32_t width, xstride, pitch_words /* 32-bit words per image row */, flags, tone;
  float scale, white, key, min_scale, max_scale;
  uint32_t low_q16, high_q16;
};
enum { PHX_DISPLAY_SPAN = 256, PHX_DISPLAY_SLOTS = 16, PHX_DISPLAY_SLOT_WORDS = 272 /* 258 counts, padded to whole 128-byte lines */ };
// what k_display_exposure leaves for the encode and for the host (phx_display_summary and the histogram)
struct DisplayBlock {
  unsigned long long histogram[256], pixels, invalid, unlit, counted;
  float scale; uint32_t from_histogram;
};
// slots: PHX_DISPLAY_SLOTS * PHX_DISPLAY_SLOT_WORDS zeroed 64-bit words; num_cus: the device's compute units
void launch_display_histogram(hipStream_t stream, const DisplayArgs& A, uint32_t num_cus, const float* film, unsigned long long* slots, DisplayBlock* block);
void launch_display_encode(hipStream_t stream, const DisplayArgs& A, const float* film, const DisplayBlock* block, uint32_t* image);

// Reprojection (phx_reproject in phx_xpu.h states the rule; reproject.hip): one launch, one thread per output pixel in binary64,
// workgroups of PHX_REPROJECT_BLOCK consecutive pixels.  The four taps are gathered straight from memory: neighbouring threads share them.
// ReprojectCamera: a camera as reproject_check.cpp derives it on the host (reproject_check.h).
struct ReprojectArgs {
  ReprojectCamera from, to;
  uint64_t num_pixels;
  uint32_t width, height, xstride_a, normals_offset_a, m2_offset_a, samples_offset_a, xstride_g;
  double sigma_plane, sigma_dist, max_history;
};
enum { PHX_REPROJECT_BLOCK = 256 };
// counters: summary slots (above); pixels, reused, no_geometry, disoccluded, samples (phx_reproject_summary)
void launch_reproject(hipStream_t stream, const ReprojectArgs& A, const float* acc_from, const float* guides_from, const float* guides_to, float* acc_to,
                      unsigned long long* counters);

// The outlier clamp (phx_outlier_clamp in phx_xpu.h states the rule; outlier_clamp.hip): one launch, a workgroup per tile of
// PHX_OUTLIER_TILE x PHX_OUTLIER_TILE output pixels, one thread per pixel in binary64.  The workgroup moves the rows of ref that its tile
// and a halo of `radius` pixels cover into LDS as they lie in memory (16-byte accesses where a row's range allows them), and every tap is
// read from there.  xstride_b <= PHX_OUTLIER_MAX_XSTRIDE and radius <= PHX_OUTLIER_MAX_RADIUS (outlier_clamp_check.h: the check refuses
// more) bound the LDS of a launch: 22 rows of at most 22 * 24 + 4 floats = 47 KB (outlier_clamp.hip asserts it).
struct OutlierClampArgs {
  uint32_t width, height, xstride_a, m2_offset_a, samples_offset_a, xstride_b;
  uint32_t flags, radius, trim, min_taps;
  uint32_t a_is_b;  // ref is film (or the call's copy of it): a thread reads its own pixel of A out of the tile in LDS
  double gamma, floor, clamped_history;
};
enum { PHX_OUTLIER_TILE = 16 };
// film_out may be film; ref shares no byte with film_out.  counters: summary slots (above); pixels, skipped, unbounded, inside, clamped,
// capped (phx_outlier_clamp_summary)
void launch_outlier_clamp(hipStream_t stream, const OutlierClampArgs& A, const float* film, const float* ref, float* film_out, unsigned long long* counters);

// stage-level entry points (synchronous helpers for the parity tests)
// light_pick + triangle_t::sample as k_shade_g's next-event block runs them: per item u3 = (pick, lu, lv) -> light, triangle inside it, (bu, bv), P, lpdf
void launch_light_sample(hipStream_t stream, const DevScene& sc, uint32_t n, const float* u3, uint32_t* light, uint32_t* tri, float* bary, float* P, float* pdf);
// light_pick + triangle_t::sample + light_emission as k_shade_g's next-event block runs them: per item u3 -> st (2 floats), e (3 floats)
void launch_light_emission(hipStream_t stream, const DevScene& sc, uint32_t n, const float* u3, float* st, float* e);
// SC_LIGHTS_ENV: light_pick + env_sample + env_emission as k_shade_g<.., ENV>'s next-event block runs them: per item u3 -> the pick, and for an
// environment pick the texel (i, j), (s, t), the direction, pdf = p_env * pdf_omega (0: no shadow ray) and the environment's e there (emission ex, ey, ez)
void launch_environment_sample(hipStream_t stream, const DevScene& sc, float ex, float ey, float ez, uint32_t n, const float* u3, uint32_t* light, uint32_t* texel,
                               float* st, float* dir, float* pdf, float* e);
void launch_trace_rays(hipStream_t stream, const DevScene& sc, uint32_t n, const float4* ro, const float4* rd, float4* hit, int any);
void launch_bsdf_f(hipStream_t stream, const DevMaterial* mat, uint32_t n, const float* n3, const float* wi3, const float* wo3, float* f3);
void launch_bsdf_sample(hipStream_t stream, const DevMaterial* mat, uint32_t n, const float* n3, const float* wi3, const float* u2,
                        float* wo3, float* f3, float* pdf, uint32_t* flags);
// every baked lobe's weight at a hit (3 x 8 floats per item, zero where the lobe is not there) and the mask of kept lobes; textures == nullptr: a
// scene without a texture table (st is not read)
void launch_lobe_weights(hipStream_t stream, const DevMaterial* mat, const DevTexture* textures, const float4* texels, const uint32_t* lobe_tex, uint32_t n,
                         const float* n3, const float* wi3, const float* st, float* w, uint32_t* kept);
void launch_texture_lookup(hipStream_t stream, const DevTexture* textures, const float4* texels, uint32_t tex, uint32_t n, const float* st, float* rgb);
void launch_environment_lookup(hipStream_t stream, const DevTexture* textures, const float4* texels, uint32_t tex, uint32_t mapping, float ex, float ey, float ez,
                               uint32_t n, const float* dirs, float* rgb);

}  // namespace phx
