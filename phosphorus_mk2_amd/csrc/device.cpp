// device.cpp — host side of the gfx950 device: the C ABI of include/phx_xpu.h, its device object and preprocess.
//
// Mirrors cpu_t (reference src/xpu/cpu.cpp:208-248): preprocess() flattens the scene and builds the accelerator (cpu.cpp:35-44), start() hands
// the frame to the device's driver thread, join() waits for it.  Here: the last error, discovery, the life cycle of a phx_device, preprocess
// (build_tree, commit_scene), start / join / statistics, the adaptive setting, the tile queue and phx_dev_copy_bvh.
// The rest of the ABI lives beside this file, over device_internal.h: frame_driver.cpp is the driver thread and the frame (it drains the shared
// tile queue, cpu.cpp:223-238, in batches of many tiles, each carried through the wavefront kernels of trace.hip, shade_lambert.hip,
// shade_general.hip, film_hooks.hip, and hands finished tiles to the film sink, cpu.cpp:201), stage_hooks.cpp the scene-reading stage hooks,
// film_calls.cpp the film calls no frame launches (the denoiser of denoise.hip, the guide pass of guides.hip, film accumulation of accumulate.hip).
// What needs no device: scene_flatten.cpp is the host-only half of preprocess, frame_plan.cpp that of the frame driver (the film's pixel layout,
// the pixel cap, the batch cutter, the pass schedule), denoise_check.cpp, guides_check.cpp and accumulate_check.cpp the argument checks of the film calls, over film_checks.h.
// There is no CPU rendering path in this library: without a gfx950 device every entry point fails.
#include "device_internal.h"
#include "bvh_build.h"
#include "bvh_gpu.h"
#include "film_checks.h"
#include "scene_flatten.h"

#include <atomic>
#include <cfloat>
#include <cstdio>
#include <cstring>

using namespace phx;

#ifndef PHX_TEST_HOOKS
#define PHX_TEST_HOOKS 0  /* 1 only in the twin library libphx_hip_hooks.so (fault injection for the tests); never in the product build */
#endif

namespace phx {

thread_local std::string g_error;  // (device_internal.h)

int fail(int code, const std::string& msg) { g_error = msg; return code; }

}  // namespace phx

struct phx_tiles {
  std::vector<phx_tile> tiles;
  std::atomic<uint32_t> cursor{0};
};

// ---- preprocess ---------------------------------------------------------------------------------------
// Three stages: the state checks, flatten_scene (scene_flatten.cpp: validation and everything derived on the host — a refusal leaves the
// device and its previous scene untouched), and commit_scene, which builds the tree and replaces the device's tables.
namespace {

// PHX_BVH_AUTO: the device builder (bvh_gpu.hip) unless the scene is tiny.  Round 2 kept the host's binned SAH for scenes up to 2 M
// triangles because its trees traced 3-5 % faster on mesh-like scenes; with extended Morton codes (the size of a primitive as a
// fourth coordinate) the device trees are as fast or faster everywhere measured — soups -2 ... -7 % k_trace time, the showroom
// -3 % — and they are built in milliseconds (profiles/r03_z_emc_probe.log, r03_za_builder_ab.log).
// Fills d_pool, the tree's words of d->scene and of the statistics, and elem_of_prim: the pool index of every primitive's triangle record (the
// shade records and the normals table are laid out by it).  d_prim_material holds the scene's material words already.
int build_tree(phx_device* d, const FlatScene& fs, DevBuf<uint32_t>& elem_of_prim) {
  int rc;
  const uint32_t builder = d->opt.bvh_builder;
  const uint32_t ntri = (uint32_t)fs.prim_material.size();
  bool want_host = builder == PHX_BVH_HOST_SAH || (builder == PHX_BVH_AUTO && ntri < 64u);
  GpuBvh g{};
  if (!want_host) {
    // the triangles go up once (36 B each); the tree is built and stays in HBM (bvh_gpu.hip)
    DevBuf<float> d_abc;
    char msg[256] = {0};
    rc = d_abc.upload(fs.abc);
    int brc = rc ? (rc == PHX_ERR_OOM ? (int)BVH_GPU_RECOVERABLE : 1) : 0;
    if (rc) std::snprintf(msg, sizeof(msg), "%s", g_error.c_str());
#if PHX_TEST_HOOKS
    // test hook, compiled into the twin library libphx_hip_hooks.so only (tests/test_gpu_parity.py): makes the device build report a
    // recoverable or a fatal failure
    if (const char* how = std::getenv("PHX_TEST_FAIL_DEVICE_BUILD")) {
      brc = std::strcmp(how, "fatal") == 0 ? 1 : (int)BVH_GPU_RECOVERABLE;
      std::snprintf(msg, sizeof(msg), "forced %s failure (PHX_TEST_FAIL_DEVICE_BUILD)", brc == 1 ? "fatal" : "recoverable");
    }
#endif
    if (!brc && elem_of_prim.alloc(ntri)) brc = (int)BVH_GPU_RECOVERABLE, std::snprintf(msg, sizeof(msg), "%s", g_error.c_str());
    if (!brc) brc = build_bvh8_gpu(d->stream, d_abc.p, d->d_prim_material.p, ntri, &g, msg, sizeof(msg), elem_of_prim.p);
    if (brc) {
      // An explicit DEVICE_LBVH request fails loudly, and so does AUTO when the device builder reports anything but a RECOVERABLE cause
      // (a HIP error from a launch or a sync, lost triangles: bugs that a silent 0.6-7 s host build would hide).  Under AUTO a device
      // build that cannot get its scratch memory, or meets a tree deeper than its tables, falls back to the host's binned-SAH builder
      // — which handled every scene before the device builder became the default — and says so: on stderr, in phx_last_error of this
      // thread (a successful call leaves the text in place) and in phx_stats::bvh_built_on_device.
      if (builder != PHX_BVH_AUTO || brc != (int)BVH_GPU_RECOVERABLE) return fail(rc ? rc : PHX_ERR_DEVICE, std::string("device BVH build: ") + msg);
      (void)hipGetLastError();  // a failed hipMalloc leaves its error behind
      g_error = std::string("device BVH build fell back to the host builder: ") + msg;
      std::fprintf(stderr, "libphx_hip: %s\n", g_error.c_str());
      want_host = true;
    }
  }
  DevScene& sc = d->scene;
  if (want_host) {
    Bvh8 bvh;
    const int threads = (int)std::max(1u, std::thread::hardware_concurrency());
    build_bvh8(fs.abc.data(), ntri, bvh, threads, fs.prim_material.data());
    if ((rc = d->d_pool.upload(bvh.pool))) return rc;
    if ((rc = elem_of_prim.upload(bvh.elem_of_prim))) return rc;
    sc.stack_levels = bvh.depth; sc.num_elems = (uint32_t)bvh.pool.size(); sc.grid = bvh.grid;
    d->bvh_nodes = bvh.num_nodes; d->bvh_cost_model = bvh.cost; d->bvh_built_on_device = 0;
  } else {
    d->d_pool.adopt(g.pool, g.num_elems);
    sc.stack_levels = g.depth; sc.num_elems = g.num_elems; sc.grid = g.grid;
    d->bvh_nodes = g.num_nodes; d->bvh_cost_model = g.cost; d->bvh_built_on_device = 1;
  }
  sc.pool = reinterpret_cast<const uint32_t*>(d->d_pool.p);
  sc.tris = reinterpret_cast<const TriRec*>(d->d_pool.p);
  d->bvh_bytes = (uint64_t)sc.num_elems * sizeof(PoolElem);
  return PHX_OK;
}

// The tables of floats that ride directly behind the light records, each padded to whole records of the light table: the selection table
// (shade_common.h: light_pcdf), then the area CDF (light_cdf), one float per light triangle.
void append_light_tables(const DevScene& sc, FlatScene& fs) {
  auto append_behind_lights = [&](const std::vector<float>& table) {
    const size_t nl = fs.lights.size();
    fs.lights.resize(nl + (table.size() * sizeof(float) + sizeof(DevLight) - 1) / sizeof(DevLight), DevLight{});
    std::memcpy(static_cast<void*>(fs.lights.data() + nl), table.data(), table.size() * sizeof(float));
  };
  if (sc.any_tex & SC_LIGHTS_BY_POWER) append_behind_lights(fs.light_pcdf);
  if (sc.any_tex & SC_LIGHTS_BY_AREA) append_behind_lights(fs.light_cdf);
}

// Replaces the device's scene by `fs`.  From its first line to its last the device has NO scene (preprocessed == false): a failure on the
// way — the device builder's fatal error, a tree too deep, a hipMalloc that fails — leaves buffers of the old and the new scene mixed, and
// start / the stage hooks answer PHX_ERR_STATE until a preprocess succeeds.
int commit_scene(phx_device* d, FlatScene& fs) {
  int rc;
  d->preprocessed = false;
  DevScene& sc = d->scene = fs.scene;
  const uint32_t ntri = (uint32_t)fs.prim_material.size();
  const bool any_tex = (sc.any_tex & SC_TEX_LOBES) != 0, any_image = (sc.any_tex & SC_TEX_ANY) != 0;
  if ((rc = d->d_prim_material.upload(fs.prim_material))) return rc;
  const auto t_bvh0 = Clock::now();
  DevBuf<uint32_t> d_elem_of_prim;
  if ((rc = build_tree(d, fs, d_elem_of_prim))) return rc;
  d->bvh_build_ms = ms_between(t_bvh0, Clock::now());
  // k_trace / k_trace_rays keep one pending sibling group per level and lane in LDS (bvh8.h: PHX_MAX_BVH_DEPTH)
  if (sc.stack_levels > PHX_MAX_BVH_DEPTH)
    return fail(PHX_ERR_ARG, "tree too deep: " + std::to_string(sc.stack_levels) + " levels, the traversal stack in LDS holds " + std::to_string(PHX_MAX_BVH_DEPTH));
  if ((rc = d->d_materials.upload(fs.materials))) return rc;
  append_light_tables(sc, fs);
  if ((rc = d->d_lights.upload(fs.lights)) || (rc = d->d_light_tris.upload(fs.light_tris))) return rc;
  // what shading reads of a hit triangle, 16 bytes per POOL ELEMENT: geometric normal + material word
  if ((rc = d->d_elem_shade.alloc(sc.num_elems))) return rc;
  launch_build_shade_recs(d->stream, sc.tris, d_elem_of_prim.p, d->d_elem_shade.p, ntri);
  HIPCHK(hipGetLastError());
  // Vertex normals by POOL ELEMENT (the index a hit record carries), so that the shade kernels request them with the triangle record and not
  // after it; the smooth light triangles' `prim` becomes a pool index too (shading_normal on the light's face, spt.hpp:212-255).  Corner UVs
  // likewise (textured lobes only).  The tables in primitive order live until the stream has been synchronised below.
  DevBuf<float> d_prim_normals; DevBuf<float2> d_prim_uv;
  if (fs.any_smooth) {
    if ((rc = d_prim_normals.upload(fs.prim_normals)) || (rc = d->d_elem_normals.alloc(9 * (size_t)sc.num_elems))) return rc;
    launch_permute_normals(d->stream, d_prim_normals.p, d_elem_of_prim.p, d->d_elem_normals.p, ntri);
    launch_remap_light_tris(d->stream, d->d_light_tris.p, (uint32_t)fs.light_tris.size(), d_elem_of_prim.p);
  } else {
    d->d_elem_normals.release();
  }
  if (any_tex) {
    if ((rc = d_prim_uv.upload(fs.prim_uv)) || (rc = d->d_elem_uv.alloc(3 * (size_t)sc.num_elems)) || (rc = d->d_lobe_tex.upload(fs.lobe_tex))) return rc;
    launch_permute_uvs(d->stream, d_prim_uv.p, d_elem_of_prim.p, d->d_elem_uv.p, ntri);
    // emitter images: every light triangle reaches its corner UVs by pool element (the smooth ones were remapped above)
    if (fs.any_emit_tex) launch_remap_flat_light_tris(d->stream, d->d_light_tris.p, (uint32_t)fs.light_tris.size(), d_elem_of_prim.p);
  } else {
    d->d_elem_uv.release(); d->d_lobe_tex.release();
  }
  HIPCHK(hipGetLastError());
  if (fs.any_emit_tex) { if ((rc = d->d_mat_emit_tex.upload(fs.mat_emit_tex))) return rc; } else d->d_mat_emit_tex.release();
  if (sc.any_tex & SC_LIGHTS_ENV) { if ((rc = d->d_env_cdf.upload(fs.env_cdf))) return rc; } else d->d_env_cdf.release();
  if (any_image) {  // the texture table and the texels, and the one record through which the shade kernels find them
    if ((rc = d->d_textures.upload(fs.textures)) || (rc = d->d_texels.upload(fs.texels))) return rc;
    d->tex_scene = DevTexScene{any_tex ? d->d_elem_uv.p : nullptr, d->d_textures.p, d->d_texels.p, any_tex ? d->d_lobe_tex.p : nullptr,
                               fs.env_tex ? fs.env_tex - 1u : 0u, fs.env_mapping, fs.any_emit_tex ? 1u : 0u, fs.env_p,
                               fs.any_emit_tex ? d->d_mat_emit_tex.p : nullptr, (sc.any_tex & SC_LIGHTS_ENV) ? d->d_env_cdf.p : nullptr};
    if ((rc = d->d_tex_scene.upload(std::vector<DevTexScene>{d->tex_scene}))) return rc;
  } else {
    d->d_textures.release(); d->d_texels.release(); d->d_tex_scene.release();
  }
  if (sc.diffuse_only == 2 && (rc = d->d_mat_lite.upload(fs.mat_lite))) return rc;
  HIPCHK(hipStreamSynchronize(d->stream));  // d_elem_of_prim and the tables in primitive order go out of scope below

  sc.elem_normals = fs.any_smooth ? d->d_elem_normals.p : nullptr;
  sc.elem_shade = d->d_elem_shade.p;
  sc.materials = d->d_materials.p;
  sc.mat_lite = sc.diffuse_only == 2 ? d->d_mat_lite.p : nullptr;
  sc.lights = d->d_lights.p; sc.light_tris = d->d_light_tris.p;
  sc.tex = any_image ? d->d_tex_scene.p : nullptr;
  {
    hipDeviceProp_t prop; HIPCHK(hipGetDeviceProperties(&prop, d->hip_device));
    sc.num_cus = (uint32_t)prop.multiProcessorCount;
  }
  d->plan = trace_plan(sc);
  if (d->plan.spill_threads) {  // stack levels below the ones k_trace keeps in LDS (trace.hip: trace_plan)
    if ((rc = d->d_spill.alloc((size_t)d->plan.spill_threads * (d->plan.levels - d->plan.lds_levels)))) return rc;
    sc.stack_spill = d->d_spill.p; sc.spill_stride = d->plan.spill_threads;
  }
  d->num_materials = (uint32_t)fs.materials.size();
  d->mat_masked = std::move(fs.mat_masked);
  d->num_textures = any_image ? (uint32_t)fs.textures.size() : 0;
  d->env_tex = fs.env_tex; d->env_mapping = fs.env_mapping;
  for (int c = 0; c < 3; ++c) d->env_e[c] = fs.env_e[c];
  d->num_triangles = ntri;
  d->geometry = std::move(fs.fingerprint);
  // Who reads (u, v) of a hit: a smooth face's normal, the corner UVs' interpolation (lobe images, masks, emitter images: SC_TEX_LOBES) and a
  // per-hit material — the classes flatten_scene made for launch_shade.  PHX_HIT_UV=1 (tests only) carries the stream on a scene that does not.
  {
    const char* force = std::getenv("PHX_HIT_UV");
    d->hit_uv = fs.any_smooth || any_tex || sc.any_per_hit != 0 || (force && std::atoi(force) != 0);
  }
  d->budget_bytes = 0;  // the next frame asks the device again how much memory is free
  d->preprocessed = true;
  return PHX_OK;
}

// Brings the device's scene to the moved geometry `fs` (flatten_geometry's: accepted against d->geometry).  Refit: the pool is refitted in
// place (bvh_refit.hip).  Rebuild: build_tree makes a new one, the corner UVs are carried over by the old and the new elem_of_prim, the
// traversal plan and the spill buffer are recomputed.  Then the commit's geometry half, by commit_scene's own launches: shade records,
// normals by pool element, the light tables and the light triangles' remaps.  As in commit_scene the device has no scene from the first
// device write to the last line.  ms: uploads, device work (host clock; every stretch ends in a synchronise).  Under a rebuild the triangles go
// up inside build_tree, so their upload is counted with the device's work.
int update_scene_geometry(phx_device* d, FlatScene& fs, uint32_t mode, phx_geometry_summary* sum, double* ms) {
  int rc;
  DevScene& sc = d->scene;
  const uint32_t ntri = (uint32_t)fs.prim_material.size();
  const bool any_tex = (sc.any_tex & SC_TEX_LOBES) != 0, any_image = (sc.any_tex & SC_TEX_ANY) != 0, rebuild = mode == PHX_UPDATE_REBUILD;
  double upload_ms = 0.0, device_ms = 0.0;
  auto timed = [](double& acc, auto&& body) { const auto t = Clock::now(); const int r = body(); acc += ms_between(t, Clock::now()); return r; };
  char msg[256] = {0};
  DevBuf<float> d_abc, d_prim_normals; DevBuf<uint32_t> d_elem_of_prim; DevBuf<float2> d_prim_uv;
  if (!rebuild) {
    if ((rc = timed(upload_ms, [&] { return d_abc.upload(fs.abc); })) || (rc = d_elem_of_prim.alloc(ntri))) return rc;
    d->preprocessed = false;
    GpuRefit r{};
    const int brc = timed(device_ms, [&] { return refit_bvh8_gpu(d->stream, d->d_pool.p, sc.num_elems, d_abc.p, ntri, d_elem_of_prim.p, &r, msg, sizeof(msg)); });
    if (brc) return fail(brc == (int)BVH_GPU_RECOVERABLE ? PHX_ERR_OOM : PHX_ERR_DEVICE, std::string("update_geometry: ") + msg);
    sc.grid = r.grid;
  } else {
    if (any_tex) {  // the corner UVs in primitive order, read back through the old tree's elem_of_prim: no UV value is read from the scene again
      DevBuf<uint32_t> d_old;
      if ((rc = d_old.alloc(ntri)) || (rc = d_prim_uv.alloc(3 * (size_t)ntri))) return rc;
      const int brc = timed(device_ms, [&] {
        const int e = pool_elem_of_prim_gpu(d->stream, d->d_pool.p, sc.num_elems, ntri, d_old.p, msg, sizeof(msg));
        if (e) return e;
        launch_gather_rows(d->stream, reinterpret_cast<const float*>(d->d_elem_uv.p), d_old.p, reinterpret_cast<float*>(d_prim_uv.p), ntri, 6, sc.num_elems);
        return hipStreamSynchronize(d->stream) == hipSuccess ? 0 : 1;
      });
      if (brc) return fail(brc == (int)BVH_GPU_RECOVERABLE ? PHX_ERR_OOM : PHX_ERR_DEVICE, std::string("update_geometry: ") + msg);
    }
    d->preprocessed = false;
    // Everything sized by the tree is released where the new tree's size differs, not kept at the larger of the two (DevBuf grows only): after
    // a rebuild the device holds what a fresh preprocess of the moved scene holds.  The old pool has been read for the last time above.
    const uint32_t elems_before = sc.num_elems;
    d->d_pool.release();
    const auto t_bvh0 = Clock::now();
    if ((rc = build_tree(d, fs, d_elem_of_prim))) return rc;
    d->bvh_build_ms = ms_between(t_bvh0, Clock::now()); device_ms += d->bvh_build_ms;
    if (sc.stack_levels > PHX_MAX_BVH_DEPTH)
      return fail(PHX_ERR_ARG, "tree too deep: " + std::to_string(sc.stack_levels) + " levels, the traversal stack in LDS holds " + std::to_string(PHX_MAX_BVH_DEPTH));
    if (sc.num_elems != elems_before) { d->d_elem_shade.release(); d->d_elem_normals.release(); d->d_elem_uv.release(); }  // sized by pool element
    if ((rc = d->d_elem_shade.alloc(sc.num_elems))) return rc;
    if (fs.any_smooth && (rc = d->d_elem_normals.alloc(9 * (size_t)sc.num_elems))) return rc;
    if (any_tex && (rc = d->d_elem_uv.alloc(3 * (size_t)sc.num_elems))) return rc;
  }
  append_light_tables(sc, fs);
  rc = timed(upload_ms, [&] {
    int r = d->d_lights.upload(fs.lights);
    if (!r) r = d->d_light_tris.upload(fs.light_tris);
    if (!r && fs.any_smooth) r = d_prim_normals.upload(fs.prim_normals);
    return r;
  });
  if (rc) return rc;
  const bool any_emit_tex = d->geometry.any_emit_tex;
  rc = timed(device_ms, [&]() -> int {
    launch_build_shade_recs(d->stream, reinterpret_cast<const TriRec*>(d->d_pool.p), d_elem_of_prim.p, d->d_elem_shade.p, ntri);
    if (fs.any_smooth) {
      launch_permute_normals(d->stream, d_prim_normals.p, d_elem_of_prim.p, d->d_elem_normals.p, ntri);
      launch_remap_light_tris(d->stream, d->d_light_tris.p, (uint32_t)fs.light_tris.size(), d_elem_of_prim.p);
    }
    if (any_tex) {
      if (rebuild) launch_permute_uvs(d->stream, d_prim_uv.p, d_elem_of_prim.p, d->d_elem_uv.p, ntri);
      if (any_emit_tex) launch_remap_flat_light_tris(d->stream, d->d_light_tris.p, (uint32_t)fs.light_tris.size(), d_elem_of_prim.p);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(d->stream));  // d_elem_of_prim and the tables in primitive order go out of scope below
    return PHX_OK;
  });
  if (rc) return rc;
  if (any_image && ((sc.any_tex & SC_LIGHTS_ENV) || (rebuild && any_tex))) {  // the environment's interval moved with the bounds; a rebuild may have moved elem_uv
    d->tex_scene.env_p = fs.env_p; d->tex_scene.elem_uv = any_tex ? d->d_elem_uv.p : nullptr;
    if ((rc = timed(upload_ms, [&] { return d->d_tex_scene.upload(std::vector<DevTexScene>{d->tex_scene}); }))) return rc;
  }
  sc.elem_normals = fs.any_smooth ? d->d_elem_normals.p : nullptr;
  sc.elem_shade = d->d_elem_shade.p;
  sc.lights = d->d_lights.p; sc.light_tris = d->d_light_tris.p;
  if (rebuild) {
    sc.stack_spill = nullptr; sc.spill_stride = 0;
    d->plan = trace_plan(sc);
    const size_t spill = d->plan.spill_threads ? (size_t)d->plan.spill_threads * (d->plan.levels - d->plan.lds_levels) : 0;
    if (spill != d->d_spill.n) d->d_spill.release();
    if (spill) {
      if ((rc = d->d_spill.alloc(spill))) return rc;
      sc.stack_spill = d->d_spill.p; sc.spill_stride = d->plan.spill_threads;
    }
    d->budget_bytes = 0;
  }
  if (sum) {
    *sum = phx_geometry_summary{mode, ntri, (uint32_t)d->bvh_nodes, sc.stack_levels, sc.num_lights, (uint32_t)fs.light_tris.size(),
                                {fs.bounds[0], fs.bounds[1], fs.bounds[2], fs.bounds[3], fs.bounds[4], fs.bounds[5]}, tri_box_inflation(fs.bounds, fs.bounds + 3)};
  }
  // the call's own device buffers go here, inside the device's timer, not when the function returns
  (void)timed(device_ms, [&] { d_abc.release(); d_elem_of_prim.release(); d_prim_normals.release(); d_prim_uv.release(); return 0; });
  ms[1] = upload_ms; ms[2] = device_ms;
  d->preprocessed = true;
  return PHX_OK;
}

}  // namespace

extern "C" {

const char* phx_last_error(void) { return g_error.c_str(); }  // last error of the CALLING thread

int phx_discover(const phx_options* options, int* num_devices) {
  if (!num_devices) return fail(PHX_ERR_ARG, "phx_discover: null out pointer");
  *num_devices = 0;
  if (options && options->host_only) return PHX_OK;  // --no-gpu (src/core.cpp:49-52)
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) { (void)hipGetLastError(); return fail(PHX_ERR_NO_DEVICE, std::string("hipGetDeviceCount: ") + hipGetErrorString(e)); }
  int usable = 0;
  for (int i = 0; i < n; ++i) {
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, i) == hipSuccess && std::strncmp(p.gcnArchName, "gfx950", 6) == 0) ++usable;
  }
  *num_devices = usable;
  if (!usable) return fail(PHX_ERR_NO_DEVICE, "no gfx950 (MI355X) device visible");
  return PHX_OK;
}

phx_device* phx_dev_make(const phx_options* options) {
  if (!options) { fail(PHX_ERR_ARG, "phx_dev_make: null options"); return nullptr; }
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n == 0) { (void)hipGetLastError(); fail(PHX_ERR_NO_DEVICE, "no HIP device: the gfx950 path cannot run"); return nullptr; }
  int dev = options->device_ordinal;
  if (dev < 0) { if (hipGetDevice(&dev) != hipSuccess) dev = 0; }
  if (dev >= n) { fail(PHX_ERR_ARG, "device_ordinal out of range"); return nullptr; }
  hipDeviceProp_t p;
  if (hipGetDeviceProperties(&p, dev) != hipSuccess || std::strncmp(p.gcnArchName, "gfx950", 6) != 0) {
    fail(PHX_ERR_NO_DEVICE, std::string("device is not gfx950: ") + p.gcnArchName);
    return nullptr;
  }
  DeviceScope on(dev);  // the caller's current device is restored when this returns
  if (!on.ok) { fail(PHX_ERR_DEVICE, "hipSetDevice failed"); return nullptr; }
  phx_device* d = new (std::nothrow) phx_device();
  if (!d) { fail(PHX_ERR_OOM, "host memory allocation failed"); return nullptr; }
  d->opt = *options; d->hip_device = dev;
  if (d->opt.samples_per_pixel == 0) d->opt.samples_per_pixel = 16;
  if (d->opt.paths_per_sample == 0) d->opt.paths_per_sample = 1;
  if (d->opt.path_depth == 0) d->opt.path_depth = 9;
  if (hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking) != hipSuccess) { delete d; fail(PHX_ERR_DEVICE, "hipStreamCreate failed"); return nullptr; }
  // dynamic-LDS limit of the traversal kernels: a per-device, per-kernel attribute, so it is set for every device made
  const hipError_t ae = init_kernels_on_current_device();
  if (ae != hipSuccess) { delete d; fail(PHX_ERR_DEVICE, std::string("hipFuncSetAttribute(MaxDynamicSharedMemorySize): ") + hipGetErrorString(ae)); return nullptr; }
  return d;
}

void phx_dev_destroy(phx_device* dev) {
  if (!dev) return;
  DeviceScope on(dev->hip_device);
  delete dev;
}

int phx_dev_preprocess(phx_device* d, const phx_scene* s) {
  return guarded([&]() -> int {
    if (!d || !s) return fail(PHX_ERR_ARG, "preprocess: null argument");
    if (d->running) return fail(PHX_ERR_STATE, "preprocess while a frame is running");
    const auto t0 = Clock::now();
    FlatScene fs; std::string why;
    if (const int rc = flatten_scene(*s, d->opt, fs, why)) return fail(rc, why);
    if (d->opt.bvh_builder > PHX_BVH_HOST_SAH) return fail(PHX_ERR_ARG, "unknown bvh_builder");
    DeviceScope on(d->hip_device);
    if (!on.ok) return fail(PHX_ERR_DEVICE, "hipSetDevice failed");
    if (const int rc = commit_scene(d, fs)) return rc;
    d->preprocess_ms = ms_between(t0, Clock::now());
    return PHX_OK;
  });
}

int phx_dev_update_geometry(phx_device* d, const phx_scene* s, const phx_geometry_update* u, phx_geometry_summary* summary) {
  return guarded([&]() -> int {
    if (!s || !u) return fail(PHX_ERR_ARG, "update_geometry: null argument");
    // (the struct's own refusals need no device: they come first, as the film calls' checks do)
    if (u->mode > PHX_UPDATE_REBUILD) return fail(PHX_ERR_ARG, "update_geometry: mode is outside its range (phx_geometry_update)");
    if (u->reserved[0] || u->reserved[1] || u->reserved[2]) return fail(PHX_ERR_ARG, "update_geometry: reserved is outside its range (phx_geometry_update): it must be 0");
    if (!d) return fail(PHX_ERR_ARG, "update_geometry: null device");
    if (!d->preprocessed) return fail(PHX_ERR_STATE, "update_geometry before preprocess");
    if (d->running) return fail(PHX_ERR_STATE, "update_geometry while a frame is running");
    const auto t0 = Clock::now();
    double ms[4] = {0.0, 0.0, 0.0, 0.0};
    FlatScene fs; std::string why;
    if (const int rc = flatten_geometry(*s, d->opt, d->geometry, fs, why)) return fail(rc, why);
    ms[0] = ms_between(t0, Clock::now());
    DeviceScope on(d->hip_device);
    if (!on.ok) return fail(PHX_ERR_DEVICE, "hipSetDevice failed");
    if (const int rc = update_scene_geometry(d, fs, u->mode, summary, ms)) return rc;
    ms[3] = ms_between(t0, Clock::now());
    for (int k = 0; k < 4; ++k) d->update_geometry_ms[k] = ms[k];
    return PHX_OK;
  });
}
int phx_dev_update_geometry_times(const phx_device* d, double* ms) {
  if (!d || !ms) return fail(PHX_ERR_ARG, "update_geometry_times: null argument");
  for (int k = 0; k < 4; ++k) ms[k] = d->update_geometry_ms[k];
  return PHX_OK;
}

// The camera is nine host-side words of d->scene (scene_flatten.cpp: flatten_camera) and nothing on the device: every launch takes the
// scene by value, rebuilds its camera rays from those words and picks its lens or pinhole instantiation then (launch_trace_primary,
// launch_shade, launch_guides); trace_plan reads the tree alone, and the pixel, tile and jitter tables the film's size and the seed.
int phx_dev_set_camera(phx_device* d, const phx_camera* c) {
  return guarded([&]() -> int {
    if (!d || !c) return fail(PHX_ERR_ARG, "set_camera: null argument");
    if (!d->preprocessed) return fail(PHX_ERR_STATE, "set_camera before preprocess");
    if (d->running) return fail(PHX_ERR_STATE, "set_camera while a frame is running");
    DevScene sc = d->scene; std::string why;
    if (const int rc = flatten_camera(*c, sc, why)) return fail(rc, why);
    if (sc.width != d->scene.width || sc.height != d->scene.height)
      return fail(PHX_ERR_ARG, "set_camera: the film size must stay the preprocessed scene's (" + std::to_string(d->scene.width) + " x " + std::to_string(d->scene.height) + ")");
    d->scene = sc;
    return PHX_OK;
  });
}

int phx_dev_start(phx_device* d, const phx_frame* f) {
  if (!d || !f) return fail(PHX_ERR_ARG, "start: null argument");
  if (!d->preprocessed) return fail(PHX_ERR_STATE, "start before preprocess");
  if (d->running) return fail(PHX_ERR_STATE, "start while a frame is running");
  if (!f->next_tile) return fail(PHX_ERR_ARG, "frame without a tile queue");
  if (!f->add_tile && !f->device_film && !f->host_film) return fail(PHX_ERR_ARG, "frame without a film sink");
  if (f->primary_components != 3 && f->primary_components != 4) return fail(PHX_ERR_ARG, "primary channel must have 3 or 4 components");
  if (f->moments_channel > 1) return fail(PHX_ERR_ARG, "moments_channel must be 0 or 1");
  if (d->adaptive_on && f->moments_channel != 1) return fail(PHX_ERR_ARG, "adaptive sampling is on (phx_dev_set_adaptive): the frame must have moments_channel == 1");
  d->frame = *f;
  {
    static const int timing_env = [] { const char* v = std::getenv("PHX_KERNEL_TIMING"); return v ? std::atoi(v) : -1; }();
    d->kernel_timing = timing_env >= 0 ? timing_env != 0 : true;
  }
  d->t_start = Clock::now();
  const int rc = guarded([&]() {
    if (!d->driver.joinable()) d->driver = std::thread([d]() { d->driver_loop(); });  // the first frame of this device starts its driver
    return (int)PHX_OK;
  });
  if (rc != PHX_OK) return rc;  // the driver thread could not be created
  {
    std::lock_guard<std::mutex> lk(d->mu);
    d->running = true; d->frame_status = PHX_OK; d->frame_done = false; d->frame_pending = true;
  }
  d->cv.notify_all();
  return PHX_OK;
}

int phx_dev_join(phx_device* d) {
  if (!d) return fail(PHX_ERR_ARG, "join: null device");
  if (!d->running) return fail(PHX_ERR_STATE, "join without start");
  {
    std::unique_lock<std::mutex> lk(d->mu);
    d->cv.wait(lk, [d]() { return d->frame_done; });
    d->running = false;
  }
  if (d->frame_status != PHX_OK) g_error = d->frame_error;
  return d->frame_status;
}

int phx_dev_get_stats(const phx_device* d, phx_stats* out) {
  if (!d || !out) return fail(PHX_ERR_ARG, "get_stats: null argument");
  *out = d->stats;
  out->bvh_nodes = d->bvh_nodes; out->bvh_bytes = d->bvh_bytes; out->triangles = d->num_triangles;
  out->preprocess_ms = d->preprocess_ms; out->bvh_build_ms = d->bvh_build_ms;
  out->trace_block = d->plan.block; out->trace_ntop = d->plan.ntop; out->trace_levels = d->plan.levels; out->trace_lds_levels = d->plan.lds_levels; out->trace_stack_packed = d->plan.packed;
  out->trace_waves_per_cu = (uint64_t)d->plan.wg_per_cu * (d->plan.block / 64u); out->bvh_depth = d->scene.stack_levels;
  out->paths_in_flight = d->paths_in_flight;
  out->bvh_cost_model = d->bvh_cost_model; out->bvh_built_on_device = d->bvh_built_on_device;
  out->shade_general = d->scene.diffuse_only ? 0 : 1;
  out->device_bytes = d->device_bytes();
  return PHX_OK;
}

uint32_t phx_abi_sizeof(int which) {
  switch (which) {
    case 0: return sizeof(phx_options); case 1: return sizeof(phx_lobe); case 2: return sizeof(phx_material);
    case 3: return sizeof(phx_face_set); case 4: return sizeof(phx_mesh); case 5: return sizeof(phx_camera);
    case 6: return sizeof(phx_scene); case 7: return sizeof(phx_tile); case 8: return sizeof(phx_frame);
    case 9: return sizeof(phx_stats); case 10: return sizeof(phx_texture); case 11: return sizeof(phx_adaptive);
    case 13: return sizeof(phx_denoise);  // (12 stays unused: tests/test_adaptive_sampling.py pins it to 0)
    case 15: return sizeof(phx_guides); case 16: return sizeof(phx_denoise_guides);  // (14 likewise: tests/test_denoise.py)
    case 18: return sizeof(phx_accumulate);  // (17 likewise: tests/test_guides.py)
    case 19: return sizeof(phx_display); case 20: return sizeof(phx_display_summary);
    case 21: return sizeof(phx_reproject); case 22: return sizeof(phx_reproject_summary);
    case 23: return sizeof(phx_outlier_clamp); case 24: return sizeof(phx_outlier_clamp_summary);
    case 25: return sizeof(phx_tile_map); case 26: return sizeof(phx_tile_record); case 27: return sizeof(phx_tile_map_summary);
    case 28: return sizeof(phx_geometry_update); case 29: return sizeof(phx_geometry_summary);
    default: return 0;
  }
}

int phx_dev_set_adaptive(phx_device* d, const phx_adaptive* a) {
  if (!d) return fail(PHX_ERR_ARG, "set_adaptive: null device");
  if (d->running) return fail(PHX_ERR_STATE, "set_adaptive while a frame is running");
  if (!a) { d->adaptive_on = false; return PHX_OK; }
  if (const char* field = adaptive_invalid(*a)) return fail(PHX_ERR_ARG, outside_its_range("set_adaptive", field, "phx_adaptive"));
  d->adaptive = *a; d->adaptive_on = true;
  return PHX_OK;
}

// ---- tile queue: job::tiles_t (src/jobs/tiles.hpp:10-90) ------------------------------------------------
phx_tiles* phx_tiles_make(uint32_t width, uint32_t height, uint32_t ts, uint32_t rank, uint32_t world) {
  if (ts == 0 || world == 0 || rank >= world) { fail(PHX_ERR_ARG, "phx_tiles_make: bad arguments"); return nullptr; }
  uint32_t ht = width / ts, vt = height / ts;
  const uint32_t rh = height - ts * vt, rw = width - ts * ht;
  if (rh > 0) vt++;
  if (rw > 0) ht++;
  phx_tiles* q = new (std::nothrow) phx_tiles();
  if (!q) { fail(PHX_ERR_OOM, "host memory allocation failed"); return nullptr; }
  try {
  // owner of tile (x, y) = (x + s*y) mod world, s the smallest odd number >= 3 coprime to world: every rank's tiles run in
  // diagonals over the whole film.  (Plain "tile id mod world" degenerates into vertical stripes whenever the row length is
  // a multiple of world — 40 tiles per row at 1280 px — and the stripes under the light cost 8 % more rays than the mean.)
  uint32_t s = 3;
  for (;; s += 2) { uint32_t a = s, b = world; while (b) { const uint32_t t = a % b; a = b; b = t; } if (a == 1) break; }
  for (uint32_t y = 0; y < vt; ++y)
    for (uint32_t x = 0; x < ht; ++x) {
      uint32_t tw = ts, th = ts;
      if (y == vt - 1 && rh > 0) th = rh;
      if (x == ht - 1 && rw > 0) tw = rw;
      if ((x + s * y) % world == rank) q->tiles.push_back(phx_tile{x * ts, y * ts, tw, th});
    }
  } catch (...) { delete q; fail(PHX_ERR_OOM, "host memory allocation failed"); return nullptr; }
  return q;
}
phx_tiles* phx_tiles_make_list(const phx_tile* tiles, uint32_t count) {
  if (count && !tiles) { fail(PHX_ERR_ARG, "phx_tiles_make_list: null list"); return nullptr; }
  phx_tiles* q = new (std::nothrow) phx_tiles();
  if (!q) { fail(PHX_ERR_OOM, "host memory allocation failed"); return nullptr; }
  try { if (count) q->tiles.assign(tiles, tiles + count); } catch (...) { delete q; fail(PHX_ERR_OOM, "host memory allocation failed"); return nullptr; }
  return q;
}
int phx_tiles_next(void* tiles, phx_tile* out) {
  phx_tiles* q = (phx_tiles*)tiles;
  const uint32_t t = q->cursor++;
  if (t < q->tiles.size()) { *out = q->tiles[t]; return 1; }
  return 0;
}
uint32_t phx_tiles_count(const phx_tiles* q) { return q ? (uint32_t)q->tiles.size() : 0; }
void phx_tiles_reset(phx_tiles* q) { if (q) q->cursor = 0; }
void phx_tiles_free(phx_tiles* q) { delete q; }

int phx_dev_copy_bvh(phx_device* d, void* out, uint64_t capacity, uint64_t* bytes, float* grid6) {
  if (!d || !d->preprocessed) return fail(PHX_ERR_STATE, "copy_bvh before preprocess");
  if (!bytes) return fail(PHX_ERR_ARG, "copy_bvh: null size pointer");
  DeviceScope on(d->hip_device);
  if (!on.ok) return fail(PHX_ERR_DEVICE, "hipSetDevice failed");
  *bytes = d->bvh_bytes;
  if (grid6) for (int a = 0; a < 3; ++a) { grid6[a] = d->scene.grid.lo[a]; grid6[3 + a] = d->scene.grid.cell[a]; }
  const uint64_t n = std::min<uint64_t>(capacity, d->bvh_bytes);
  if (out && n) HIPCHK(hipMemcpy(out, d->d_pool.p, n, hipMemcpyDeviceToHost));
  return PHX_OK;
}

}  // extern "C"
