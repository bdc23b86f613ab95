// scene_commit.cpp — the two writers of the device's committed scene (device_internal.h: SceneTables, phx_device::scene): commit_scene, the
// last stage of phx_dev_preprocess, and update_scene_geometry, the device half of phx_dev_update_geometry.
//
// Both are sequences of the same steps, each stated once here:
//   the tree       build_checked_tree (build_tree, its timing, the depth refusal), then alloc_elem_tables (the tables sized by pool element)
//   the geometry   enqueue_geometry_tables: light tables, normals, shade records, UVs by pool element, the light triangles' remaps
//   the record     upload_tex_record: the DevTexScene through which the shade kernels find the images
//   the plan       plan_trace: trace_plan and the spill buffer
// What differs is the callers' own: preprocess uploads the appearance and lets buffers grow only (DevBuf); a rebuild releases what the new
// tree sizes differently, so that the device holds what a fresh preprocess holds; an update feeds its upload / device timers.
#include "device_internal.h"
#include "bvh_build.h"
#include "bvh_gpu.h"

#include <cstdio>
#include <cstring>

using namespace phx;

#ifndef PHX_TEST_HOOKS
#define PHX_TEST_HOOKS 0  /* 1 only in the twin library libphx_hip_hooks.so (fault injection for the tests); never in the product build */
#endif

namespace {

// PHX_BVH_AUTO: the device builder (bvh_gpu.hip) unless the scene is tiny.  Round 2 kept the host's binned SAH for scenes up to 2 M
// triangles because its trees traced 3-5 % faster on mesh-like scenes; with extended Morton codes (the size of a primitive as a
// fourth coordinate) the device trees are as fast or faster everywhere measured — soups -2 ... -7 % k_trace time, the showroom
// -3 % — and they are built in milliseconds (profiles/r03_z_emc_probe.log, r03_za_builder_ab.log).
// Fills d_pool, the tree's words of d->scene and of the statistics, and elem_of_prim: the pool index of every primitive's triangle record (the
// shade records and the normals table are laid out by it).  d_prim_material holds the scene's material words already.
int build_tree(phx_device* d, const FlatScene& fs, DevBuf<uint32_t>& elem_of_prim) {
  int rc;
  SceneTables& T = d->tables;
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
    if (!brc) brc = build_bvh8_gpu(d->stream, d_abc.p, T.d_prim_material.p, ntri, &g, msg, sizeof(msg), elem_of_prim.p);
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
    if ((rc = T.d_pool.upload(bvh.pool))) return rc;
    if ((rc = elem_of_prim.upload(bvh.elem_of_prim))) return rc;
    sc.stack_levels = bvh.depth; sc.num_elems = (uint32_t)bvh.pool.size(); sc.grid = bvh.grid;
    T.bvh_nodes = bvh.num_nodes; T.bvh_cost_model = bvh.cost; T.bvh_built_on_device = 0;
  } else {
    T.d_pool.adopt(g.pool, g.num_elems);
    sc.stack_levels = g.depth; sc.num_elems = g.num_elems; sc.grid = g.grid;
    T.bvh_nodes = g.num_nodes; T.bvh_cost_model = g.cost; T.bvh_built_on_device = 1;
  }
  sc.pool = reinterpret_cast<const uint32_t*>(T.d_pool.p);
  sc.tris = reinterpret_cast<const TriRec*>(T.d_pool.p);
  T.bvh_bytes = (uint64_t)sc.num_elems * sizeof(PoolElem);
  return PHX_OK;
}

// The tree step, first half: build_tree, what it took (phx_stats::bvh_build_ms) and the refusal of a tree the traversal cannot walk.
int build_checked_tree(phx_device* d, const FlatScene& fs, DevBuf<uint32_t>& elem_of_prim) {
  const auto t0 = Clock::now();
  if (const int rc = build_tree(d, fs, elem_of_prim)) return rc;
  d->bvh_build_ms = ms_between(t0, Clock::now());
  // k_trace / k_trace_rays keep one pending sibling group per level and lane in LDS (bvh8.h: PHX_MAX_BVH_DEPTH)
  if (d->scene.stack_levels > PHX_MAX_BVH_DEPTH)
    return fail(PHX_ERR_ARG, "tree too deep: " + std::to_string(d->scene.stack_levels) + " levels, the traversal stack in LDS holds " + std::to_string(PHX_MAX_BVH_DEPTH));
  return PHX_OK;
}

// The tree step, second half: the tables sized by POOL ELEMENT (the index a hit record carries), each held only by a scene that reads it.  What
// shading reads of a hit triangle, 16 bytes: geometric normal + material word; the vertex normals, so that the shade kernels request them
// with the triangle record and not after it; the corner UVs likewise (textured lobes, masks and emitter images).  Grow-only, as DevBuf is:
// a rebuild releases what its new tree sizes differently before it comes here.
int alloc_elem_tables(phx_device* d, const FlatScene& fs) {
  int rc;
  SceneTables& T = d->tables;
  const size_t elems = d->scene.num_elems;
  if ((rc = T.d_elem_shade.alloc(elems))) return rc;
  if (fs.any_smooth) { if ((rc = T.d_elem_normals.alloc(9 * elems))) return rc; } else T.d_elem_normals.release();
  if (d->scene.any_tex & SC_TEX_LOBES) { if ((rc = T.d_elem_uv.alloc(3 * elems))) return rc; } else T.d_elem_uv.release();
  return PHX_OK;
}

// The uploads and the device work of a geometry update (update_geometry_ms[1], [2]: host clock).  Preprocess reports neither and hands the
// steps no timers.
struct UpdateTimers { double upload_ms = 0.0, device_ms = 0.0; };
template <typename F>
int timed(UpdateTimers* t, double UpdateTimers::*which, F&& body) {
  if (!t) return body();
  const auto t0 = Clock::now();
  const int rc = body();
  t->*which += ms_between(t0, Clock::now());
  return rc;
}

// What the geometry step reads in primitive order, on the device.  The step only enqueues its kernels: the caller holds these until it has
// synchronised the stream.
struct PrimOrderTables {
  DevBuf<uint32_t> elem_of_prim;  // the tree's: the pool index of every primitive's triangle record (build_tree, refit_bvh8_gpu)
  DevBuf<float2> uv;              // 3 corner UVs per primitive, from the caller when the corner UVs are to be laid out anew; else empty
  DevBuf<float> normals;          // the step's own upload (a scene with a smooth face)
  void release() { elem_of_prim.release(); uv.release(); normals.release(); }
};

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

// The geometry step: everything the device derives from the triangles' positions and normals and the tree's order (d->scene's tree words,
// po.elem_of_prim; alloc_elem_tables has sized the tables).  Uploads the light tables and the normals, then enqueues on d->stream: the shade
// records, the normals by pool element, the smooth light triangles' `prim` as a pool index (shading_normal on the light's face,
// spt.hpp:212-255), the corner UVs by pool element and — emitter images: every light triangle reaches its corner UVs by pool element — the
// flat ones' too.  Both remaps follow the upload of light_tris, the flat one the smooth one.  Sets the scene's pointers to what it wrote.
int enqueue_geometry_tables(phx_device* d, FlatScene& fs, PrimOrderTables& po, UpdateTimers* t) {
  SceneTables& T = d->tables;
  DevScene& sc = d->scene;
  const uint32_t ntri = (uint32_t)fs.prim_material.size();
  append_light_tables(sc, fs);
  int rc = timed(t, &UpdateTimers::upload_ms, [&] {
    int r = T.d_lights.upload(fs.lights);
    if (!r) r = T.d_light_tris.upload(fs.light_tris);
    if (!r && fs.any_smooth) r = po.normals.upload(fs.prim_normals);
    return r;
  });
  if (rc) return rc;
  rc = timed(t, &UpdateTimers::device_ms, [&]() -> int {
    launch_build_shade_recs(d->stream, sc.tris, po.elem_of_prim.p, T.d_elem_shade.p, ntri);
    if (fs.any_smooth) {
      launch_permute_normals(d->stream, po.normals.p, po.elem_of_prim.p, T.d_elem_normals.p, ntri);
      launch_remap_light_tris(d->stream, T.d_light_tris.p, (uint32_t)fs.light_tris.size(), po.elem_of_prim.p);
    }
    if (sc.any_tex & SC_TEX_LOBES) {
      if (po.uv.p) launch_permute_uvs(d->stream, po.uv.p, po.elem_of_prim.p, T.d_elem_uv.p, ntri);
      if (T.geometry.any_emit_tex) launch_remap_flat_light_tris(d->stream, T.d_light_tris.p, (uint32_t)fs.light_tris.size(), po.elem_of_prim.p);
    }
    HIPCHK(hipGetLastError());
    return PHX_OK;
  });
  if (rc) return rc;
  sc.elem_normals = fs.any_smooth ? T.d_elem_normals.p : nullptr;
  sc.elem_shade = T.d_elem_shade.p;
  sc.lights = T.d_lights.p; sc.light_tris = T.d_light_tris.p;
  return PHX_OK;
}

// The record step: the one record through which the shade kernels find the images, made from the device's buffers as they are now (a scene
// with SC_TEX_ANY only).  env_p: the environment's interval of the selection table (FlatScene::env_p), which moves with the scene's bounds.
int upload_tex_record(phx_device* d, float env_p) {
  SceneTables& T = d->tables;
  const bool any_tex = (d->scene.any_tex & SC_TEX_LOBES) != 0, emit_tex = T.geometry.any_emit_tex;
  return T.d_tex_scene.upload(std::vector<DevTexScene>{DevTexScene{
      any_tex ? T.d_elem_uv.p : nullptr, T.d_textures.p, T.d_texels.p, any_tex ? T.d_lobe_tex.p : nullptr, T.env_tex ? T.env_tex - 1u : 0u, T.env_mapping,
      emit_tex ? 1u : 0u, env_p, emit_tex ? T.d_mat_emit_tex.p : nullptr, (d->scene.any_tex & SC_LIGHTS_ENV) ? T.d_env_cdf.p : nullptr}});
}

// The plan step: how k_trace runs on the tree in d->scene, and the stack levels below the ones it keeps in LDS (trace.hip: trace_plan).
// The scene's spill words are zero on entry.  Grow-only, as alloc_elem_tables.
size_t spill_entries(const TracePlan& p) { return p.spill_threads ? (size_t)p.spill_threads * (p.levels - p.lds_levels) : 0; }
int plan_trace(phx_device* d) {
  d->plan = trace_plan(d->scene);
  if (const size_t spill = spill_entries(d->plan)) {
    if (const int rc = d->tables.d_spill.alloc(spill)) return rc;
    d->scene.stack_spill = d->tables.d_spill.p; d->scene.spill_stride = d->plan.spill_threads;
  }
  d->budget_bytes = 0;  // the next frame asks the device again how much memory is free
  return PHX_OK;
}

int update_failed(int brc, const char* msg) {
  return fail(brc == (int)BVH_GPU_RECOVERABLE ? PHX_ERR_OOM : PHX_ERR_DEVICE, std::string("update_geometry: ") + msg);
}

}  // namespace

namespace phx {

// From its first line to its last the device has NO scene (preprocessed == false): a failure on the way — the device builder's fatal error,
// a tree too deep, a hipMalloc that fails — leaves buffers and facts of the old and the new scene mixed, and start / the stage hooks answer
// PHX_ERR_STATE until a preprocess succeeds.
int commit_scene(phx_device* d, FlatScene& fs) {
  int rc;
  d->preprocessed = false;
  SceneTables& T = d->tables;
  DevScene& sc = d->scene = fs.scene;
  const uint32_t ntri = (uint32_t)fs.prim_material.size();
  const bool any_tex = (sc.any_tex & SC_TEX_LOBES) != 0, any_image = (sc.any_tex & SC_TEX_ANY) != 0;
  // the host facts first: the steps read the scene's classes from them, as they do in an update
  T.num_materials = (uint32_t)fs.materials.size();
  T.mat_masked = std::move(fs.mat_masked);
  T.num_textures = any_image ? (uint32_t)fs.textures.size() : 0;
  T.env_tex = fs.env_tex; T.env_mapping = fs.env_mapping;
  for (int c = 0; c < 3; ++c) T.env_e[c] = fs.env_e[c];
  T.num_triangles = ntri;
  T.geometry = std::move(fs.fingerprint);
  // Who reads (u, v) of a hit: a smooth face's normal, the corner UVs' interpolation (lobe images, masks, emitter images: SC_TEX_LOBES) and a
  // per-hit material — the classes flatten_scene made for launch_shade.  PHX_HIT_UV=1 (tests only) carries the stream on a scene that does not.
  {
    const char* force = std::getenv("PHX_HIT_UV");
    d->hit_uv = fs.any_smooth || any_tex || sc.any_per_hit != 0 || (force && std::atoi(force) != 0);
  }
  if ((rc = T.d_prim_material.upload(fs.prim_material))) return rc;
  PrimOrderTables po;
  if ((rc = build_checked_tree(d, fs, po.elem_of_prim)) || (rc = alloc_elem_tables(d, fs))) return rc;
  // The geometry's kernels go first and run under the uploads of the appearance below; one synchronise, at the end, covers them.
  if (any_tex && (rc = po.uv.upload(fs.prim_uv))) return rc;
  if ((rc = enqueue_geometry_tables(d, fs, po, nullptr))) return rc;
  // the appearance (preprocess only: an update reads no material, lobe, texel or environment image again)
  if ((rc = T.d_materials.upload(fs.materials))) return rc;
  if (any_tex) { if ((rc = T.d_lobe_tex.upload(fs.lobe_tex))) return rc; } else T.d_lobe_tex.release();
  if (T.geometry.any_emit_tex) { if ((rc = T.d_mat_emit_tex.upload(fs.mat_emit_tex))) return rc; } else T.d_mat_emit_tex.release();
  if (sc.any_tex & SC_LIGHTS_ENV) { if ((rc = T.d_env_cdf.upload(fs.env_cdf))) return rc; } else T.d_env_cdf.release();
  if (any_image) {  // the texture table and the texels, and the record that points at them
    if ((rc = T.d_textures.upload(fs.textures)) || (rc = T.d_texels.upload(fs.texels)) || (rc = upload_tex_record(d, fs.env_p))) return rc;
  } else {
    T.d_textures.release(); T.d_texels.release(); T.d_tex_scene.release();
  }
  if (sc.diffuse_only == 2 && (rc = T.d_mat_lite.upload(fs.mat_lite))) return rc;
  HIPCHK(hipStreamSynchronize(d->stream));  // `po` goes out of scope below
  sc.materials = T.d_materials.p;
  sc.mat_lite = sc.diffuse_only == 2 ? T.d_mat_lite.p : nullptr;
  sc.tex = any_image ? T.d_tex_scene.p : nullptr;
  {
    hipDeviceProp_t prop; HIPCHK(hipGetDeviceProperties(&prop, d->hip_device));
    sc.num_cus = (uint32_t)prop.multiProcessorCount;
  }
  if ((rc = plan_trace(d))) return rc;
  d->preprocessed = true;
  return PHX_OK;
}

// Refit: the pool is refitted in place (bvh_refit.hip).  Rebuild: build_tree makes a new one, the corner UVs are carried over by the old and
// the new elem_of_prim, the traversal plan and the spill buffer are recomputed; everything sized by the tree is released where the new
// tree's size differs, not kept at the larger of the two, so that after a rebuild the device holds what a fresh preprocess of the moved
// scene holds.  Then the geometry step, as in commit_scene.  As there, the device has no scene from the first device write to the last line.
// Timers: every stretch of device work ends in a synchronise; under a rebuild the triangles go up inside build_tree, so their upload is
// counted with the device's work.
int update_scene_geometry(phx_device* d, FlatScene& fs, uint32_t mode, phx_geometry_summary* sum, double* ms) {
  int rc;
  SceneTables& T = d->tables;
  DevScene& sc = d->scene;
  const uint32_t ntri = (uint32_t)fs.prim_material.size();
  const bool any_tex = (sc.any_tex & SC_TEX_LOBES) != 0, any_image = (sc.any_tex & SC_TEX_ANY) != 0, rebuild = mode == PHX_UPDATE_REBUILD;
  UpdateTimers t;
  char msg[256] = {0};
  DevBuf<float> d_abc; PrimOrderTables po;
  if (!rebuild) {
    if ((rc = timed(&t, &UpdateTimers::upload_ms, [&] { return d_abc.upload(fs.abc); })) || (rc = po.elem_of_prim.alloc(ntri))) return rc;
    d->preprocessed = false;
    GpuRefit r{};
    const int brc = timed(&t, &UpdateTimers::device_ms, [&] { return refit_bvh8_gpu(d->stream, T.d_pool.p, sc.num_elems, d_abc.p, ntri, po.elem_of_prim.p, &r, msg, sizeof(msg)); });
    if (brc) return update_failed(brc, msg);
    sc.grid = r.grid;
  } else {
    if (any_tex) {  // the corner UVs in primitive order, read back through the old tree's elem_of_prim: no UV value is read from the scene again
      DevBuf<uint32_t> d_old;
      if ((rc = d_old.alloc(ntri)) || (rc = po.uv.alloc(3 * (size_t)ntri))) return rc;
      const int brc = timed(&t, &UpdateTimers::device_ms, [&] {
        const int e = pool_elem_of_prim_gpu(d->stream, T.d_pool.p, sc.num_elems, ntri, d_old.p, msg, sizeof(msg));
        if (e) return e;
        launch_gather_rows(d->stream, reinterpret_cast<const float*>(T.d_elem_uv.p), d_old.p, reinterpret_cast<float*>(po.uv.p), ntri, 6, sc.num_elems);
        return hipStreamSynchronize(d->stream) == hipSuccess ? 0 : 1;
      });
      if (brc) return update_failed(brc, msg);
    }
    d->preprocessed = false;
    const uint32_t elems_before = sc.num_elems;
    T.d_pool.release();  // read for the last time above
    if ((rc = build_checked_tree(d, fs, po.elem_of_prim))) return rc;
    t.device_ms += d->bvh_build_ms;
    if (sc.num_elems != elems_before) { T.d_elem_shade.release(); T.d_elem_normals.release(); T.d_elem_uv.release(); }
    if ((rc = alloc_elem_tables(d, fs))) return rc;
  }
  if ((rc = enqueue_geometry_tables(d, fs, po, &t))) return rc;
  if ((rc = timed(&t, &UpdateTimers::device_ms, [&]() -> int { HIPCHK(hipStreamSynchronize(d->stream)); return PHX_OK; }))) return rc;
  if (any_image && ((sc.any_tex & SC_LIGHTS_ENV) || (rebuild && any_tex))) {  // the environment's interval moved with the bounds; a rebuild may have moved elem_uv
    if ((rc = timed(&t, &UpdateTimers::upload_ms, [&] { return upload_tex_record(d, fs.env_p); }))) return rc;
  }
  if (rebuild) {
    sc.stack_spill = nullptr; sc.spill_stride = 0;
    if (spill_entries(trace_plan(sc)) != T.d_spill.n) T.d_spill.release();
    if ((rc = plan_trace(d))) return rc;
  }
  if (sum) {
    *sum = phx_geometry_summary{mode, ntri, (uint32_t)T.bvh_nodes, sc.stack_levels, sc.num_lights, (uint32_t)fs.light_tris.size(),
                                {fs.bounds[0], fs.bounds[1], fs.bounds[2], fs.bounds[3], fs.bounds[4], fs.bounds[5]}, tri_box_inflation(fs.bounds, fs.bounds + 3)};
  }
  // the call's own device buffers go here, inside the device's timer, not when the function returns
  (void)timed(&t, &UpdateTimers::device_ms, [&] { d_abc.release(); po.release(); return 0; });
  ms[1] = t.upload_ms; ms[2] = t.device_ms;
  d->preprocessed = true;
  return PHX_OK;
}

}  // namespace phx
