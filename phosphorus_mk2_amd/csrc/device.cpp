// device.cpp — host side of the gfx950 device: the C ABI of include/phx_xpu.h and its device object.
//
// Mirrors cpu_t (reference src/xpu/cpu.cpp:208-248): preprocess() flattens the scene and builds the accelerator (cpu.cpp:35-44), start() hands
// the frame to the device's driver thread, join() waits for it.  Here: the last error, discovery, the life cycle of a phx_device, the entry
// points of preprocess, update_geometry and set_camera, start / join / statistics, the adaptive setting, the tile queue and phx_dev_copy_bvh.
// What preprocess and update_geometry write to the device is scene_commit.cpp's (commit_scene, update_scene_geometry: the tree, the scene's
// tables, the traversal plan).  The rest of the ABI lives beside this file, over device_internal.h: frame_driver.cpp is the driver thread and the frame (it drains the shared
// tile queue, cpu.cpp:223-238, in batches of many tiles, each carried through the wavefront kernels of trace.hip, shade_lambert.hip,
// shade_general.hip, film_hooks.hip, and hands finished tiles to the film sink, cpu.cpp:201), stage_hooks.cpp the scene-reading stage hooks,
// film_calls.cpp the film calls no frame launches (the denoiser of denoise.hip, the guide pass of guides.hip, film accumulation of accumulate.hip).
// What needs no device: scene_flatten.cpp is the host-only half of preprocess, frame_plan.cpp that of the frame driver (the film's pixel layout,
// the pixel cap, the batch cutter, the pass schedule), denoise_check.cpp, guides_check.cpp and accumulate_check.cpp the argument checks of the film calls, over film_checks.h.
// There is no CPU rendering path in this library: without a gfx950 device every entry point fails.
#include "device_internal.h"
#include "film_checks.h"
#include "scene_flatten.h"

#include <atomic>
#include <cfloat>
#include <cstdio>
#include <cstring>

using namespace phx;

namespace phx {

thread_local std::string g_error;  // (device_internal.h)

int fail(int code, const std::string& msg) { g_error = msg; return code; }

}  // namespace phx

struct phx_tiles {
  std::vector<phx_tile> tiles;
  std::atomic<uint32_t> cursor{0};
};

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

// Three stages: the state checks, flatten_scene (scene_flatten.cpp: validation and everything derived on the host — a refusal leaves the
// device and its previous scene untouched), and commit_scene (scene_commit.cpp), which builds the tree and replaces the device's tables.
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
    if (const int rc = flatten_geometry(*s, d->opt, d->tables.geometry, fs, why)) return fail(rc, why);
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
  out->bvh_nodes = d->tables.bvh_nodes; out->bvh_bytes = d->tables.bvh_bytes; out->triangles = d->tables.num_triangles;
  out->preprocess_ms = d->preprocess_ms; out->bvh_build_ms = d->bvh_build_ms;
  out->trace_block = d->plan.block; out->trace_ntop = d->plan.ntop; out->trace_levels = d->plan.levels; out->trace_lds_levels = d->plan.lds_levels; out->trace_stack_packed = d->plan.packed;
  out->trace_waves_per_cu = (uint64_t)d->plan.wg_per_cu * (d->plan.block / 64u); out->bvh_depth = d->scene.stack_levels;
  out->paths_in_flight = d->paths_in_flight;
  out->bvh_cost_model = d->tables.bvh_cost_model; out->bvh_built_on_device = d->tables.bvh_built_on_device;
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
  *bytes = d->tables.bvh_bytes;
  if (grid6) for (int a = 0; a < 3; ++a) { grid6[a] = d->scene.grid.lo[a]; grid6[3 + a] = d->scene.grid.cell[a]; }
  const uint64_t n = std::min<uint64_t>(capacity, d->tables.bvh_bytes);
  if (out && n) HIPCHK(hipMemcpy(out, d->tables.d_pool.p, n, hipMemcpyDeviceToHost));
  return PHX_OK;
}

}  // extern "C"
