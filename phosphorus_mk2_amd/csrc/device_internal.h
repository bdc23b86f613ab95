// device_internal.h — what the host units of the C ABI share: device.cpp (the device object's life cycle, the entry points), scene_commit.cpp
// (what preprocess and a geometry update write to the device), frame_driver.cpp (the frame), stage_hooks.cpp (the scene-reading stage hooks)
// and film_calls.cpp (the film calls no frame launches).
//
// The last error, the HIP wrappers (HIPCHK, DeviceScope, DevBuf, PinnedBuf), SceneTables, guarded(), the clock, Staging, PathQueues and struct
// phx_device itself.  Not installed and no part of the ABI: include/phx_xpu.h knows phx_device by name only.
#pragma once
#include "../../include/phx_xpu.h"
#include "frame_plan.h"
#include "kernels.h"
#include "scene_flatten.h"

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <deque>
#include <mutex>
#include <new>
#include <optional>
#include <string>
#include <thread>
#include <vector>

namespace phx {

// Errors: every thread has its own last-error string; a driver thread's error is also kept with its device (phx_device::
// frame_error) and handed to the thread that calls phx_dev_join, so two devices rendering at once never share a buffer.
// (One string per thread for ALL units — defined in device.cpp, where phx_last_error reads it.)
extern thread_local std::string g_error;

int fail(int code, const std::string& msg);

#define HIPCHK(expr)                                                                                     \
  do {                                                                                                   \
    hipError_t e_ = (expr);                                                                              \
    if (e_ != hipSuccess) return phx::fail(PHX_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

// Entry points run on the CALLER's thread: they switch to their device and put the caller's current device back on the way out,
// so a host that mixes several phx_devices with its own HIP / torch allocations never finds itself on another GPU.
struct DeviceScope {
  int prev = -1; bool ok = false;
  explicit DeviceScope(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) { prev = -1; (void)hipGetLastError(); }
    ok = hipSetDevice(dev) == hipSuccess;
  }
  ~DeviceScope() { if (prev >= 0) (void)hipSetDevice(prev); }
};

template <typename T>
struct DevBuf {
  T* p = nullptr; size_t n = 0;
  int alloc(size_t count) {
    if (count <= n && p) return PHX_OK;
    release();
    hipError_t e = hipMalloc((void**)&p, std::max<size_t>(count, 1) * sizeof(T));
    if (e != hipSuccess) { p = nullptr; return fail(PHX_ERR_OOM, std::string("hipMalloc: ") + hipGetErrorString(e)); }
    n = count;
    return PHX_OK;
  }
  int upload(const std::vector<T>& h) {
    int rc = alloc(h.size()); if (rc) return rc;
    if (!h.empty()) HIPCHK(hipMemcpy(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    return PHX_OK;
  }
  void adopt(T* ptr, size_t count) { release(); p = ptr; n = count; }  // take ownership of a hipMalloc'd array
  void release() { if (p) { (void)hipFree(p); p = nullptr; n = 0; } }
  size_t bytes() const { return p ? std::max<size_t>(n, 1) * sizeof(T) : 0; }
  ~DevBuf() { release(); }
};
// Pinned host memory (flags: hipHostMalloc's).  Grow-only, as DevBuf: a larger request frees and allocates anew, a smaller one is served in place.
template <typename T>
struct PinnedBuf {
  T* p = nullptr; size_t n = 0;
  int alloc(size_t count, unsigned flags) {
    if (count <= n && p) return PHX_OK;
    release();
    hipError_t e = hipHostMalloc((void**)&p, std::max<size_t>(count, 1) * sizeof(T), flags);
    if (e != hipSuccess) { p = nullptr; return fail(PHX_ERR_DEVICE, std::string("hipHostMalloc: ") + hipGetErrorString(e)); }
    n = count;
    return PHX_OK;
  }
  void release() { if (p) { (void)hipHostFree(p); p = nullptr; n = 0; } }
  ~PinnedBuf() { release(); }
};

// The committed scene as the device holds it: its buffers, and the host facts that describe them.  scene_commit.cpp is their only writer
// (commit_scene, update_scene_geometry); the stage hooks and phx_dev_copy_bvh read them.
struct SceneTables {
  DevBuf<PoolElem> d_pool; DevBuf<uint32_t> d_prim_material; DevBuf<float> d_elem_normals; DevBuf<float4> d_elem_shade; DevBuf<uint2> d_spill;
  DevBuf<DevMaterial> d_materials; DevBuf<DevMatLite> d_mat_lite; DevBuf<DevLight> d_lights; DevBuf<DevLightTri> d_light_tris;
  // image textures: held only while the preprocessed scene has a textured lobe
  DevBuf<float2> d_elem_uv; DevBuf<DevTexture> d_textures; DevBuf<float4> d_texels; DevBuf<uint32_t> d_lobe_tex; DevBuf<DevTexScene> d_tex_scene;
  DevBuf<uint32_t> d_mat_emit_tex;  // per material: the image on its emission + 1 (scenes with emitter images only)
  DevBuf<float> d_env_cdf;          // PHX_LIGHT_INCLUDE_ENVIRONMENT: the environment's direction tables (FlatScene::env_cdf)
  uint32_t num_materials = 0, num_textures = 0;
  std::vector<uint8_t> mat_masked;  // per material: some lobe's factor is an image mask (the untextured KAT hooks refuse those)
  uint32_t env_tex = 0, env_mapping = 0; float env_e[3] = {0.0f, 0.0f, 0.0f};  // the environment's image (texture + 1, 0 = none), mapping and emission
  GeometryFingerprint geometry;  // of the committed scene (host memory): what phx_dev_update_geometry accepts a moved scene against
  // the tree's statistics (build_tree)
  uint64_t bvh_nodes = 0, bvh_bytes = 0, num_triangles = 0;
  double bvh_cost_model = 0; uint32_t bvh_built_on_device = 0;
  uint64_t bytes() const {  // every buffer above: a new one is added here, beside its declaration
    return d_pool.bytes() + d_prim_material.bytes() + d_elem_normals.bytes() + d_elem_shade.bytes() + d_spill.bytes() + d_materials.bytes() + d_mat_lite.bytes() +
           d_lights.bytes() + d_light_tris.bytes() + d_elem_uv.bytes() + d_textures.bytes() + d_texels.bytes() + d_lobe_tex.bytes() + d_tex_scene.bytes() +
           d_mat_emit_tex.bytes() + d_env_cdf.bytes();
  }
};

// No C++ exception may cross the C ABI (the reference's own std::runtime_error cases become status codes): every entry
// point that allocates or spawns runs its body through guarded().
template <typename F>
int guarded(F&& body) {
  try { return body(); }
  catch (const std::bad_alloc&) { return fail(PHX_ERR_OOM, "host memory allocation failed"); }
  catch (const std::exception& e) { return fail(PHX_ERR_DEVICE, std::string("unexpected exception: ") + e.what()); }
  catch (...) { return fail(PHX_ERR_DEVICE, "unexpected exception"); }
}

using Clock = std::chrono::steady_clock;
inline double ms_between(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); }

// Queues + state of the paths in flight, 16 bytes per path each (kernels.h: PassBuffers): ray queues 2 x 32, path state travelling with them
// 2 x 16, shadow queue 48, radiance 16, and the primary normal 16 when the frame has a normals channel; the hit record is two streams of 8:
// (t, triangle) always, the barycentrics only for a scene that reads them (`uv`: phx_device::hit_uv).
struct PathQueues {
  enum { RO, RD, QS, RO1, RD1, QS1, SO, SD, SC, PR, PN, COUNT };  // PN last: allocated only for a frame with a normals channel
  DevBuf<float4> q[COUNT];
  DevBuf<uint2> hit_tt; DevBuf<float2> hit_uv;
  // (with both hit streams: what a scene without barycentrics saves is not handed to more paths in flight, so a batch is cut the same way either way)
  static constexpr size_t bytes_per_path(bool normals) { return (COUNT - (normals ? 0 : 1)) * sizeof(float4) + sizeof(uint2) + sizeof(float2); }
  int alloc(size_t npaths, bool normals, bool uv) {
    for (int i = 0; i < COUNT - (normals ? 0 : 1); ++i) if (const int rc = q[i].alloc(npaths)) return rc;
    if (const int rc = hit_tt.alloc(npaths)) return rc;
    if (!uv) { hit_uv.release(); return PHX_OK; }  // a scene switch: the stream goes with the scene that read it
    return hit_uv.alloc(npaths);
  }
  void release() { for (auto& b : q) b.release(); hit_tt.release(); hit_uv.release(); }
  size_t bytes() const { size_t n = hit_tt.bytes() + hit_uv.bytes(); for (auto& b : q) n += b.bytes(); return n; }
  size_t capacity() const { return hit_tt.n; }  // paths the queues hold
  void fill(PassBuffers& B, bool normals, bool uv) const {
    for (int k = 0; k < 2; ++k) { B.ro[k] = q[RO + 3 * k].p; B.rd[k] = q[RD + 3 * k].p; B.qs[k] = q[QS + 3 * k].p; }
    B.hit_tt = hit_tt.p; B.hit_uv = uv ? hit_uv.p : nullptr;
    B.so = q[SO].p; B.sd = q[SD].p; B.sc = q[SC].p; B.pr = q[PR].p; B.pn = normals ? q[PN].p : nullptr;
  }
};
static_assert(PathQueues::bytes_per_path(false) == queue_bytes_per_path(false) && PathQueues::bytes_per_path(true) == queue_bytes_per_path(true),
              "what path_budget divides the device's memory by (frame_plan.h: FilmLayout::path_bytes)");

// frame_driver.cpp: what run_frame and its batches share with the film calls
// what the selection behind a round that ended at n of spp samples takes from the setting (phx_adaptive: q, g, k), in binary64
void adaptive_args(const phx_adaptive& a, uint32_t n, uint32_t spp, AdaptiveArgs& A);
// the film jitter of sample index 0 .. spp - 1, shared by all pixels (run_frame and phx_dev_render_guides read the same table)
std::vector<float2> jitter_table(uint64_t seed, uint32_t spp);

}  // namespace phx

struct phx_device {
  phx_options opt{};
  int hip_device = 0;
  hipStream_t stream = nullptr;
  bool preprocessed = false;

  phx::SceneTables tables;  // the committed scene's buffers and the host facts about them (scene_commit.cpp writes them)
  phx::DevScene scene{};
  double update_geometry_ms[4] = {};  // the last phx_dev_update_geometry: host flatten, uploads, device work, call
  double preprocess_ms = 0, bvh_build_ms = 0;

  // pass buffers
  phx::PathQueues queues;
  phx::DevBuf<uint32_t> counters; phx::DevBuf<phx::DevStats> dstats; phx::DevBuf<uint32_t> pix_xy; phx::DevBuf<float2> jitter; phx::DevBuf<float> acc;
  uint64_t jitter_seed = 0; uint32_t jitter_spp = 0;  // what the jitter table on the device was made for
  phx::PinnedBuf<float> h_acc;      // pinned staging for add_tile
  phx::PinnedBuf<uint32_t> h_qlen;  // pinned, device-visible: queue lengths published by k_trace, one word per (pass, step) of a batch (enqueue_batch)
  std::vector<phx_tile> pix_xy_tiles;          // the tiles pix_xy currently describes
  // adaptive sampling (phx_dev_set_adaptive), held only by a device that rendered a frame with it: the working copies of acc and pix_xy that a
  // pass over the pixels still active reads (working row w = row sel_idx[.][w] of the batch), the two lists a selection reads and writes
  // by turns, a word per workgroup of the selection, and the pinned word through which the host reads how many pixels go on
  phx::DevBuf<float> w_acc; phx::DevBuf<uint32_t> w_xy, sel_idx[2], sel_blocks;
  phx::PinnedBuf<uint32_t> h_sel;
  phx_adaptive adaptive{}; bool adaptive_on = false;
  // the milliseconds of each film call's last run (film_calls.cpp: FilmCall writes them, a phx_dev_*_times getter copies its array out whole,
  // times_of): kernel and call; the display's histogram + exposure, encode and call; the denoiser's pack, iterations 1 .. 8, unpack and call
  double guides_ms[2] = {}, accumulate_ms[2] = {}, reproject_ms[2] = {}, outlier_clamp_ms[2] = {}, tile_map_ms[2] = {};
  double display_ms[3] = {};
  double denoise_ms[11] = {};

  // frame
  phx_frame frame{};
  phx::FilmLayout layout;  // of `frame` (run_frame)
  // ONE driver thread per device, kept across frames (cpu_t spawns its workers per frame, src/xpu/cpu.cpp:223-238; here a frame of a rank
  // of eight lasts 9 ms and a thread start costs 50-70 us of it): phx_dev_start hands it the frame, phx_dev_join waits for `frame_done`
  std::thread driver;
  std::mutex mu; std::condition_variable cv;
  bool frame_pending = false, frame_done = false, quit = false;
  bool running = false;
  int frame_status = PHX_OK;
  std::string frame_error;  // g_error of the driver thread, copied when its frame ends
  phx_stats stats{};
  phx::TracePlan plan{};
  uint64_t paths_in_flight = 0;
  // the committed scene reads the barycentrics of a hit (scene_commit.cpp: commit_scene): the passes carry PassBuffers::hit_uv and the trace kernels run as UV = true
  bool hit_uv = false;
  enum class Launch { Trace, Primary, Shade, Pass /* begin-pass, film */ };
  struct Timed { size_t begin, end; Launch kind; };  // (event before, event behind, what ran between them)
  // The launches of a batch and the HIP events between them.  (Round 5 captured a batch's launches — memset, [begin-pass, camera rays,
  // shade, (trace, shade) x (depth - 1), trace, film] per pass, film scatter — as ONE hipGraph, cached by a hash of the kernel arguments:
  // rank 0 of 8 of the bench frame 9.12-9.27 ms with direct launches and events, 9.08-9.37 without events, 9.14-9.16 as a graph — nothing,
  // the fixed costs of a short frame are k_trace's drain tails on the GPU, not the host's enqueue; and an event recorded by a graph's
  // event-record node cannot be read with hipEventElapsedTime on ROCm 7.2.  profiles/r05_b_graph_rank_share.log, r05_b_graph.patch.)
  struct BatchLaunches {
    std::vector<hipEvent_t> events; size_t events_used = 0;
    std::vector<Timed> timed;
  };
  BatchLaunches direct;
  bool kernel_timing = true;        // per-kernel HIP events (phx_stats::closest_ms ...); PHX_KERNEL_TIMING=0 launches without them (probe)
  phx::Clock::time_point t_start, t_enq, t_sync;  // host timing probe (PHX_HOST_TIMING)

  ~phx_device() {
    {
      std::lock_guard<std::mutex> lk(mu);
      quit = true;
    }
    cv.notify_all();
    if (driver.joinable()) driver.join();
    for (auto e : direct.events) (void)hipEventDestroy(e);
    if (stream) (void)hipStreamDestroy(stream);
  }

  static int next_event(BatchLaunches& g, hipEvent_t* out) {
    if (g.events_used == g.events.size()) {
      hipEvent_t e; HIPCHK(hipEventCreate(&e));
      g.events.push_back(e);
    }
    *out = g.events[g.events_used++];
    return PHX_OK;
  }
  // HBM held by this device object (phx_stats::device_bytes)
  uint64_t device_bytes() const {
    return tables.bytes() + queues.bytes() + counters.bytes() + dstats.bytes() + pix_xy.bytes() + jitter.bytes() + acc.bytes() +
           w_acc.bytes() + w_xy.bytes() + sel_idx[0].bytes() + sel_idx[1].bytes() + sel_blocks.bytes();
  }
  // paths in flight this device may carry: up to 512 M (about 95 GB of queues + state: sized for 288 GB of HBM), but never more than 60 % of
  // what the device has free right now plus what this object already holds for queues (another device object, torch or RCCL may share the GPU)
  mutable uint64_t budget_bytes = 0;  // hipMemGetInfo costs ~0.1 ms a call: asked once per preprocess, not twice per frame
  uint64_t path_budget(size_t path_bytes) const {
    static const uint64_t cap_m = [] { const char* v = std::getenv("PHX_PATH_BUDGET_M"); const long x = v ? std::atol(v) : 0; return x >= 1 && x <= 1536 ? (uint64_t)x : 512ull; }();  // knob: millions of paths (128 / 256 / 512: config 4 on one GPU 6 987 / 7 182 / 7 314 Mrays/s, profiles/r04_x_budget.log)
    if (!budget_bytes) {
      budget_bytes = ~0ull;
      size_t free_b = 0, total_b = 0;
      if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) budget_bytes = (uint64_t)((double)(free_b + queues.bytes()) * 0.6);
    }
    return std::min<uint64_t>(cap_m << 20, budget_bytes / path_bytes);
  }
  void driver_loop();  // frame_driver.cpp, as run_frame, enqueue_batch and render_batch
  int run_frame();
  const phx_adaptive* adaptive_setting() const { return adaptive_on ? &adaptive : nullptr; }
  // the passes of a batch of P pixels under today's budget (frame_plan.h: plan_passes; with samples_in_flight set the device is not asked)
  uint32_t plan_batch(uint32_t P, uint32_t limit, std::vector<phx::Pass>& passes) const {
    return phx::plan_passes(P, opt.samples_per_pixel, opt.samples_in_flight, opt.samples_in_flight ? 0 : path_budget(layout.path_bytes), adaptive_setting(), limit, passes);
  }
  int enqueue_batch(BatchLaunches& g, const phx::PassBuffers& B0, uint32_t P, const std::vector<phx::Pass>& passes);
  int render_batch(const std::vector<phx_tile>& tiles);
};

namespace phx {

// scene_commit.cpp: the two writers of the committed scene.  Each runs on its device (DeviceScope) with no frame running, and from its first
// device write to its last line the device has NO scene (preprocessed == false).
// Replaces the device's scene by `fs` (flatten_scene's).
int commit_scene(phx_device* d, FlatScene& fs);
// Brings the device's scene to the moved geometry `fs` (flatten_geometry's, accepted against d->tables.geometry); mode: PHX_UPDATE_REFIT /
// PHX_UPDATE_REBUILD.  ms[1], ms[2]: the call's uploads and its device work.
int update_scene_geometry(phx_device* d, FlatScene& fs, uint32_t mode, phx_geometry_summary* sum, double* ms);

// Device copies of a stage hook's arrays.  in() uploads, out() allocates and remembers where the result goes, run() launches, waits and copies
// back.  The first array enters the hook's device (after the hook's own argument checks, as ever), and the caller's device comes back when the
// hook returns.  The first failure sticks (rc), and run() returns it without launching.
// (Here because two units stage arrays this way: the stage hooks, and phx_dev_film_moments and phx_dev_adaptive_select in film_calls.cpp.)
struct Staging {
  phx_device* d; int rc = PHX_OK;
  std::optional<DeviceScope> on;
  std::deque<DevBuf<uint32_t>> bufs;
  struct Back { void* host; const void* dev; size_t bytes; };
  std::vector<Back> back;
  template <typename T> T* out(T* host, size_t n) {  // host == nullptr: nothing to copy back
    static_assert(sizeof(T) % 4 == 0, "arrays of 32-bit words");
    if (!rc && !on && !on.emplace(d->hip_device).ok) rc = fail(PHX_ERR_DEVICE, "hipSetDevice failed");
    if (rc) return nullptr;
    bufs.emplace_back();
    if ((rc = bufs.back().alloc(n * (sizeof(T) / 4)))) return nullptr;
    if (host) back.push_back({host, bufs.back().p, n * sizeof(T)});
    return reinterpret_cast<T*>(bufs.back().p);
  }
  template <typename T> const T* in(const T* src, size_t n) {
    T* p = out<T>(nullptr, n);
    const hipError_t e = p ? hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice) : hipSuccess;
    if (e != hipSuccess) rc = fail(PHX_ERR_DEVICE, std::string("hipMemcpy(dst.p, src, n * sizeof(float), hipMemcpyHostToDevice): ") + hipGetErrorString(e));  // (the text these hooks have always given)
    return p;
  }
  template <typename F> int run(F&& launch) {
    if (rc) return rc;
    launch();
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(d->stream));
    for (const Back& b : back) HIPCHK(hipMemcpy(b.host, b.dev, b.bytes, hipMemcpyDeviceToHost));
    return PHX_OK;
  }
};

}  // namespace phx
