// device.cpp — host side of the gfx950 device: the C ABI of include/phx_xpu.h.
//
// Mirrors cpu_t (reference src/xpu/cpu.cpp:208-248): preprocess() flattens the scene and builds the
// accelerator (cpu.cpp:35-44), start() spawns a driver thread that drains the shared tile queue
// (cpu.cpp:223-238) — in batches of many tiles, each carried through the wavefront kernels of
// trace.hip, shade_lambert.hip, shade_general.hip, film_hooks.hip — and hands finished tiles to the film sink (cpu.cpp:201), join() waits for it.
// What needs no device lives beside this file: scene_flatten.cpp is the host-only half of preprocess, frame_plan.cpp that of the frame driver
// (the film's pixel layout, the pixel cap, the batch cutter, the pass schedule), denoise_check.cpp the argument check of the film denoiser
// (denoise.hip, a post-process no frame launches), accumulate_check.cpp that of film accumulation (accumulate.hip, likewise); here are the allocations, the launches and the waits.
// There is no CPU rendering path in this library: without a gfx950 device every entry point fails.
#include "../../include/phx_xpu.h"
#include "accumulate_check.h"
#include "bvh_build.h"
#include "bvh_gpu.h"
#include "denoise_check.h"
#include "frame_plan.h"
#include "guides_check.h"
#include "kernels.h"
#include "scene_flatten.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <mutex>
#include <new>
#include <optional>
#include <string>
#include <thread>
#include <vector>

using namespace phx;

#ifndef PHX_TEST_HOOKS
#define PHX_TEST_HOOKS 0  /* 1 only in the twin library libphx_hip_hooks.so (fault injection for the tests); never in the product build */
#endif

namespace {

// Errors: every thread has its own last-error string; a driver thread's error is also kept with its device (phx_device::
// frame_error) and handed to the thread that calls phx_dev_join, so two devices rendering at once never share a buffer.
thread_local std::string g_error;

int fail(int code, const std::string& msg) { g_error = msg; return code; }

#define HIPCHK(expr)                                                                                     \
  do {                                                                                                   \
    hipError_t e_ = (expr);                                                                              \
    if (e_ != hipSuccess) return fail(PHX_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
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
// phx_adaptive: the name of the first field outside its range, or nullptr
const char* adaptive_invalid(const phx_adaptive& a) {
  if (!std::isfinite(a.threshold) || a.threshold < 0.0f) return "threshold";
  if (!std::isfinite(a.floor) || a.floor < 0.0f) return "floor";
  if (a.min_samples < 2u) return "min_samples";
  if (a.step < 1u) return "step";
  for (uint32_t w : a.reserved) if (w) return "reserved";
  return nullptr;
}
// what the selection behind a round that ended at n of spp samples takes from the setting (phx_adaptive: q, g, k), in binary64
void adaptive_args(const phx_adaptive& a, uint32_t n, uint32_t spp, AdaptiveArgs& A) {
  A.q = (double)n / (double)(n - 1u);
  A.g = ((double)a.floor * (double)n) / (double)spp;
  A.tau = (double)a.threshold;
  A.k = (double)spp / (double)n;
  A.n = (float)n;
}
// The film jitter of sample index 0 .. spp - 1, shared by all pixels (run_frame and phx_dev_render_guides read the same table): sampler_t::preprocess
// (sampling.cpp:98-112) with sample::stratified_2d (math/sampling.hpp:65-77), numbers from the counter sampler.  A cell past spp - 1 (spp is not a
// square) is dropped, and an index no cell names keeps (0, 0).
std::vector<float2> jitter_table(uint64_t seed, uint32_t spp) {
  std::vector<float2> jit(spp, make_float2(0.0f, 0.0f));
  const uint32_t spd = (uint32_t)std::lroundf(std::sqrt((float)spp));
  const float step = 1.0f / (float)spd;
  float dy = 0.0f;
  for (uint32_t i = 0; i < spd; ++i, dy += step) {
    float dx = 0.0f;
    for (uint32_t j = 0; j < spd; ++j, dx += step) {
      const uint32_t cell = j * spd + i;
      const uint32_t key = path_key(seed, FILM_JITTER_STREAM, cell);
      const float a = dx + draw_f32(key, 0) * step;
      const float b = dy + draw_f32(key, 1) * step;
      if (cell < spp) jit[cell] = make_float2(a, b);
    }
  }
  return jit;
}
static_assert(PathQueues::bytes_per_path(false) == queue_bytes_per_path(false) && PathQueues::bytes_per_path(true) == queue_bytes_per_path(true),
              "what path_budget divides the device's memory by (frame_plan.h: FilmLayout::path_bytes)");

bool host_timing() {  // PHX_HOST_TIMING, read at the first frame: where a frame's and a batch's host time goes, on stderr (probe)
  static const bool on = std::getenv("PHX_HOST_TIMING") != nullptr;
  return on;
}
using Clock = std::chrono::steady_clock;
double ms_between(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); }

// A word in pinned memory that the host set to 0xffffffff and a kernel overwrites: its value once the kernel has written it.  Never for ever:
// the clock is looked at every 1 024 spins, and after two seconds the answer is 0xffffffff — a device that has stopped (fault, watchdog) is
// reported by the caller's next synchronisation, not here.
uint32_t device_word(const uint32_t* w) {
  const auto t0 = Clock::now();
  for (uint32_t spins = 0;; ++spins) {
    const uint32_t v = __atomic_load_n(w, __ATOMIC_ACQUIRE);
    if (v != 0xffffffffu || ((spins & 1023u) == 1023u && Clock::now() - t0 > std::chrono::seconds(2))) return v;
  }
}

}  // namespace

struct phx_tiles {
  std::vector<phx_tile> tiles;
  std::atomic<uint32_t> cursor{0};
};

struct phx_device {
  phx_options opt{};
  int hip_device = 0;
  hipStream_t stream = nullptr;
  bool preprocessed = false;

  // scene
  DevBuf<PoolElem> d_pool; DevBuf<uint32_t> d_prim_material; DevBuf<float> d_elem_normals; DevBuf<float4> d_elem_shade; DevBuf<uint2> d_spill;
  DevBuf<DevMaterial> d_materials; DevBuf<DevMatLite> d_mat_lite; DevBuf<DevLight> d_lights; DevBuf<DevLightTri> d_light_tris;
  // image textures: held only while the preprocessed scene has a textured lobe
  DevBuf<float2> d_elem_uv; DevBuf<DevTexture> d_textures; DevBuf<float4> d_texels; DevBuf<uint32_t> d_lobe_tex; DevBuf<DevTexScene> d_tex_scene;
  DevBuf<uint32_t> d_mat_emit_tex;  // per material: the image on its emission + 1 (scenes with emitter images only)
  DevBuf<float> d_env_cdf;          // PHX_LIGHT_INCLUDE_ENVIRONMENT: the environment's direction tables (FlatScene::env_cdf)
  DevScene scene{};
  uint32_t num_materials = 0, num_textures = 0;
  std::vector<uint8_t> mat_masked;  // per material: some lobe's factor is an image mask (the untextured KAT hooks refuse those)
  uint32_t env_tex = 0, env_mapping = 0; float env_e[3] = {0.0f, 0.0f, 0.0f};  // the environment's image (texture + 1, 0 = none), mapping and emission
  uint64_t bvh_nodes = 0, bvh_bytes = 0, num_triangles = 0;
  double preprocess_ms = 0, bvh_build_ms = 0;

  // pass buffers
  PathQueues queues;
  DevBuf<uint32_t> counters; DevBuf<DevStats> dstats; DevBuf<uint32_t> pix_xy; DevBuf<float2> jitter; DevBuf<float> acc;
  uint64_t jitter_seed = 0; uint32_t jitter_spp = 0;  // what the jitter table on the device was made for
  PinnedBuf<float> h_acc;      // pinned staging for add_tile
  PinnedBuf<uint32_t> h_qlen;  // pinned, device-visible: queue lengths published by k_trace, one word per (pass, step) of a batch (enqueue_batch)
  std::vector<phx_tile> pix_xy_tiles;          // the tiles pix_xy currently describes
  // adaptive sampling (phx_dev_set_adaptive), held only by a device that rendered a frame with it: the working copies of acc and pix_xy that a
  // pass over the pixels still active reads (working row w = row sel_idx[.][w] of the batch), the two lists a selection reads and writes
  // by turns, a word per workgroup of the selection, and the pinned word through which the host reads how many pixels go on
  DevBuf<float> w_acc; DevBuf<uint32_t> w_xy, sel_idx[2], sel_blocks;
  PinnedBuf<uint32_t> h_sel;
  phx_adaptive adaptive{}; bool adaptive_on = false;
  double guides_ms[2] = {};    // phx_dev_guides_times: the last phx_dev_render_guides' kernel and call
  double accumulate_ms[2] = {};  // phx_dev_accumulate_times: the last phx_dev_film_accumulate's kernel and call
  double denoise_ms[11] = {};  // phx_dev_denoise_times: the last phx_dev_denoise's stages (it holds no device memory between calls)

  // frame
  phx_frame frame{};
  FilmLayout layout;  // of `frame` (run_frame)
  // ONE driver thread per device, kept across frames (cpu_t spawns its workers per frame, src/xpu/cpu.cpp:223-238; here a frame of a rank
  // of eight lasts 9 ms and a thread start costs 50-70 us of it): phx_dev_start hands it the frame, phx_dev_join waits for `frame_done`
  std::thread driver;
  std::mutex mu; std::condition_variable cv;
  bool frame_pending = false, frame_done = false, quit = false;
  bool running = false;
  int frame_status = PHX_OK;
  std::string frame_error;  // g_error of the driver thread, copied when its frame ends
  phx_stats stats{};
  TracePlan plan{};
  uint64_t paths_in_flight = 0;
  // the committed scene reads the barycentrics of a hit (commit_scene): the passes carry PassBuffers::hit_uv and the trace kernels run as UV = true
  bool hit_uv = false;
  double bvh_cost_model = 0; uint32_t bvh_built_on_device = 0;
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
  Clock::time_point t_start, t_enq, t_sync;  // host timing probe (PHX_HOST_TIMING)

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
    return d_pool.bytes() + d_prim_material.bytes() + d_elem_normals.bytes() + d_elem_shade.bytes() + d_spill.bytes() + d_materials.bytes() + d_mat_lite.bytes() +
           d_lights.bytes() + d_light_tris.bytes() + queues.bytes() + counters.bytes() + dstats.bytes() + pix_xy.bytes() + jitter.bytes() + acc.bytes() +
           d_elem_uv.bytes() + d_textures.bytes() + d_texels.bytes() + d_lobe_tex.bytes() + d_tex_scene.bytes() + d_mat_emit_tex.bytes() + d_env_cdf.bytes() +
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
  void driver_loop();
  int run_frame();
  const phx_adaptive* adaptive_setting() const { return adaptive_on ? &adaptive : nullptr; }
  // the passes of a batch of P pixels under today's budget (frame_plan.h: plan_passes; with samples_in_flight set the device is not asked)
  uint32_t plan_batch(uint32_t P, uint32_t limit, std::vector<Pass>& passes) const {
    return plan_passes(P, opt.samples_per_pixel, opt.samples_in_flight, opt.samples_in_flight ? 0 : path_budget(layout.path_bytes), adaptive_setting(), limit, passes);
  }
  int enqueue_batch(BatchLaunches& g, const PassBuffers& B0, uint32_t P, const std::vector<Pass>& passes);
  int render_batch(const std::vector<phx_tile>& tiles);
};

// ---- preprocess ---------------------------------------------------------------------------------------
// Three stages: the state checks, flatten_scene (scene_flatten.cpp: validation and everything derived on the host — a refusal leaves the
// device and its previous scene untouched), and commit_scene, which builds the tree and replaces the device's tables.
namespace {

// No C++ exception may cross the C ABI (the reference's own std::runtime_error cases become status codes): every entry
// point that allocates or spawns runs its body through guarded().
template <typename F>
int guarded(F&& body) {
  try { return body(); }
  catch (const std::bad_alloc&) { return fail(PHX_ERR_OOM, "host memory allocation failed"); }
  catch (const std::exception& e) { return fail(PHX_ERR_DEVICE, std::string("unexpected exception: ") + e.what()); }
  catch (...) { return fail(PHX_ERR_DEVICE, "unexpected exception"); }
}

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
  if (sc.any_tex & SC_LIGHTS_BY_POWER) {  // the selection table rides directly behind the light records (shade_common.h: light_pcdf), padded to whole records
    const size_t nl = fs.lights.size();
    fs.lights.resize(nl + (fs.light_pcdf.size() * sizeof(float) + sizeof(DevLight) - 1) / sizeof(DevLight), DevLight{});
    std::memcpy(static_cast<void*>(fs.lights.data() + nl), fs.light_pcdf.data(), fs.light_pcdf.size() * sizeof(float));
  }
  if (sc.any_tex & SC_LIGHTS_BY_AREA) {  // the CDF rides behind the light table (shade_common.h: light_cdf): one float per light triangle, in records of the table's size
    const size_t nl = fs.lights.size();
    fs.lights.resize(nl + (fs.light_cdf.size() * sizeof(float) + sizeof(DevLight) - 1) / sizeof(DevLight), DevLight{});
    std::memcpy(static_cast<void*>(fs.lights.data() + nl), fs.light_cdf.data(), fs.light_cdf.size() * sizeof(float));
  }
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
    const std::vector<DevTexScene> ts{DevTexScene{any_tex ? d->d_elem_uv.p : nullptr, d->d_textures.p, d->d_texels.p, any_tex ? d->d_lobe_tex.p : nullptr,
                                                  fs.env_tex ? fs.env_tex - 1u : 0u, fs.env_mapping, fs.any_emit_tex ? 1u : 0u, fs.env_p,
                                                  fs.any_emit_tex ? d->d_mat_emit_tex.p : nullptr, (sc.any_tex & SC_LIGHTS_ENV) ? d->d_env_cdf.p : nullptr}};
    if ((rc = d->d_tex_scene.upload(ts))) return rc;
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
    default: return 0;
  }
}

int phx_dev_set_adaptive(phx_device* d, const phx_adaptive* a) {
  if (!d) return fail(PHX_ERR_ARG, "set_adaptive: null device");
  if (d->running) return fail(PHX_ERR_STATE, "set_adaptive while a frame is running");
  if (!a) { d->adaptive_on = false; return PHX_OK; }
  if (const char* field = adaptive_invalid(*a)) return fail(PHX_ERR_ARG, std::string("set_adaptive: ") + field + " is outside its range (phx_adaptive)");
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
int phx_tiles_next(void* tiles, phx_tile* out) {
  phx_tiles* q = (phx_tiles*)tiles;
  const uint32_t t = q->cursor++;
  if (t < q->tiles.size()) { *out = q->tiles[t]; return 1; }
  return 0;
}
uint32_t phx_tiles_count(const phx_tiles* q) { return q ? (uint32_t)q->tiles.size() : 0; }
void phx_tiles_reset(phx_tiles* q) { if (q) q->cursor = 0; }
void phx_tiles_free(phx_tiles* q) { delete q; }

// ---- stage-level entry points ----------------------------------------------------------------------------
}  // extern "C"

namespace {

// Device copies of a stage hook's arrays.  in() uploads, out() allocates and remembers where the result goes, run() launches, waits and copies
// back.  The first array enters the hook's device (after the hook's own argument checks, as ever), and the caller's device comes back when the
// hook returns.  The first failure sticks (rc), and run() returns it without launching.
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

// A stage hook: no exception leaves it, and it needs a preprocessed scene.  `body` does the hook's own argument checks, stages its arrays and runs its launch.
template <typename F>
int stage_hook(phx_device* d, const char* name, F&& body) {
  return guarded([&]() -> int {
    if (!d || !d->preprocessed) return fail(PHX_ERR_STATE, std::string(name) + " before preprocess");
    Staging s{d};
    return body(s);
  });
}

}  // namespace

extern "C" {

int phx_dev_trace(phx_device* d, uint32_t n, const float* o, const float* dir, const float* tmax, int shadow,
                  float* t, float* u, float* v, uint32_t* prim, uint8_t* hit) {
  return stage_hook(d, "trace", [&](Staging& s) -> int {
    if (n == 0) return PHX_OK;
    std::vector<float4> ro(n), rd(n), hh(n);
    for (uint32_t i = 0; i < n; ++i) { ro[i] = make_float4(o[3 * i], o[3 * i + 1], o[3 * i + 2], 0.0f); rd[i] = make_float4(dir[3 * i], dir[3 * i + 1], dir[3 * i + 2], tmax[i]); }
    const float4 *a = s.in(ro.data(), n), *b = s.in(rd.data(), n); float4* c = s.out(hh.data(), n);
    if (const int rc = s.run([&] { launch_trace_rays(d->stream, d->scene, n, a, b, c, shadow); })) return rc;
    for (uint32_t i = 0; i < n; ++i) {  // k_trace_rays stores the primitive id (scene_t::triangles() order) in w, 0xffffffff on a miss
      const uint32_t tri = bits_of(hh[i].w);
      if (t) t[i] = hh[i].x;
      if (u) u[i] = hh[i].y;
      if (v) v[i] = hh[i].z;
      if (prim) prim[i] = tri;
      if (hit) hit[i] = tri != 0xffffffffu;
    }
    return PHX_OK;
  });
}

int phx_dev_bsdf_f(phx_device* d, uint32_t material, uint32_t n, const float* n3, const float* wi3, const float* wo3, float* f3) {
  return stage_hook(d, "bsdf_f", [&](Staging& s) -> int {
    if (material >= d->num_materials) return fail(PHX_ERR_ARG, "material out of range");
    if (d->mat_masked[material]) return fail(PHX_ERR_ARG, "bsdf_f: the material has image-masked lobes, whose weights need the hit's (s, t) (see phx_dev_lobe_weights)");
    if (n == 0) return PHX_OK;
    const size_t n3s = 3 * (size_t)n;
    const float *a = s.in(n3, n3s), *b = s.in(wi3, n3s), *c = s.in(wo3, n3s); float* f = s.out(f3, n3s);
    return s.run([&] { launch_bsdf_f(d->stream, d->d_materials.p + material, n, a, b, c, f); });
  });
}

// (no stage_hook: the film stage reads no scene, so a device that has preprocessed nothing serves)
int phx_dev_film_moments(phx_device* d, uint32_t num_pixels, uint32_t num_samples, uint32_t samples_done, float inv, const float* radiance, float* acc) {
  return guarded([&]() -> int {
    if (!d) return fail(PHX_ERR_ARG, "film_moments: null device");
    if (d->running) return fail(PHX_ERR_STATE, "film_moments while a frame is running");
    if (num_pixels == 0 || num_samples == 0) return PHX_OK;
    if (!radiance || !acc) return fail(PHX_ERR_ARG, "film_moments: null argument");
    const size_t npaths = (size_t)num_pixels * num_samples;
    if (npaths >= 0x7fffffffull) return fail(PHX_ERR_ARG, "film_moments: too many samples");
    Staging s{d};
    const float4* pr = reinterpret_cast<const float4*>(s.in(radiance, 4 * npaths));
    float* a = s.out(acc, 6 * (size_t)num_pixels);
    if (s.rc) return s.rc;
    HIPCHK(hipMemcpy(a, acc, 6 * (size_t)num_pixels * sizeof(float), hipMemcpyHostToDevice));
    PassBuffers B{};
    B.pr = const_cast<float4*>(pr); B.acc = a; B.num_pixels = num_pixels; B.num_samples = num_samples; B.xstride = 6;
    return s.run([&] { launch_film_moments(d->stream, B, num_samples, inv, samples_done, 3); });
  });
}

// (no stage_hook: the denoiser reads a film and no scene)
int phx_dev_denoise(phx_device* d, const phx_denoise* q, const float* film_in, float* film_out) { return phx_dev_denoise_guided(d, q, nullptr, film_in, film_out); }

// g == nullptr or g->flags == 0: the unguided filter, by the launches it has always had
int phx_dev_denoise_guided(phx_device* d, const phx_denoise* q, const phx_denoise_guides* g, const float* film_in, float* film_out) {
  return guarded([&]() -> int {
    if (!d) return fail(PHX_ERR_ARG, "denoise: null device");
    if (d->running) return fail(PHX_ERR_STATE, "denoise while a frame is running");
    if (!q) return fail(PHX_ERR_ARG, "denoise: null argument");
    std::string why;
    if (const int rc = denoise_check(*q, film_in, film_out, why)) return fail(rc, why);
    if (g && !g->flags) g = nullptr;
    if (g) if (const int rc = denoise_guides_check(*q, *g, why)) return fail(rc, why);
    const auto t0 = Clock::now();
    DeviceScope on(d->hip_device);
    if (!on.ok) return fail(PHX_ERR_DEVICE, "hipSetDevice failed");
    std::fill(std::begin(d->denoise_ms), std::end(d->denoise_ms), 0.0);
    const size_t npix = (size_t)q->width * q->height, film_bytes = npix * q->xstride * sizeof(float);
    // everything the call holds on the device lives in these and goes with them, on every way out
    DevBuf<float> staged, gstaged; DevBuf<float4> c[2], v[2], n, gx; DevBuf<double> e[2];
    struct Events {
      std::vector<hipEvent_t> ev;
      ~Events() { for (hipEvent_t x : ev) (void)hipEventDestroy(x); }
      int mark(hipStream_t s) { hipEvent_t x; HIPCHK(hipEventCreate(&x)); ev.push_back(x); HIPCHK(hipEventRecord(x, s)); return PHX_OK; }
    } events;
    const float* src = film_in; float* dst = film_out;
    if (!q->on_device) {  // host films: one device copy, denoised in place
      if (const int rc = staged.alloc(npix * q->xstride)) return rc;
      HIPCHK(hipMemcpy(staged.p, film_in, film_bytes, hipMemcpyHostToDevice));
      src = dst = staged.p;
    }
    if (q->iterations) {
      for (int k = 0; k < 2; ++k) {
        if (const int rc = c[k].alloc(npix)) return rc;
        if (const int rc = v[k].alloc(npix)) return rc;
        if (const int rc = e[k].alloc(npix)) return rc;
      }
      if (const int rc = n.alloc(npix)) return rc;
      DenoiseGuideArgs G{};
      if (g) {
        G.guides = g->guides; G.xstride = g->xstride; G.flags = g->flags;
        G.albedo_floor = (double)g->albedo_floor; G.tol_scale = (double)g->sigma_x * (double)g->plane_scale;
        if (!q->on_device) {  // host guides: a device copy, like the film's
          if (const int rc = gstaged.alloc(npix * g->xstride)) return rc;
          HIPCHK(hipMemcpy(gstaged.p, g->guides, npix * g->xstride * sizeof(float), hipMemcpyHostToDevice));
          G.guides = gstaged.p;
        }
        if (g->flags & PHX_GUIDE_PLANE) { if (const int rc = gx.alloc(npix)) return rc; G.x = gx.p; }
      }
      DenoiseArgs A{};
      A.width = q->width; A.height = q->height; A.xstride = q->xstride; A.normals_offset = q->normals_offset; A.m2_offset = q->m2_offset;
      A.samples_offset = q->samples_offset; A.spp = q->spp; A.normal_power_log2 = q->normal_power_log2; A.sigma_l = (double)q->sigma_l;
      for (int k = 0; k < 2; ++k) { A.c[k] = c[k].p; A.v[k] = v[k].p; A.e[k] = e[k].p; }
      A.n = n.p;
      if (const int rc = events.mark(d->stream)) return rc;
      if (g) launch_denoise_pack_guided(d->stream, A, G, src); else launch_denoise_pack(d->stream, A, src);
      if (const int rc = events.mark(d->stream)) return rc;
      for (uint32_t i = 0; i < q->iterations; ++i) {
        if (g) launch_denoise_iteration_guided(d->stream, A, G, (int)(i & 1u), 1u << i); else launch_denoise_iteration(d->stream, A, (int)(i & 1u), 1u << i);
        if (const int rc = events.mark(d->stream)) return rc;
      }
      if (dst != src) HIPCHK(hipMemcpyAsync(dst, src, film_bytes, hipMemcpyDeviceToDevice, d->stream));
      if (g) launch_denoise_unpack_guided(d->stream, A, G, (int)(q->iterations & 1u), dst); else launch_denoise_unpack(d->stream, A, (int)(q->iterations & 1u), dst);
      if (const int rc = events.mark(d->stream)) return rc;
    } else if (dst != src) HIPCHK(hipMemcpyAsync(dst, src, film_bytes, hipMemcpyDeviceToDevice, d->stream));
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(d->stream));
    if (!q->on_device) HIPCHK(hipMemcpy(film_out, staged.p, film_bytes, hipMemcpyDeviceToHost));
    for (size_t k = 0; k + 1 < events.ev.size(); ++k) {
      float ms = 0.0f;
      HIPCHK(hipEventElapsedTime(&ms, events.ev[k], events.ev[k + 1]));
      d->denoise_ms[k == 0 ? 0 : k <= q->iterations ? k : 9] = ms;
    }
    d->denoise_ms[10] = ms_between(t0, Clock::now());
    return PHX_OK;
  });
}

// The first-hit guide film (phx_guides; guides.hip).  Everything the call holds on the device lives in the DevBufs below and goes with them.
int phx_dev_render_guides(phx_device* d, const phx_guides* g, float* film) {
  return guarded([&]() -> int {
    if (!d) return fail(PHX_ERR_ARG, "render_guides: null device");
    if (!d->preprocessed) return fail(PHX_ERR_STATE, "render_guides before preprocess");
    if (d->running) return fail(PHX_ERR_STATE, "render_guides while a frame is running");
    if (!g) return fail(PHX_ERR_ARG, "render_guides: null argument");
    const uint32_t W = d->scene.width, H = d->scene.height, spp = d->opt.samples_per_pixel;
    std::string why;
    if (const int rc = guides_check(*g, W, H, spp, film, why)) return fail(rc, why);
    const auto t0 = Clock::now();
    d->guides_ms[0] = d->guides_ms[1] = 0.0;
    DeviceScope on(d->hip_device);
    if (!on.ok) return fail(PHX_ERR_DEVICE, "hipSetDevice failed");
    const size_t npix = (size_t)W * H;
    std::vector<uint32_t> xy(npix);
    for (uint32_t y = 0; y < H; ++y) for (uint32_t x = 0; x < W; ++x) xy[(size_t)y * W + x] = x | y << 16;
    DevBuf<uint32_t> d_xy; DevBuf<float2> d_jit; DevBuf<float> staged;
    if (const int rc = d_xy.upload(xy)) return rc;
    if (const int rc = d_jit.upload(jitter_table(g->sampler_seed, spp))) return rc;
    float* dst = film;
    if (!g->on_device) { if (const int rc = staged.alloc(npix * 8)) return rc; dst = staged.p; }
    PassBuffers B{};
    B.pix_xy = d_xy.p; B.jitter = d_jit.p; B.num_pixels = (uint32_t)npix; B.num_samples = g->samples; B.seed = g->sampler_seed;
    struct Events {
      hipEvent_t ev[2] = {nullptr, nullptr};
      ~Events() { for (hipEvent_t x : ev) if (x) (void)hipEventDestroy(x); }
    } events;
    for (hipEvent_t& x : events.ev) HIPCHK(hipEventCreate(&x));
    HIPCHK(hipEventRecord(events.ev[0], d->stream));
    launch_guides(d->stream, d->scene, B, dst);
    HIPCHK(hipEventRecord(events.ev[1], d->stream));
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(d->stream));
    if (!g->on_device) HIPCHK(hipMemcpy(film, staged.p, npix * 8 * sizeof(float), hipMemcpyDeviceToHost));
    float ms = 0.0f;
    HIPCHK(hipEventElapsedTime(&ms, events.ev[0], events.ev[1]));
    d->guides_ms[0] = ms; d->guides_ms[1] = ms_between(t0, Clock::now());
    return PHX_OK;
  });
}

// Film accumulation (phx_accumulate; accumulate.hip).  Everything the call holds on the device lives in the DevBufs below and goes with them.
// (no stage_hook: the call reads two films and no scene)
int phx_dev_film_accumulate(phx_device* d, const phx_accumulate* a, float* acc, const float* frame_film, phx_accumulate_summary* summary) {
  return guarded([&]() -> int {
    if (!d) return fail(PHX_ERR_ARG, "accumulate: null device");
    if (d->running) return fail(PHX_ERR_STATE, "accumulate while a frame is running");
    if (!a) return fail(PHX_ERR_ARG, "accumulate: null argument");
    std::string why;
    if (const int rc = accumulate_check(*a, acc, frame_film, why)) return fail(rc, why);
    const auto t0 = Clock::now();
    d->accumulate_ms[0] = d->accumulate_ms[1] = 0.0;
    DeviceScope on(d->hip_device);
    if (!on.ok) return fail(PHX_ERR_DEVICE, "hipSetDevice failed");
    const size_t npix = (size_t)a->width * a->height, floats_a = npix * a->xstride_a, floats_b = npix * a->xstride_b;
    const size_t slot_words = (size_t)PHX_ACCUMULATE_SLOTS * PHX_ACCUMULATE_SLOT_WORDS;
    DevBuf<float> staged_a, staged_b; DevBuf<unsigned long long> counters;
    float* dst = acc; const float* src = frame_film;
    if (!a->on_device) {  // host films: device copies, acc's pooled in place and copied back
      if (const int rc = staged_a.alloc(floats_a)) return rc;
      if (const int rc = staged_b.alloc(floats_b)) return rc;
      HIPCHK(hipMemcpy(staged_a.p, acc, floats_a * sizeof(float), hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(staged_b.p, frame_film, floats_b * sizeof(float), hipMemcpyHostToDevice));
      dst = staged_a.p; src = staged_b.p;
    }
    if (summary) {
      if (const int rc = counters.alloc(slot_words)) return rc;
      HIPCHK(hipMemsetAsync(counters.p, 0, slot_words * sizeof(unsigned long long), d->stream));
    }
    AccumulateArgs A{};
    A.num_pixels = npix;
    A.xstride_a = a->xstride_a; A.normals_offset_a = a->normals_offset_a; A.m2_offset_a = a->m2_offset_a; A.samples_offset_a = a->samples_offset_a;
    A.xstride_b = a->xstride_b; A.normals_offset_b = a->normals_offset_b; A.m2_offset_b = a->m2_offset_b; A.samples_offset_b = a->samples_offset_b;
    A.spp_b = a->spp_b; A.tau = (double)a->tau; A.floor = (double)a->floor;
    struct Events {
      hipEvent_t ev[2] = {nullptr, nullptr};
      ~Events() { for (hipEvent_t x : ev) if (x) (void)hipEventDestroy(x); }
    } events;
    for (hipEvent_t& x : events.ev) HIPCHK(hipEventCreate(&x));
    HIPCHK(hipEventRecord(events.ev[0], d->stream));
    launch_accumulate(d->stream, A, dst, src, counters.p);
    HIPCHK(hipEventRecord(events.ev[1], d->stream));
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(d->stream));
    if (!a->on_device) HIPCHK(hipMemcpy(acc, staged_a.p, floats_a * sizeof(float), hipMemcpyDeviceToHost));
    if (summary) {
      std::vector<unsigned long long> slots(slot_words);
      HIPCHK(hipMemcpy(slots.data(), counters.p, slot_words * sizeof(unsigned long long), hipMemcpyDeviceToHost));
      unsigned long long c[4] = {0ull, 0ull, 0ull, 0ull};  // integers, modulo 2^64: whatever the order, the same sums
      for (size_t s = 0; s < (size_t)PHX_ACCUMULATE_SLOTS; ++s) for (int k = 0; k < 4; ++k) c[k] += slots[s * PHX_ACCUMULATE_SLOT_WORDS + k];
      summary->pixels = c[0]; summary->invalid = c[1]; summary->converged = c[2]; summary->samples = c[3];
    }
    float ms = 0.0f;
    HIPCHK(hipEventElapsedTime(&ms, events.ev[0], events.ev[1]));
    d->accumulate_ms[0] = ms; d->accumulate_ms[1] = ms_between(t0, Clock::now());
    return PHX_OK;
  });
}

int phx_dev_accumulate_times(const phx_device* d, double* ms) {
  if (!d || !ms) return fail(PHX_ERR_ARG, "accumulate_times: null argument");
  ms[0] = d->accumulate_ms[0]; ms[1] = d->accumulate_ms[1];
  return PHX_OK;
}

int phx_dev_guides_times(const phx_device* d, double* ms) {
  if (!d || !ms) return fail(PHX_ERR_ARG, "guides_times: null argument");
  ms[0] = d->guides_ms[0]; ms[1] = d->guides_ms[1];
  return PHX_OK;
}

int phx_dev_denoise_times(const phx_device* d, double* ms) {
  if (!d || !ms) return fail(PHX_ERR_ARG, "denoise_times: null argument");
  std::copy(std::begin(d->denoise_ms), std::end(d->denoise_ms), ms);
  return PHX_OK;
}

// (no stage_hook either: the selection reads no scene)
int phx_dev_adaptive_select(phx_device* d, uint32_t num_active, const uint32_t* active, uint32_t num_rows, float* acc, uint32_t samples_done, uint32_t spp,
                            const phx_adaptive* a, uint32_t* survivors, uint32_t* num_survivors) {
  return guarded([&]() -> int {
    if (!d) return fail(PHX_ERR_ARG, "adaptive_select: null device");
    if (d->running) return fail(PHX_ERR_STATE, "adaptive_select while a frame is running");
    if (!acc || !a || !survivors || !num_survivors) return fail(PHX_ERR_ARG, "adaptive_select: null argument");
    if (samples_done < 2u || samples_done >= spp) return fail(PHX_ERR_ARG, "adaptive_select: samples_done must be at least 2 and below spp");
    if (const char* field = adaptive_invalid(*a)) return fail(PHX_ERR_ARG, std::string("adaptive_select: ") + field + " is outside its range (phx_adaptive)");
    if (num_active > num_rows) return fail(PHX_ERR_ARG, "adaptive_select: more active rows than rows");
    for (uint32_t i = 0; active && i < num_active; ++i) {
      if (active[i] >= num_rows) return fail(PHX_ERR_ARG, "adaptive_select: an index past num_rows");
      if (i && active[i] <= active[i - 1]) return fail(PHX_ERR_ARG, "adaptive_select: the indices must ascend strictly");
    }
    *num_survivors = 0;
    if (num_active == 0) return PHX_OK;
    Staging s{d};
    const size_t nfl = 7 * (size_t)num_rows;
    AdaptiveArgs A{};
    A.acc = s.out(acc, nfl); A.xstride = 7; A.m2_offset = 3; A.samples_offset = 6;
    A.active = active ? s.in(active, num_active) : nullptr; A.num_active = num_active;
    adaptive_args(*a, samples_done, spp, A);
    uint32_t* scratch = s.out<uint32_t>(nullptr, (num_active + PHX_ADAPTIVE_BLOCK - 1) / PHX_ADAPTIVE_BLOCK);
    uint32_t *surv = s.out(survivors, num_active), *total = s.out(num_survivors, 1);
    if (s.rc) return s.rc;
    HIPCHK(hipMemcpy(A.acc, acc, nfl * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(hipMemsetAsync(surv, 0, (size_t)num_active * sizeof(uint32_t), d->stream));  // the words past the survivors: zeros, not what the allocation held
    return s.run([&] { launch_adaptive_select(d->stream, A, scratch, surv, total); });
  });
}

int phx_dev_bsdf_sample(phx_device* d, uint32_t material, uint32_t n, const float* n3, const float* wi3, const float* u2,
                        float* wo3, float* f3, float* pdf, uint32_t* flags) {
  return stage_hook(d, "bsdf_sample", [&](Staging& s) -> int {
    if (material >= d->num_materials) return fail(PHX_ERR_ARG, "material out of range");
    if (d->mat_masked[material]) return fail(PHX_ERR_ARG, "bsdf_sample: the material has image-masked lobes, whose weights need the hit's (s, t) (see phx_dev_lobe_weights)");
    if (n == 0) return PHX_OK;
    const size_t n3s = 3 * (size_t)n;
    const float *a = s.in(n3, n3s), *b = s.in(wi3, n3s), *c = s.in(u2, 2 * (size_t)n);
    float *wo = s.out(wo3, n3s), *f = s.out(f3, n3s), *p = s.out(pdf, n); uint32_t* fl = s.out(flags, n);
    return s.run([&] { launch_bsdf_sample(d->stream, d->d_materials.p + material, n, a, b, c, wo, f, p, fl); });
  });
}

int phx_dev_texture_lookup(phx_device* d, uint32_t texture, uint32_t n, const float* st, float* rgb) {
  return stage_hook(d, "texture_lookup", [&](Staging& s) -> int {
    if (texture >= d->num_textures) return fail(PHX_ERR_ARG, "texture out of range (textures are kept only for scenes with a textured lobe)");
    if (n == 0) return PHX_OK;
    if (!st || !rgb) return fail(PHX_ERR_ARG, "texture_lookup: null argument");
    const float* a = s.in(st, 2 * (size_t)n); float* o = s.out(rgb, 3 * (size_t)n);
    return s.run([&] { launch_texture_lookup(d->stream, d->d_textures.p, d->d_texels.p, texture, n, a, o); });
  });
}

int phx_dev_lobe_weights(phx_device* d, uint32_t material, uint32_t n, const float* n3, const float* wi3, const float* st, float* w, uint32_t* kept) {
  return stage_hook(d, "lobe_weights", [&](Staging& s) -> int {
    if (material >= d->num_materials) return fail(PHX_ERR_ARG, "material out of range");
    if (n == 0) return PHX_OK;
    const bool tex = (d->scene.any_tex & SC_TEX_LOBES) != 0;  // the scene's lobes read images: st is needed
    if (!n3 || !wi3 || !w || !kept || (tex && !st)) return fail(PHX_ERR_ARG, "lobe_weights: null argument");
    const float *a = s.in(n3, 3 * (size_t)n), *b = s.in(wi3, 3 * (size_t)n), *c = tex ? s.in(st, 2 * (size_t)n) : nullptr;
    float* o = s.out(w, 3 * PHX_MAX_LOBES * (size_t)n); uint32_t* k = s.out(kept, n);
    return s.run([&] {
      launch_lobe_weights(d->stream, d->d_materials.p + material, tex ? d->d_textures.p : nullptr, d->d_texels.p, tex ? d->d_lobe_tex.p + 8 * (size_t)material : nullptr,
                          n, a, b, c, o, k);
    });
  });
}

int phx_dev_environment_lookup(phx_device* d, uint32_t n, const float* dirs, float* rgb) {
  return stage_hook(d, "environment_lookup", [&](Staging& s) -> int {
    if (!d->env_tex) return fail(PHX_ERR_ARG, "environment_lookup: the scene's environment has no image");
    if (n == 0) return PHX_OK;
    if (!dirs || !rgb) return fail(PHX_ERR_ARG, "environment_lookup: null argument");
    const float* a = s.in(dirs, 3 * (size_t)n); float* o = s.out(rgb, 3 * (size_t)n);
    return s.run([&] { launch_environment_lookup(d->stream, d->d_textures.p, d->d_texels.p, d->env_tex - 1u, d->env_mapping, d->env_e[0], d->env_e[1], d->env_e[2], n, a, o); });
  });
}

int phx_dev_light_sample(phx_device* d, uint32_t n, const float* u3, uint32_t* light, uint32_t* tri, float* bary, float* P, float* pdf) {
  return stage_hook(d, "light_sample", [&](Staging& s) -> int {
    if (n == 0) return PHX_OK;
    if (!u3 || !light || !tri || !bary || !P || !pdf) return fail(PHX_ERR_ARG, "light_sample: null argument");
    const float* a = s.in(u3, 3 * (size_t)n);
    uint32_t *ol = s.out(light, n), *ot = s.out(tri, n); float *ob = s.out(bary, 2 * (size_t)n), *oP = s.out(P, 3 * (size_t)n), *op = s.out(pdf, n);
    return s.run([&] { launch_light_sample(d->stream, d->scene, n, a, ol, ot, ob, oP, op); });
  });
}

int phx_dev_light_emission(phx_device* d, uint32_t n, const float* u3, float* st, float* e) {
  return stage_hook(d, "light_emission", [&](Staging& s) -> int {
    if (n == 0) return PHX_OK;
    if (!u3 || !st || !e) return fail(PHX_ERR_ARG, "light_emission: null argument");
    const float* a = s.in(u3, 3 * (size_t)n);
    float *os = s.out(st, 2 * (size_t)n), *oe = s.out(e, 3 * (size_t)n);
    return s.run([&] { launch_light_emission(d->stream, d->scene, n, a, os, oe); });
  });
}

int phx_dev_environment_sample(phx_device* d, uint32_t n, const float* u3, uint32_t* light, uint32_t* texel, float* st, float* dir, float* pdf, float* e) {
  return stage_hook(d, "environment_sample", [&](Staging& s) -> int {
    if (!(d->scene.any_tex & SC_LIGHTS_ENV)) return fail(PHX_ERR_ARG, "environment_sample: the scene does not sample its environment (light_sampling without PHX_LIGHT_INCLUDE_ENVIRONMENT)");
    if (n == 0) return PHX_OK;
    if (!u3 || !light || !texel || !st || !dir || !pdf || !e) return fail(PHX_ERR_ARG, "environment_sample: null argument");
    const float* a = s.in(u3, 3 * (size_t)n);
    uint32_t *ol = s.out(light, n), *ot = s.out(texel, 2 * (size_t)n);
    float *os = s.out(st, 2 * (size_t)n), *od = s.out(dir, 3 * (size_t)n), *op = s.out(pdf, n), *oe = s.out(e, 3 * (size_t)n);
    return s.run([&] { launch_environment_sample(d->stream, d->scene, d->env_e[0], d->env_e[1], d->env_e[2], n, a, ol, ot, os, od, op, oe); });
  });
}

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

// ---- the frame driver ------------------------------------------------------------------------------------
namespace {

void copy_stats(const DevStats& ds, phx_stats& stats) {  // what the kernels counted, into the frame's phx_stats
  stats.camera_samples = ds.camera_samples; stats.rays_closest = ds.rays_closest; stats.rays_shadow = ds.rays_shadow;
  stats.rays_masked = ds.rays_closest - ds.rays_shadow;  // every shaded slot is a shadow ray or a masked slot (spt.hpp:138-141)
  for (int k = 0; k < 2; ++k) { stats.node_visits_lds[k] = ds.node_visits_lds[k]; stats.node_visits_mem[k] = ds.node_visits_mem[k]; stats.tri_tests[k] = ds.tri_tests[k]; }
  stats.instrumented = launch_counts_traversal_work() ? 1 : 0;
  stats.wave_iters = ds.wave_iters; stats.node_block_execs = ds.node_block_execs; stats.tri_block_execs = ds.tri_block_execs; stats.refills = ds.refills;
  stats.idle_lane_iters = ds.idle_lane_iters; stats.tri_pending_lane_iters = ds.tri_pending_lane_iters;
  for (int k = 0; k < 8; ++k) { stats.stack_pushes[k] = ds.stack_pushes[k]; stats.tri_pairs_hist[k] = ds.tri_pairs_hist[k]; }
  stats.tri_pairs_pending = ds.tri_pairs_pending;
  stats.primary_packets = ds.primary_packets; stats.primary_fallbacks = ds.primary_fallbacks; stats.primary_node_tests = ds.primary_node_tests;
  stats.primary_tri_tests = ds.primary_tri_tests; stats.primary_tri_lanes_hit = ds.primary_tri_lanes_hit;
}

}  // namespace

void phx_device::driver_loop() {
  (void)hipSetDevice(hip_device);
  for (;;) {
    {
      std::unique_lock<std::mutex> lk(mu);
      cv.wait(lk, [this]() { return frame_pending || quit; });
      if (!frame_pending) return;  // quit, and no frame handed over: a frame that WAS started is rendered first (phx_dev_destroy joins it, include/phx_xpu.h)
      frame_pending = false;
    }
    const int st = guarded([this]() { return run_frame(); });
    {
      std::lock_guard<std::mutex> lk(mu);
      frame_status = st;
      frame_error = st != PHX_OK ? g_error : std::string();
      frame_done = true;
    }
    cv.notify_all();
  }
}

int phx_device::run_frame() {
  HIPCHK(hipSetDevice(hip_device));
  const auto t0 = Clock::now();
  std::memset(&stats, 0, sizeof(stats));
  int rc;
  if ((rc = dstats.alloc(1)) || (rc = counters.alloc(CNT_WORDS))) return rc;
  HIPCHK(hipMemsetAsync(dstats.p, 0, sizeof(DevStats), stream));
  HIPCHK(hipMemsetAsync(counters.p, 0, CNT_WORDS * sizeof(uint32_t), stream));

  // per-spp film jitter shared by all pixels: sampler_t::preprocess (sampling.cpp:98-112) with
  // sample::stratified_2d (math/sampling.hpp:65-77), numbers from the counter sampler
  const uint32_t spp = opt.samples_per_pixel;
  const std::vector<float2> jit = jitter_table(frame.sampler_seed, spp);
  if (jitter_seed != frame.sampler_seed || jitter_spp != spp || !jitter.p) {  // a frame loop presents the same seed again and again
    if ((rc = jitter.upload(jit))) return rc;
    jitter_seed = frame.sampler_seed; jitter_spp = spp;
  }

  // drain the shared tile queue in batches (cpu.cpp:233-234 pulls one tile at a time) of at most the frame's pixel cap, each in Morton order
  // (frame_plan.h: pixel_cap, BatchCutter)
  layout = FilmLayout(frame, adaptive_on);
  BatchCutter cutter{frame.next_tile, frame.tiles_user, pixel_cap(path_budget(layout.path_bytes), opt, adaptive_setting()), opt.tiles_per_batch, scene.width, scene.height};
  std::vector<phx_tile> tiles;
  std::string why;
  for (;;) {
    if ((rc = cutter.next(tiles, why))) return fail(rc, why);
    if (tiles.empty()) break;
    if ((rc = render_batch(tiles))) return rc;
    stats.tiles += tiles.size();
  }
  t_enq = Clock::now();
  HIPCHK(hipStreamSynchronize(stream));
  t_sync = Clock::now();
  DevStats ds;
  HIPCHK(hipMemcpy(&ds, dstats.p, sizeof(ds), hipMemcpyDeviceToHost));
  copy_stats(ds, stats);
  if (ds.watchdog) return fail(PHX_ERR_DEVICE, "k_trace: " + std::to_string(ds.watchdog) + " wave(s) hit the iteration watchdog: the frame is incomplete");
  if (ds.ring_watchdog) return fail(PHX_ERR_DEVICE, "k_shade_g: " + std::to_string(ds.ring_watchdog) + " wave(s) timed out waiting for a block of the append ring: the frame is incomplete");
  stats.trace_ms = stats.closest_ms + stats.shadow_ms + stats.primary_ms;
  stats.frame_ms = ms_between(t0, Clock::now());
  if (host_timing()) {
    auto ms = ms_between;
    std::fprintf(stderr, "host timing: start->thread %.3f  thread->sync-begin (enqueue etc.) %.3f  sync wait %.3f  stats %.3f | kernels on the GPU %.3f ms | start->done %.3f\n",
                 ms(t_start, t0), ms(t0, t_enq), ms(t_enq, t_sync), ms(t_sync, Clock::now()), stats.trace_ms + stats.shade_ms, ms(t_start, Clock::now()));
  }
  return PHX_OK;
}

int phx_device::render_batch(const std::vector<phx_tile>& tiles) {
  int rc;
  const auto tb0 = Clock::now();
  auto tb_alloc = tb0, tb_enq = tb0;
  uint32_t P = 0;
  for (auto& t : tiles) P += t.w * t.h;
  const uint32_t xs = layout.xstride;
  const bool normals = frame.normals_channel != 0;
  // the passes of the batch, and S, the most samples of a pixel any of them carries: what the queues are sized for
  std::vector<Pass> passes;
  uint32_t S = plan_batch(P, ~0u, passes);
  // The budget is a cached reading of the device's free memory (hipMemGetInfo costs ~0.1 ms).  It is only trusted while the queues this
  // object already holds are large enough: a batch that has to GROW them asks the device again — another device object, torch films or
  // RCCL buffers may have taken memory since the reading was made.
  if ((size_t)P * S > queues.capacity() && !opt.samples_in_flight) { budget_bytes = 0; S = plan_batch(P, ~0u, passes); }
  if ((size_t)P * S >= 0x7fffffffull) return fail(PHX_ERR_ARG, "too many paths in flight");

  // pixel table of the batch; a frame loop presents the same tiles again and again, so the upload is skipped when nothing changed
  if (tiles.size() != pix_xy_tiles.size() || std::memcmp(tiles.data(), pix_xy_tiles.data(), tiles.size() * sizeof(phx_tile)) != 0) {
    std::vector<uint32_t> xy(P);
    uint32_t k = 0;
    for (auto& t : tiles)
      for (uint32_t y = 0; y < t.h; ++y)
        for (uint32_t x = 0; x < t.w; ++x) xy[k++] = (t.x + x) | ((t.y + y) << 16);
    pix_xy_tiles.clear();
    if ((rc = pix_xy.upload(xy))) return rc;
    pix_xy_tiles = tiles;
  }
  if ((rc = acc.alloc((size_t)P * xs))) return rc;
  if (adaptive_on) {
    if ((rc = w_acc.alloc((size_t)P * xs)) || (rc = w_xy.alloc(P)) || (rc = sel_idx[0].alloc(P)) || (rc = sel_idx[1].alloc(P)) ||
        (rc = sel_blocks.alloc((P + PHX_ADAPTIVE_BLOCK - 1) / PHX_ADAPTIVE_BLOCK)))
      return rc;
    if ((rc = h_sel.alloc(1, hipHostMallocMapped | hipHostMallocCoherent))) return rc;
  }
  // queues + state; when the device cannot hold S samples per pixel in flight, back off to half as many (more, shorter passes)
  size_t npaths = 0;
  for (;;) {
    npaths = (size_t)P * S;
    if (!(rc = queues.alloc(npaths, normals, hit_uv))) break;
    if (rc != PHX_ERR_OOM || S == 1) return rc;
    (void)hipGetLastError();
    queues.release();
    budget_bytes = 0;  // the reading was stale: the next path_budget() — of this batch, of the next one, of the next frame — asks the device again
    S = plan_batch(P, (S + 1) / 2, passes);
  }
  paths_in_flight = npaths;
  tb_alloc = Clock::now();

  PassBuffers B{};
  queues.fill(B, normals, hit_uv);
  B.counters = counters.p; B.stats = dstats.p; B.pix_xy = pix_xy.p; B.jitter = jitter.p; B.acc = acc.p;
  B.num_pixels = P; B.xstride = xs; B.normals_offset = layout.normals_offset;
  B.seed = frame.sampler_seed;

  direct.events_used = 0; direct.timed.clear();
  if ((rc = enqueue_batch(direct, B, P, passes))) return rc;
  tb_enq = Clock::now();
  if (frame.add_tile || frame.host_film) {
    const size_t nfl = (size_t)P * xs;
    if ((rc = h_acc.alloc(nfl, hipHostMallocDefault))) return rc;
    HIPCHK(hipMemcpyAsync(h_acc.p, acc.p, nfl * sizeof(float), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    std::vector<size_t> offs(tiles.size() + 1, 0);
    for (size_t i = 0; i < tiles.size(); ++i) offs[i + 1] = offs[i] + (size_t)tiles[i].w * tiles[i].h * xs;
    if (frame.add_tile)
      for (size_t i = 0; i < tiles.size(); ++i) {
        const phx_tile& t = tiles[i];
        frame.add_tile(frame.film_user, (int32_t)t.x, (int32_t)t.y, (int32_t)t.w, (int32_t)t.h, h_acc.p + offs[i], xs, xs * t.w);
      }
    if (frame.host_film) {  // what an add_tile that copies into a frame buffer does, spread over a few host threads
      auto copy_range = [&](size_t i0, size_t i1) {
        for (size_t i = i0; i < i1; ++i) {
          const phx_tile& t = tiles[i];
          for (uint32_t y = 0; y < t.h; ++y)
            std::memcpy(frame.host_film + ((size_t)(t.y + y) * scene.width + t.x) * xs, h_acc.p + offs[i] + (size_t)y * t.w * xs, (size_t)t.w * xs * sizeof(float));
        }
      };
      const size_t nthreads = std::min<size_t>({8, std::max(1u, std::thread::hardware_concurrency() / 2), (nfl * sizeof(float)) >> 20});
      if (nthreads <= 1) copy_range(0, tiles.size());
      else {
        std::vector<std::thread> pool;
        for (size_t k = 0; k < nthreads; ++k) pool.emplace_back(copy_range, tiles.size() * k / nthreads, tiles.size() * (k + 1) / nthreads);
        for (auto& th : pool) th.join();
      }
    }
  } else {
    HIPCHK(hipStreamSynchronize(stream));
  }
  if (host_timing()) {
    auto ms = ms_between;
    std::fprintf(stderr, "batch of %u px x %u samples: tables + allocation %.3f ms, enqueue %.3f, wait + sink %.3f\n", P, S, ms(tb0, tb_alloc), ms(tb_alloc, tb_enq),
                 ms(tb_enq, Clock::now()));
  }
  // the batch is complete: its launches' HIP-event times (the next batch records the same events again)
  for (auto& te : direct.timed) {
    float ms = 0.0f;
    HIPCHK(hipEventElapsedTime(&ms, direct.events[te.begin], direct.events[te.end]));
    switch (te.kind) {
      case Launch::Trace: stats.closest_ms += ms; stats.trace_launches++; break;      // k_trace: closest + shadow rays in one launch
      case Launch::Primary: stats.primary_ms += ms; stats.primary_launches++; break;  // k_trace_primary: the camera rays of a pass
      case Launch::Shade: stats.shade_ms += ms; stats.shade_kernel_ms += ms; stats.shade_launches++; break;
      case Launch::Pass: stats.shade_ms += ms; break;  // begin-pass and film count as shading time
    }
  }
  return PHX_OK;
}

// The launches of one batch, in stream order.
int phx_device::enqueue_batch(BatchLaunches& g, const PassBuffers& B0, uint32_t P, const std::vector<Pass>& passes) {
  int rc;
  PassBuffers B = B0;
  const uint32_t spp = opt.samples_per_pixel, xs = layout.xstride;
  HIPCHK(hipMemsetAsync(acc.p, 0, (size_t)P * xs * sizeof(float), stream));
  const float inv = 1.0f / (float)(spp * opt.paths_per_sample);  // cpu.cpp:191
  // One event BETWEEN two launches serves as the end of the first and the start of the second (an event record is a packet of its own in
  // the queue: 42 of them per pass made the gaps between the 21 launches longer than the launches need).  A launch's time then includes
  // the few microseconds since the previous kernel ended.
  long last_end = -1;  // index of the event recorded behind the previous timed launch of this batch
  auto timed_launch = [&](Launch kind, auto&& fn) -> int {
    hipEvent_t e; int r;
    if (!kernel_timing) { fn(); return PHX_OK; }
    if (last_end < 0) { if ((r = next_event(g, &e))) return r; HIPCHK(hipEventRecord(e, stream)); last_end = (long)g.events_used - 1; }
    const size_t begin = (size_t)last_end;
    fn();
    if ((r = next_event(g, &e))) return r;
    HIPCHK(hipEventRecord(e, stream));
    last_end = (long)g.events_used - 1;
    g.timed.push_back({begin, (size_t)last_end, kind});
    return PHX_OK;
  };
  // Shade grids sized by the queue, not by its capacity.  k_shade runs one workgroup per 1024 entries and the host does not know the queue
  // lengths (they stay on the device): a grid for the capacity is 230 k workgroups at EVERY step of the bench frame, nearly all of them
  // empty from the third step on — 0.25 ms per launch for nothing.  k_trace of step b publishes the length of the queue it traces in pinned
  // host memory; the queue of a later step is never longer, so the shade launch of step b + 1 is sized by it.  The host waits for that word
  // before it enqueues the launch — while the device still has k_trace(b), k_shade(b) and k_trace(b + 1) in its queue: it never runs dry
  // (measured: k_shade 8.6 -> 7.5 ms on the bench frame, profiles/r06_v_grid_by_queue_ab.log).
  // (PHX_SHADE_GRID_BY_QUEUE=0: grids for the capacity, everything enqueued at once, as before.)
  static const bool grid_by_queue = [] { const char* v = std::getenv("PHX_SHADE_GRID_BY_QUEUE"); return !(v && v[0] == '0'); }();
  const uint32_t depth = opt.path_depth;
  if (grid_by_queue) {
    const size_t need = passes.size() * depth;  // (under adaptive sampling: of the passes a batch in which no pixel stops would take)
    if ((rc = h_qlen.alloc(need, hipHostMallocMapped | hipHostMallocCoherent))) return rc;
    for (size_t k = 0; k < need; ++k) __atomic_store_n(&h_qlen.p[k], 0xffffffffu, __ATOMIC_RELAXED);  // the previous batch has been joined (render_batch)
  }
  // length of the ray queue k_trace(step) of this pass traced, once it has started; a device that never says (device_word's 0xffffffff): the capacity
  auto queue_bound = [&](uint32_t pass, uint32_t step, uint32_t cap) -> uint32_t { return std::min(device_word(&h_qlen.p[(size_t)pass * depth + step]), cap); };
  // Adaptive sampling (phx_adaptive).  The first round runs on the batch's own tables.  Behind every round the selection decides
  // the pixels still active, in the batch buffer (their "home" rows); the rows that go on are gathered, in their order, into the working
  // tables, and the next round is the same kernels with B.pix_xy, B.acc and B.num_pixels naming those; behind it the rows go home again.
  uint32_t active = P;                // pixels the next pass carries
  const uint32_t* home_of = nullptr;   // their home rows (nullptr: the pass runs on the batch's own tables)
  int next_list = 0;
  for (uint32_t pass = 0; pass < (uint32_t)passes.size(); ++pass) {
    const uint32_t s0 = passes[pass].s0, ns = passes[pass].ns;
    const uint32_t cap = active * ns;
    B.num_samples = ns;
    B.qlen_out = nullptr;
    if ((rc = timed_launch(Launch::Pass, [&]() { launch_begin_pass(stream, B, ns); }))) return rc;
    int q = 0;
    for (uint32_t bounce = 0; bounce < opt.path_depth; ++bounce) {  // a path takes at most path_depth steps (spt.hpp:314)
      // step `bounce`: closest-hit rays of this step + the shadow rays k_shade produced in the previous step
      const int sq_read = (int)((bounce + 1) & 1), sq_write = (int)(bounce & 1);
      if (bounce == 0) {  // the camera rays: one packet walk per 64 x n of them
        if ((rc = timed_launch(Launch::Primary, [&]() { launch_trace_primary(stream, scene, B, cap, s0, q, sq_read); }))) return rc;
      } else {
        B.qlen_out = grid_by_queue ? h_qlen.p + (size_t)pass * depth + bounce : nullptr;
        if ((rc = timed_launch(Launch::Trace, [&]() { launch_trace(stream, scene, B, q, sq_read, 1, 1, cap); }))) return rc;
        B.qlen_out = nullptr;
      }
      // step 0: the capacity.  Step 1: the length k_trace(1) — the longest launch of a pass, enqueued just above — publishes as it starts.
      // Later steps: the length published one step earlier (the device then still has two launches queued while the host waits).
      const uint32_t shade_cap = (grid_by_queue && bounce >= 1) ? std::max(queue_bound(pass, bounce == 1 ? 1u : bounce - 1, cap), 1u) : cap;
      if ((rc = timed_launch(Launch::Shade, [&]() { stats.shade_kernels |= launch_shade(stream, scene, B, q, sq_write, shade_cap, s0, bounce == 0); }))) return rc;
      q ^= 1;
    }
    if ((rc = timed_launch(Launch::Trace, [&]() { launch_trace(stream, scene, B, q, (int)((opt.path_depth - 1) & 1), 0, 1, cap); }))) return rc;
    // the frame's error estimate (phx_frame.moments_channel) is made in the film's walk: k_film_moments INSTEAD of k_film, the channel behind the others
    if ((rc = timed_launch(Launch::Pass, [&]() {
           if (frame.moments_channel) launch_film_moments(stream, B, ns, inv, s0, layout.m2_offset);
           else launch_film(stream, B, ns, inv);
         })))
      return rc;
    HIPCHK(hipGetLastError());
    if (!passes[pass].round_end) continue;
    const uint32_t n = s0 + ns;  // samples every active pixel has taken
    uint32_t* const survivors = sel_idx[next_list].p;
    __atomic_store_n(h_sel.p, 0xffffffffu, __ATOMIC_RELEASE);  // (the previous round's count has been read, and nothing in the stream writes the word)
    if ((rc = timed_launch(Launch::Pass, [&]() {
           if (home_of) launch_adaptive_move(stream, acc.p, w_acc.p, pix_xy.p, w_xy.p, home_of, active, xs, 1);
           if (n == spp) { launch_adaptive_mark(stream, acc.p, xs, layout.samples_offset, home_of, active, (float)spp); return; }  // these took every sample: untouched
           AdaptiveArgs A{};
           A.acc = acc.p; A.xstride = xs; A.m2_offset = layout.m2_offset; A.samples_offset = layout.samples_offset; A.active = home_of; A.num_active = active;
           adaptive_args(adaptive, n, spp, A);
           launch_adaptive_select(stream, A, sel_blocks.p, survivors, h_sel.p);
         })))
      return rc;
    HIPCHK(hipGetLastError());
    if (n == spp) break;
    // How many go on: the host's one wait of a round (it sizes the next round's launches by the count).  k_adaptive_scan publishes the count in
    // pinned memory, as k_trace publishes its queue lengths, and the host reads it there without draining the stream; never for ever: after
    // two seconds the stream is synchronised, which reports a device that has stopped.
    uint32_t going_on = device_word(h_sel.p);
    if (going_on == 0xffffffffu) {
      HIPCHK(hipStreamSynchronize(stream));
      going_on = __atomic_load_n(h_sel.p, __ATOMIC_ACQUIRE);
    }
    if (going_on > active) return fail(PHX_ERR_DEVICE, "adaptive sampling: the selection reports more pixels than it was given");
    if (going_on == 0) break;  // every pixel of the batch has stopped: its remaining passes are not run
    launch_adaptive_move(stream, acc.p, w_acc.p, pix_xy.p, w_xy.p, survivors, going_on, xs, 0);
    HIPCHK(hipGetLastError());
    B.acc = w_acc.p; B.pix_xy = w_xy.p; B.num_pixels = active = going_on;
    home_of = survivors; next_list ^= 1;
  }
  // film_t<>::add_tile (film.hpp:12-15)
  if (frame.device_film) {
    B.acc = acc.p; B.pix_xy = pix_xy.p; B.num_pixels = P;  // the batch's own tables (they never were anything else without adaptive sampling)
    launch_scatter_film(stream, B, frame.device_film, scene.width);
    HIPCHK(hipGetLastError());
  }
  return PHX_OK;
}
