// frame_driver.cpp — the frame: the driver thread of a device (phx_dev_start hands it a frame, device.cpp), run_frame, which drains the shared
// tile queue in batches (reference src/xpu/cpu.cpp:223-238 pulls one tile at a time), render_batch, which sizes and allocates a batch's queues
// and hands its film to the sink (cpu.cpp:201), and enqueue_batch, the launches of a batch through the wavefront kernels of trace.hip,
// shade_lambert.hip, shade_general.hip and film_hooks.hip.
//
// What a frame decides without the device is frame_plan.cpp's (the film's pixel layout, the pixel cap, the batch cutter, the pass schedule); here
// are the allocations, the launches and the waits.  jitter_table and adaptive_args are the frame's too; the guide pass and the selection hook
// (film_calls.cpp) read them through device_internal.h.
#include "device_internal.h"

#include <cmath>
#include <cstdio>
#include <cstring>

using namespace phx;

namespace phx {

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

}  // namespace phx

namespace {

bool host_timing() {  // PHX_HOST_TIMING, read at the first frame: where a frame's and a batch's host time goes, on stderr (probe)
  static const bool on = std::getenv("PHX_HOST_TIMING") != nullptr;
  return on;
}

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
