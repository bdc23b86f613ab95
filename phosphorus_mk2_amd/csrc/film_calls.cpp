// film_calls.cpp — the entry points that work on a film and launch no frame: phx_dev_film_moments, phx_dev_denoise / _guided (denoise.hip),
// phx_dev_render_guides (guides.hip), phx_dev_film_accumulate (accumulate.hip), phx_dev_film_reproject (reproject.hip),
// phx_dev_film_outlier_clamp (outlier_clamp.hip), phx_dev_film_display (display.hip), phx_dev_film_tile_map (tile_map.hip),
// phx_dev_adaptive_select and the seven *_times getters.
//
// None of them reads a scene but the guide pass, which reads the camera and the tree.  Their argument checks are host-only (the *_check.cpp
// files over film_checks.h) and run before the device is selected.  What the large calls share is stated once below: the refusals (refused);
// device, events, host-film staging, the wait and the times (FilmCall); the summary's counters (SummarySlots, the host's side of film_pass.h);
// the times getters (times_of).  phx_dev_film_moments and phx_dev_adaptive_select stage plain arrays, as the stage hooks do (Staging).
#include "device_internal.h"
#include "accumulate_check.h"
#include "denoise_check.h"
#include "display_check.h"
#include "film_checks.h"
#include "guides_check.h"
#include "outlier_clamp_check.h"
#include "reproject_check.h"
#include "tile_map_check.h"

using namespace phx;

namespace {

// The refusals every film call opens with, in their order.  `args`: false when a pointer the call cannot do without is null.
int refused(const phx_device* d, const char* call, bool args, bool needs_scene = false) {
  auto no = [call](int code, const char* why) { return fail(code, std::string(call) + why); };  // (the text is built for a refusal only)
  if (!d) return no(PHX_ERR_ARG, ": null device");
  if (needs_scene && !d->preprocessed) return no(PHX_ERR_STATE, " before preprocess");
  if (d->running) return no(PHX_ERR_STATE, " while a frame is running");
  if (!args) return no(PHX_ERR_ARG, ": null argument");
  return PHX_OK;
}

// One film call on the device, behind its argument check: begin() enters the device and zeroes the call's times, stage() gives a host film a
// device copy, mark() records an event between launches, wait() waits and copies back, run() is both around one kernel, times() reads the events.  Everything it holds on the
// device goes with it, on every way out, and the caller's device comes back.
struct FilmCall {
  phx_device* d; double* ms;  // ms: the call's times in the device object
  Clock::time_point t0;
  std::optional<DeviceScope> on;
  std::deque<DevBuf<float>> staged;
  struct Back { float* host; const float* dev; size_t bytes; };
  std::vector<Back> back;
  std::vector<hipEvent_t> ev;
  ~FilmCall() { for (hipEvent_t x : ev) (void)hipEventDestroy(x); }

  int begin(size_t num_times) {  // (a refused call never comes here: it leaves the caller's device and the previous call's times alone)
    t0 = Clock::now();
    if (!on.emplace(d->hip_device).ok) return fail(PHX_ERR_DEVICE, "hipSetDevice failed");
    std::fill(ms, ms + num_times, 0.0);
    return PHX_OK;
  }
  // a host film of `floats` floats: `dev` becomes a device copy, filled from `from` (nullptr: left as allocated) and copied to `back_to` behind the wait (nullptr: not)
  int stage(const float* from, size_t floats, float* back_to, float*& dev) {
    staged.emplace_back();
    if (const int rc = staged.back().alloc(floats)) return rc;
    dev = staged.back().p;
    if (from) HIPCHK(hipMemcpy(dev, from, floats * sizeof(float), hipMemcpyHostToDevice));
    if (back_to) back.push_back({back_to, dev, floats * sizeof(float)});
    return PHX_OK;
  }
  int mark() {
    hipEvent_t x; HIPCHK(hipEventCreate(&x));
    ev.push_back(x);
    HIPCHK(hipEventRecord(x, d->stream));
    return PHX_OK;
  }
  int wait() {
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(d->stream));
    for (const Back& b : back) HIPCHK(hipMemcpy(b.host, b.dev, b.bytes, hipMemcpyDeviceToHost));
    return PHX_OK;
  }
  // behind wait(): the time between marks k and k + 1 into ms[slot(k)], the call's own since begin() into ms[call]
  template <typename F> int times(size_t call, F&& slot) {
    for (size_t k = 0; k + 1 < ev.size(); ++k) {
      float t = 0.0f;
      HIPCHK(hipEventElapsedTime(&t, ev[k], ev[k + 1]));
      ms[slot(k)] = t;
    }
    ms[call] = ms_between(t0, Clock::now());
    return PHX_OK;
  }
  // a call of one kernel: a mark on either side of the launch, then the wait
  template <typename F> int run(F&& launch) {
    if (const int rc = mark()) return rc;
    launch();
    if (const int rc = mark()) return rc;
    return wait();
  }
  int kernel_and_call_times() { return times(1, [](size_t) { return (size_t)0; }); }  // two marks: (kernel, call)
};

// The counters behind a summary (kernels.h: summary slots).  zero(): before the launch, only for a caller who asked for a summary (a kernel given
// p == nullptr counts nothing).  read(): behind FilmCall::wait(); out[k], k < n: the slots' k-th words summed, modulo 2^64 whatever the order.
struct SummarySlots : DevBuf<unsigned long long> {
  static constexpr size_t WORDS = (size_t)PHX_SUMMARY_SLOTS * PHX_SUMMARY_SLOT_WORDS;
  int zero(hipStream_t stream) {
    if (const int rc = alloc(WORDS)) return rc;
    HIPCHK(hipMemsetAsync(p, 0, WORDS * sizeof(unsigned long long), stream));
    return PHX_OK;
  }
  int read(uint64_t* out, int n) const {
    std::vector<unsigned long long> slots(WORDS);
    HIPCHK(hipMemcpy(slots.data(), p, WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    std::fill(out, out + n, (uint64_t)0);
    for (size_t s = 0; s < (size_t)PHX_SUMMARY_SLOTS; ++s) for (int k = 0; k < n; ++k) out[k] += slots[s * PHX_SUMMARY_SLOT_WORDS + k];
    return PHX_OK;
  }
};

// a *_times getter: `text` for a null argument, else a copy of the device object's array
template <size_t N> int times_of(const phx_device* d, double (phx_device::*ms)[N], double* out, const char* text) {
  if (!d || !out) return fail(PHX_ERR_ARG, text);
  std::copy(std::begin(d->*ms), std::end(d->*ms), out);
  return PHX_OK;
}

}  // namespace

extern "C" {

// (no stage_hook: the film stage reads no scene, so a device that has preprocessed nothing serves)
int phx_dev_film_moments(phx_device* d, uint32_t num_pixels, uint32_t num_samples, uint32_t samples_done, float inv, const float* radiance, float* acc) {
  return guarded([&]() -> int {
    if (const int rc = refused(d, "film_moments", true)) return rc;
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
    if (const int rc = refused(d, "denoise", q != nullptr)) return rc;
    std::string why;
    if (const int rc = denoise_check(*q, film_in, film_out, why)) return fail(rc, why);
    if (g && !g->flags) g = nullptr;
    if (g) if (const int rc = denoise_guides_check(*q, *g, why)) return fail(rc, why);
    FilmCall call{d, d->denoise_ms};
    if (const int rc = call.begin(11)) return rc;
    const size_t npix = (size_t)q->width * q->height, film_bytes = npix * q->xstride * sizeof(float);
    // the working buffers live in these and go with them, on every way out
    DevBuf<float4> c[2], v[2], n, gx; DevBuf<double> e[2];
    const float* src = film_in; float* dst = film_out;
    if (!q->on_device) {  // host films: one device copy, denoised in place
      if (const int rc = call.stage(film_in, npix * q->xstride, film_out, dst)) return rc;
      src = dst;
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
          float* copy = nullptr;
          if (const int rc = call.stage(g->guides, npix * g->xstride, nullptr, copy)) return rc;
          G.guides = copy;
        }
        if (g->flags & PHX_GUIDE_PLANE) { if (const int rc = gx.alloc(npix)) return rc; G.x = gx.p; }
      }
      DenoiseArgs A{};
      A.width = q->width; A.height = q->height; A.xstride = q->xstride; A.normals_offset = q->normals_offset; A.m2_offset = q->m2_offset;
      A.samples_offset = q->samples_offset; A.spp = q->spp; A.normal_power_log2 = q->normal_power_log2; A.sigma_l = (double)q->sigma_l;
      for (int k = 0; k < 2; ++k) { A.c[k] = c[k].p; A.v[k] = v[k].p; A.e[k] = e[k].p; }
      A.n = n.p;
      if (const int rc = call.mark()) return rc;
      if (g) launch_denoise_pack_guided(d->stream, A, G, src); else launch_denoise_pack(d->stream, A, src);
      if (const int rc = call.mark()) return rc;
      for (uint32_t i = 0; i < q->iterations; ++i) {
        if (g) launch_denoise_iteration_guided(d->stream, A, G, (int)(i & 1u), 1u << i); else launch_denoise_iteration(d->stream, A, (int)(i & 1u), 1u << i);
        if (const int rc = call.mark()) return rc;
      }
      if (dst != src) HIPCHK(hipMemcpyAsync(dst, src, film_bytes, hipMemcpyDeviceToDevice, d->stream));
      if (g) launch_denoise_unpack_guided(d->stream, A, G, (int)(q->iterations & 1u), dst); else launch_denoise_unpack(d->stream, A, (int)(q->iterations & 1u), dst);
      if (const int rc = call.mark()) return rc;
    } else if (dst != src) HIPCHK(hipMemcpyAsync(dst, src, film_bytes, hipMemcpyDeviceToDevice, d->stream));
    if (const int rc = call.wait()) return rc;
    // denoise_ms: 0 pack, 1 .. iterations the iterations, 9 unpack, 10 the call
    return call.times(10, [&](size_t k) -> size_t { return k == 0 ? 0 : k <= q->iterations ? k : 9; });
  });
}

// The first-hit guide film (phx_guides; guides.hip).
int phx_dev_render_guides(phx_device* d, const phx_guides* g, float* film) {
  return guarded([&]() -> int {
    if (const int rc = refused(d, "render_guides", g != nullptr, true)) return rc;
    const uint32_t W = d->scene.width, H = d->scene.height, spp = d->opt.samples_per_pixel;
    std::string why;
    if (const int rc = guides_check(*g, W, H, spp, film, why)) return fail(rc, why);
    FilmCall call{d, d->guides_ms};
    if (const int rc = call.begin(2)) return rc;
    const size_t npix = (size_t)W * H;
    std::vector<uint32_t> xy(npix);
    for (uint32_t y = 0; y < H; ++y) for (uint32_t x = 0; x < W; ++x) xy[(size_t)y * W + x] = x | y << 16;
    DevBuf<uint32_t> d_xy; DevBuf<float2> d_jit;
    if (const int rc = d_xy.upload(xy)) return rc;
    if (const int rc = d_jit.upload(jitter_table(g->sampler_seed, spp))) return rc;
    float* dst = film;
    if (!g->on_device) if (const int rc = call.stage(nullptr, npix * 8, film, dst)) return rc;
    PassBuffers B{};
    B.pix_xy = d_xy.p; B.jitter = d_jit.p; B.num_pixels = (uint32_t)npix; B.num_samples = g->samples; B.seed = g->sampler_seed;
    if (const int rc = call.run([&] { launch_guides(d->stream, d->scene, B, dst); })) return rc;
    return call.kernel_and_call_times();
  });
}

// Film accumulation (phx_accumulate; accumulate.hip).
// (no stage_hook: the call reads two films and no scene)
int phx_dev_film_accumulate(phx_device* d, const phx_accumulate* a, float* acc, const float* frame_film, phx_accumulate_summary* summary) {
  return guarded([&]() -> int {
    if (const int rc = refused(d, "accumulate", a != nullptr)) return rc;
    std::string why;
    if (const int rc = accumulate_check(*a, acc, frame_film, why)) return fail(rc, why);
    FilmCall call{d, d->accumulate_ms};
    if (const int rc = call.begin(2)) return rc;
    const size_t npix = (size_t)a->width * a->height;
    SummarySlots counters;
    float *dst = acc, *frame_copy = nullptr; const float* src = frame_film;
    if (!a->on_device) {  // host films: device copies, acc's pooled in place and copied back
      if (const int rc = call.stage(acc, npix * a->xstride_a, acc, dst)) return rc;
      if (const int rc = call.stage(frame_film, npix * a->xstride_b, nullptr, frame_copy)) return rc;
      src = frame_copy;
    }
    if (summary) if (const int rc = counters.zero(d->stream)) return rc;
    AccumulateArgs A{};
    A.num_pixels = npix;
    A.xstride_a = a->xstride_a; A.normals_offset_a = a->normals_offset_a; A.m2_offset_a = a->m2_offset_a; A.samples_offset_a = a->samples_offset_a;
    A.xstride_b = a->xstride_b; A.normals_offset_b = a->normals_offset_b; A.m2_offset_b = a->m2_offset_b; A.samples_offset_b = a->samples_offset_b;
    A.spp_b = a->spp_b; A.tau = (double)a->tau; A.floor = (double)a->floor;
    if (const int rc = call.run([&] { launch_accumulate(d->stream, A, dst, src, counters.p); })) return rc;
    if (summary) {
      uint64_t c[4];
      if (const int rc = counters.read(c, 4)) return rc;
      summary->pixels = c[0]; summary->invalid = c[1]; summary->converged = c[2]; summary->samples = c[3];
    }
    return call.kernel_and_call_times();
  });
}

int phx_dev_accumulate_times(const phx_device* d, double* ms) { return times_of(d, &phx_device::accumulate_ms, ms, "accumulate_times: null argument"); }

// The tile map (phx_tile_map; tile_map.hip).
// (no stage_hook: the call reads a film and no scene)
int phx_dev_film_tile_map(phx_device* d, const phx_tile_map* m, const float* acc, phx_tile_record* records, phx_tile_map_summary* summary) {
  return guarded([&]() -> int {
    if (const int rc = refused(d, "tile_map", m != nullptr)) return rc;
    std::string why;
    if (const int rc = tile_map_check(*m, acc, records, why)) return fail(rc, why);
    FilmCall call{d, d->tile_map_ms};
    if (const int rc = call.begin(2)) return rc;
    const size_t npix = (size_t)m->width * m->height;
    const uint32_t tiles_x = tile_map_tiles(m->width, m->tile_width), num_tiles = tiles_x * tile_map_tiles(m->height, m->tile_height);
    static_assert(sizeof(phx_tile_record) == 10 * sizeof(float), "a record is staged as ten 4-byte words");
    SummarySlots counters;
    const float* src = acc; phx_tile_record* dst = records;
    if (m->on_device == 0u) {  // a host film: a device copy
      float* copy = nullptr;
      if (const int rc = call.stage(acc, npix * m->xstride, nullptr, copy)) return rc;
      src = copy;
    }
    if (m->on_device != 1u) {  // host records: device records, copied back behind the wait
      float* words = nullptr;
      if (const int rc = call.stage(nullptr, (size_t)num_tiles * 10u, reinterpret_cast<float*>(records), words)) return rc;
      dst = reinterpret_cast<phx_tile_record*>(words);
    }
    if (summary) if (const int rc = counters.zero(d->stream)) return rc;
    TileMapArgs A{};
    A.width = m->width; A.height = m->height; A.xstride = m->xstride; A.m2_offset = m->m2_offset; A.samples_offset = m->samples_offset;
    A.tile_width = m->tile_width; A.tile_height = m->tile_height; A.tiles_x = tiles_x; A.tau = (double)m->tau; A.floor = (double)m->floor;
    if (const int rc = call.run([&] { launch_tile_map(d->stream, A, num_tiles, src, dst, counters.p); })) return rc;
    if (summary) {
      uint64_t c[6];
      if (const int rc = counters.read(c, 6)) return rc;
      summary->pixels = c[0]; summary->invalid = c[1]; summary->converged = c[2]; summary->samples = c[3]; summary->tiles = c[4]; summary->open = c[5];
    }
    return call.kernel_and_call_times();
  });
}

int phx_dev_tile_map_times(const phx_device* d, double* ms) { return times_of(d, &phx_device::tile_map_ms, ms, "tile_map_times: null argument"); }

// Reprojection (phx_reproject; reproject.hip).
// (no stage_hook: the call reads four films and two cameras of its own, and no scene)
int phx_dev_film_reproject(phx_device* d, const phx_reproject* r, const float* acc_from, const float* guides_from, const float* guides_to, float* acc_to,
                           phx_reproject_summary* summary) {
  return guarded([&]() -> int {
    if (const int rc = refused(d, "reproject", r != nullptr)) return rc;
    std::string why;
    ReprojectArgs A{};
    if (const int rc = reproject_check(*r, acc_from, guides_from, guides_to, acc_to, A.from, A.to, why)) return fail(rc, why);
    FilmCall call{d, d->reproject_ms};
    if (const int rc = call.begin(2)) return rc;
    const size_t npix = (size_t)r->width * r->height;
    SummarySlots counters;
    const float *src = acc_from, *gf = guides_from, *gt = guides_to; float* dst = acc_to;
    if (!r->on_device) {  // host films: device copies of the three inputs, and acc_to's copied back behind the wait
      float *c0 = nullptr, *c1 = nullptr, *c2 = nullptr;
      if (const int rc = call.stage(acc_from, npix * r->xstride_a, nullptr, c0)) return rc;
      if (const int rc = call.stage(guides_from, npix * r->xstride_g, nullptr, c1)) return rc;
      if (const int rc = call.stage(guides_to, npix * r->xstride_g, nullptr, c2)) return rc;
      if (const int rc = call.stage(nullptr, npix * r->xstride_a, acc_to, dst)) return rc;
      src = c0; gf = c1; gt = c2;
    }
    if (summary) if (const int rc = counters.zero(d->stream)) return rc;
    A.num_pixels = npix; A.width = r->width; A.height = r->height;
    A.xstride_a = r->xstride_a; A.normals_offset_a = r->normals_offset_a; A.m2_offset_a = r->m2_offset_a; A.samples_offset_a = r->samples_offset_a;
    A.xstride_g = r->xstride_g;
    A.sigma_plane = (double)r->sigma_plane; A.sigma_dist = (double)r->sigma_dist; A.max_history = (double)r->max_history;
    if (const int rc = call.run([&] { launch_reproject(d->stream, A, src, gf, gt, dst, counters.p); })) return rc;
    if (summary) {
      uint64_t c[5];
      if (const int rc = counters.read(c, 5)) return rc;
      summary->pixels = c[0]; summary->reused = c[1]; summary->no_geometry = c[2]; summary->disoccluded = c[3]; summary->samples = c[4];
    }
    return call.kernel_and_call_times();
  });
}

int phx_dev_reproject_times(const phx_device* d, double* ms) { return times_of(d, &phx_device::reproject_ms, ms, "reproject_times: null argument"); }

// The outlier clamp (phx_outlier_clamp; outlier_clamp.hip).
// (no stage_hook: the call reads two films and no scene)
int phx_dev_film_outlier_clamp(phx_device* d, const phx_outlier_clamp* c, const float* film, const float* ref, float* film_out, phx_outlier_clamp_summary* summary) {
  return guarded([&]() -> int {
    if (const int rc = refused(d, "outlier_clamp", c != nullptr)) return rc;
    std::string why;
    bool ref_needs_copy = false;
    if (const int rc = outlier_clamp_check(*c, film, ref, film_out, ref_needs_copy, why)) return fail(rc, why);
    FilmCall call{d, d->outlier_clamp_ms};
    if (const int rc = call.begin(2)) return rc;
    const size_t npix = (size_t)c->width * c->height, floats_b = npix * c->xstride_b;
    SummarySlots counters; DevBuf<float> ref_copy;
    const float *src = film, *bounds = ref; float* dst = film_out;
    if (!c->on_device) {  // host films: a device copy of film, clamped in place and copied back to film_out, and one of ref
      float* copy = nullptr;
      if (const int rc = call.stage(film, npix * c->xstride_a, film_out, dst)) return rc;
      if (const int rc = call.stage(ref, floats_b, nullptr, copy)) return rc;
      src = dst; bounds = copy;
    } else if (ref_needs_copy) {  // film_out is ref: the bounds come from ref as it was
      if (const int rc = ref_copy.alloc(floats_b)) return rc;
      HIPCHK(hipMemcpyAsync(ref_copy.p, ref, floats_b * sizeof(float), hipMemcpyDeviceToDevice, d->stream));
      bounds = ref_copy.p;
    }
    if (summary) if (const int rc = counters.zero(d->stream)) return rc;
    OutlierClampArgs A{};
    A.width = c->width; A.height = c->height; A.xstride_a = c->xstride_a; A.m2_offset_a = c->m2_offset_a; A.samples_offset_a = c->samples_offset_a;
    A.xstride_b = c->xstride_b; A.flags = c->flags; A.radius = c->radius; A.trim = c->trim; A.min_taps = c->min_taps;
    A.a_is_b = ref == film ? 1u : 0u;  // (the check: then of one stride; a copy of ref holds what film holds)
    A.gamma = (double)c->gamma; A.floor = (double)c->floor; A.clamped_history = (double)c->clamped_history;
    if (const int rc = call.run([&] { launch_outlier_clamp(d->stream, A, src, bounds, dst, counters.p); })) return rc;
    if (summary) {
      uint64_t s[6];
      if (const int rc = counters.read(s, 6)) return rc;
      summary->pixels = s[0]; summary->skipped = s[1]; summary->unbounded = s[2]; summary->inside = s[3]; summary->clamped = s[4]; summary->capped = s[5];
    }
    return call.kernel_and_call_times();
  });
}

int phx_dev_outlier_clamp_times(const phx_device* d, double* ms) { return times_of(d, &phx_device::outlier_clamp_ms, ms, "outlier_clamp_times: null argument"); }

// The display pass (phx_display; display.hip).
// (no stage_hook: the call reads a film and no scene)
int phx_dev_film_display(phx_device* d, const phx_display* p, const float* film, uint8_t* image, phx_display_summary* summary, uint64_t* histogram) {
  return guarded([&]() -> int {
    if (const int rc = refused(d, "display", p != nullptr)) return rc;
    std::string why;
    if (const int rc = display_check(*p, film, image, why)) return fail(rc, why);
    FilmCall call{d, d->display_ms};
    if (const int rc = call.begin(3)) return rc;
    const size_t npix = (size_t)p->width * p->height;
    const bool counts = (p->flags & PHX_DISPLAY_AUTO_EXPOSURE) || summary || histogram;
    const float* src = film; uint32_t* dst = reinterpret_cast<uint32_t*>(image);
    DisplayArgs A{};
    A.num_pixels = npix; A.width = p->width; A.xstride = p->xstride; A.pitch_words = (uint32_t)(display_pitch(*p) / 4u); A.flags = p->flags; A.tone = p->tone;
    A.scale = p->scale; A.white = p->white; A.key = p->key; A.min_scale = p->min_scale; A.max_scale = p->max_scale; A.low_q16 = p->low_q16; A.high_q16 = p->high_q16;
    if (p->on_device == 0u) {  // a host film: a device copy
      float* copy = nullptr;
      if (const int rc = call.stage(film, npix * p->xstride, nullptr, copy)) return rc;
      src = copy;
    }
    if (p->on_device != 1u) {  // a host image: a device image of 4 * width bytes a row, copied back row by row behind the wait
      float* words = nullptr;
      if (const int rc = call.stage(nullptr, npix, nullptr, words)) return rc;
      dst = reinterpret_cast<uint32_t*>(words); A.pitch_words = p->width;
    }
    DevBuf<unsigned long long> slots; DevBuf<DisplayBlock> block;
    int num_cus = 0;
    if (counts) {
      const size_t slot_words = (size_t)PHX_DISPLAY_SLOTS * PHX_DISPLAY_SLOT_WORDS;
      if (const int rc = slots.alloc(slot_words)) return rc;
      if (const int rc = block.alloc(1)) return rc;
      HIPCHK(hipMemsetAsync(slots.p, 0, slot_words * sizeof(unsigned long long), d->stream));
      HIPCHK(hipDeviceGetAttribute(&num_cus, hipDeviceAttributeMultiprocessorCount, d->hip_device));
    }
    if (const int rc = call.mark()) return rc;
    if (counts) launch_display_histogram(d->stream, A, (uint32_t)std::max(num_cus, 1), src, slots.p, block.p);
    if (const int rc = call.mark()) return rc;
    launch_display_encode(d->stream, A, src, block.p, dst);
    if (const int rc = call.mark()) return rc;
    if (const int rc = call.wait()) return rc;
    if (p->on_device != 1u) HIPCHK(hipMemcpy2D(image, display_pitch(*p), dst, 4ull * p->width, 4ull * p->width, p->height, hipMemcpyDeviceToHost));
    if (summary || histogram) {
      DisplayBlock b;
      HIPCHK(hipMemcpy(&b, block.p, sizeof b, hipMemcpyDeviceToHost));
      if (histogram) std::copy(b.histogram, b.histogram + 256, histogram);
      if (summary) { summary->pixels = b.pixels; summary->invalid = b.invalid; summary->unlit = b.unlit; summary->counted = b.counted; summary->scale = b.scale; summary->from_histogram = b.from_histogram; }
    }
    return call.times(2, [](size_t k) { return k; });  // display_ms: 0 histogram + exposure, 1 encode, 2 the call
  });
}

int phx_dev_display_times(const phx_device* d, double* ms) { return times_of(d, &phx_device::display_ms, ms, "display_times: null argument"); }
int phx_dev_guides_times(const phx_device* d, double* ms) { return times_of(d, &phx_device::guides_ms, ms, "guides_times: null argument"); }
int phx_dev_denoise_times(const phx_device* d, double* ms) { return times_of(d, &phx_device::denoise_ms, ms, "denoise_times: null argument"); }

// (no stage_hook either: the selection reads no scene)
int phx_dev_adaptive_select(phx_device* d, uint32_t num_active, const uint32_t* active, uint32_t num_rows, float* acc, uint32_t samples_done, uint32_t spp,
                            const phx_adaptive* a, uint32_t* survivors, uint32_t* num_survivors) {
  return guarded([&]() -> int {
    if (const int rc = refused(d, "adaptive_select", acc && a && survivors && num_survivors)) return rc;
    if (samples_done < 2u || samples_done >= spp) return fail(PHX_ERR_ARG, "adaptive_select: samples_done must be at least 2 and below spp");
    if (const char* field = adaptive_invalid(*a)) return fail(PHX_ERR_ARG, outside_its_range("adaptive_select", field, "phx_adaptive"));
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

}  // extern "C"
