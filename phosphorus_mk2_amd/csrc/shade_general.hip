// shade_general.hip — the shade kernel of scenes with closures other than Lambert lobes, its append ring, and launch_shade (see
// kernels.h for the HBM layout and the map of kernels to files).  One path per lane, 64-lane wavefronts.
//
//   k_shade_g   deferred_shading_kernel_t (reference src/kernels/cpu/deferred_shading_kernel.hpp:20-72) + light_sampler_t
//               (spt.hpp:95-149) + integrator_t (spt.hpp:161-328) fused, the hits of a workgroup's window sorted by material;
//               survivors and shadow rays leave through a workgroup-local ring in LDS (one global atomic per 256 entries)
// The 30 instantiations of k_shade_g are most of the library's device code and of its compile time: nothing else lives here.
#include "shade_common.h"
#include "shade_launch.h"

namespace phx {

#ifndef PHX_SHADE_BLOCK_G
#define PHX_SHADE_BLOCK_G 512  /* general k_shade (measured on the 16-recipe stand-in: 256: +4 % shade time, 128: +29 %, 64: +144 % — one atomic per workgroup and append) */
#endif
#ifndef PHX_SHADE_WAVES_G
#define PHX_SHADE_WAVES_G 4    /* general k_shade: waves per SIMD the register allocator must leave room for */
#endif

// ---- general closures: shade + NEE + integrate with the hits of a workgroup sorted by material ----------------------------------
// k_shade_g replaces the round-2 k_shade<0/3> (128 VGPRs, 160-700 B of scratch per lane, 4 waves per SIMD: the weakest kernel of the
// repo).  What changed, and why:
//   * no per-hit copy of the material.  A glass hit used to resolve its closure weights into a private 576-byte DevMaterial (scratch
//     memory, and every material read a flat load); now bsdf_f / bsdf_sample resolve a lobe's weight where they use it (bsdf.h).
//   * the two halves of a step (light_sampler_t and integrator_t, spt.hpp:95-149 / 161-328) share the hit's tangent frame, built once.
//     (For most of round 3 the NEE ray was appended to its queue BEFORE roulette and BSDF sampling started, so that its ten registers
//     were dead by then; once the kernel stood at 4 waves per SIMD whatever it did, one append for both queues per round won.)
//   * a workgroup sorts a WINDOW of BLOCK x ITEMS hits by material, not BLOCK: with 16 recipes assigned round-robin a 512-hit
//     bucket sort left 2-3 materials in every wave; a window of 4096 leaves most waves with one (deferred_shading_kernel_t buckets
//     a 1024-slot stream per material for the same reason, deferred_shading_kernel.hpp:9-33, 63).
//   * a fixed grid walks the queue (see k_shade).
#ifndef PHX_SHADE_ITEMS_G
#define PHX_SHADE_ITEMS_G 8
#endif
#define PHX_SHADE_BUCKETS 64  /* sort key = material mod 64; then the misses; slots past the end of the queue go last */
// probe builds (-DPHX_SHADE_TIMING=1, scripts/shade_phase_probe.py): s_memtime at the phase boundaries of a shading round, per wave.
// PHX_PHASE(n) closes phase n: everything the wave has in flight is waited for first, so that a phase is charged the latency of what it
// asked for (loads issued in a phase and consumed later would otherwise be billed to the consumer).
#ifndef PHX_SHADE_TIMING
#define PHX_SHADE_TIMING 0  /* 1: the ticks are summed into DevStats fields the count build uses */
#endif
#if PHX_SHADE_TIMING
#define PHX_PHASE_DECL long long ph_t = clock64(); unsigned long long ph_acc[6] = {0, 0, 0, 0, 0, 0};
#define PHX_PHASE(n) { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); const long long now_ = clock64(); ph_acc[n] += (unsigned long long)(now_ - ph_t); ph_t = now_; }
#else
#define PHX_PHASE_DECL
#define PHX_PHASE(n)
#endif
// The lanes that reach a closure evaluation, one distinct material of the wave at a time (after the window's sort by material most
// waves hold one): the material's index is made wave-uniform (v_readlane), its recipe is addressed in the CONSTANT address space, and
// every read with a uniform address — the lobe loops of bsdf_f and bsdf_sample — becomes an s_load into SGPRs instead of a
// vector load into 64 copies (round 3 made the address uniform without the address space: the compiler cannot prove the table is
// read-only then and keeps the vector loads; profiles/r03_v_unimat_ab.log).  `body` runs under `mine`; `cm` is the ConstMat&.
#define PHX_FOR_EACH_MATERIAL_OF_THE_WAVE(mat, cm, body)                                                                      \
  for (unsigned long long todo_ = __ballot(true); todo_ != 0ull;) {                                                           \
    uint32_t m0_ = (uint32_t)__builtin_amdgcn_readlane((int)(mat), (int)(__ffsll((long long)todo_) - 1));                     \
    const bool mine_ = (mat) == m0_;                                                                                          \
    /* inside `mine_` the optimiser knows mat == m0_ and would address the table with the per-lane register: hide the SGPR */ \
    asm volatile("" : "+s"(m0_));                                                                                             \
    if (mine_) { ConstMat& cm = *((ConstMat*)(sc.materials) + m0_); body; }                                                    \
    todo_ &= ~__ballot(mine_);                                                                                                \
  }
// ---- k_shade_g's append: a workgroup-local ring in LDS, no barrier and no global atomic inside a shading round -------------------------
// Until round 5 every round of 512 entries ended in block_append2: barrier, the workgroup's two atomics on the queue counters, barrier —
// 24 % of a wave's time (profiles/r05_c_shade_phases.md: the atomics' round trip ~2 200 clocks, ~5 000 waiting for the slowest of the eight
// waves, every round).  Now a WAVE reserves its slots in a ring of 2 x PHX_RING_BLK entries with one ds_add_rtn, writes its records there and
// adds its count to the block's commit counter; the wave whose commit completes a block of PHX_RING_BLK entries flushes it: ONE global
// atomic for exactly PHX_RING_BLK slots and coalesced 16-byte stores.  A block is written again only after its flush (`flushed`, per
// buffer), which the writers of the block after next wait for — they wait for waves with LOWER ring positions only, so there is no cycle —
// and what is left in the ring when the workgroup has shaded its last window goes out with an exact count.  The queues stay dense; their
// ORDER changes (blocks of 256 in completion order), which no result depends on (one closest-hit ray and at most one shadow ray per path
// and step; the film add is per path).  LDS: 16 KB (survivors, 32 B) + 24 KB (NEE rays, 48 B) per workgroup, two workgroups per CU.
// Ordering: the LDS executes the DS instructions of one wave in issue order, so "records, then commit" and "reads, then release" need no
// fence in hardware; s_waitcnt lgkmcnt(0) + a compiler barrier keep the compiler (and any doubt) out.  NOT __builtin_amdgcn_fence: a
// workgroup-scope fence also waits for the wave's global loads — the next round's records, requested right before the append.
#ifndef PHX_RING_BLK
#define PHX_RING_BLK 256u  /* entries per flush = per global atomic (the counters sustain ~80 returning atomics per us and address: 256 keeps the kernel near 50) */
#endif
#ifndef PHX_RING_SPINS
#define PHX_RING_SPINS (1u << 19)
#endif
struct RingCtl { uint32_t head, committed[2], flushed[2], dead; };  // dead: a wait of this workgroup timed out — its later appends are dropped, the frame fails
#define PHX_LDS_ORDER() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")
template <int NREC>
__device__ __forceinline__ void ring_flush(const float4* ring /* [NREC][2 x BLK] */, uint32_t first, uint32_t n, uint32_t* gcounter, float4* g0, float4* g1, float4* g2) {
  const uint32_t lane = __lane_id();
  uint32_t gb = 0;
  if (lane == 0) gb = atomicAdd(gcounter, n);
  gb = PHX_UNI(gb);
  for (uint32_t k = lane; k < n; k += 64u) {
    g0[gb + k] = ring[first + k];
    g1[gb + k] = ring[2u * PHX_RING_BLK + first + k];
    if (NREC == 3) g2[gb + k] = ring[4u * PHX_RING_BLK + first + k];
  }
}
// The two queues are appended ONE AFTER THE OTHER, each completely (reserve, records, commit, flush if this wave completed a block) before the
// next begins.  Interleaving them — both reservations, then both waits, both sets of records, both commits: three LDS round trips instead of
// six — was built in round 6 and DEADLOCKED on the closed showroom: a wave then holds an uncommitted reservation in one ring while it waits
// for a block of the other, and the two rings do not order the waves alike — inside a burst of eight waves (512 entries = the whole ring)
// wave 1 can be ahead of wave 3 in ring A and behind it in ring B, each waiting for the block the other has not committed (state dumped at
// the time-out: profiles/r06_g_ring_merged_deadlock.log).  One ring at a time, a wave waits only for LOWER positions of the SAME ring and
// holds nothing else: a total order, no cycle.
template <int NREC>
__device__ __forceinline__ void ring_append(bool want, const float4& r0, const float4& r1, const float4& r2, RingCtl* ctl, float4* ring,
                                            uint32_t* gcounter, float4* g0, float4* g1, float4* g2, unsigned long long* watchdog) {
  constexpr uint32_t BLK = PHX_RING_BLK;
  static_assert((BLK & (BLK - 1u)) == 0u && BLK >= 64u, "a wave's reservation spans at most two blocks");
  const unsigned long long mask = __ballot(want);
  if (mask == 0ull) return;  // wave-uniform
  const uint32_t lane = __lane_id(), n = (uint32_t)__popcll(mask);
  uint32_t pos = 0;
  if (lane == 0) pos = __hip_atomic_fetch_add(&ctl->head, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  pos = PHX_UNI(pos);
  const uint32_t gen0 = pos / BLK, gen1 = (pos + n - 1u) / BLK;  // generation g lives in buffer g & 1; it is that buffer's (g >> 1)-th use
  // (a wait is rare: the block after next fills a whole round later than this one's flush starts.  Every wait is bounded — PHX_RING_SPINS
  // sleeps of 64 clocks, ~30 ms — after which the wave counts itself in DevStats::watchdog and goes on: the frame is then reported as failed
  // (device.cpp), exactly as for k_trace's watchdog; no wave can spin for ever.)
  uint32_t spins = 0;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const uint32_t gen = h ? gen1 : gen0;
    if (h && gen1 == gen0) break;
    while (PHX_UNI(__hip_atomic_load(&ctl->flushed[gen & 1u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) < (gen >> 1)) {
      if (++spins > PHX_RING_SPINS || PHX_UNI(__hip_atomic_load(&ctl->dead, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP))) {
        if (lane == 0) { atomicAdd(watchdog, 1ull); __hip_atomic_store(&ctl->dead, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
        return;
      }
      __builtin_amdgcn_s_sleep(1);
    }
  }
  asm volatile("" ::: "memory");
  if (want) {
    const uint32_t idx = (pos + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))) & (2u * BLK - 1u);
    ring[idx] = r0; ring[2u * BLK + idx] = r1;
    if (NREC == 3) ring[4u * BLK + idx] = r2;
  }
  PHX_LDS_ORDER();  // the records are in LDS before the commit
  const uint32_t n0 = min(n, (gen0 + 1u) * BLK - pos), n1 = n - n0;
  uint32_t c0 = 0, c1 = 0;
  if (lane == 0) {
    c0 = __hip_atomic_fetch_add(&ctl->committed[gen0 & 1u], n0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (n1) c1 = __hip_atomic_fetch_add(&ctl->committed[gen1 & 1u], n1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  c0 = PHX_UNI(c0); c1 = PHX_UNI(c1);
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const uint32_t gen = h ? gen1 : gen0;
    if (h ? (n1 != 0u && c1 + n1 == BLK) : (c0 + n0 == BLK)) {  // this wave's commit completed the block: it flushes it
      asm volatile("" ::: "memory");
      ring_flush<NREC>(ring, (gen & 1u) * BLK, BLK, gcounter, g0, g1, g2);
      PHX_LDS_ORDER();  // the block has been read before it is handed back
      if (lane == 0) {
        __hip_atomic_store(&ctl->committed[gen & 1u], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        PHX_LDS_ORDER();
        __hip_atomic_fetch_add(&ctl->flushed[gen & 1u], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
    }
  }
}
template <bool PERHIT /* some material's closure weights depend on the hit (glass) */, bool FIRST, bool LENS = false /* FIRST: thin-lens camera */,
          bool TEX = false /* some lobe's weight is multiplied by an image texel (DevScene::any_tex & SC_TEX_LOBES) */,
          bool ENV = false /* the environment has an image: a miss reads it in the ray's direction (DevScene::any_tex & SC_TEX_ENV) */,
          bool MASK = false /* some lobe's mix factor is the luminance of an image texel (DevScene::any_tex & SC_TEX_MASK; with PERHIT and TEX) */>
__global__ void __launch_bounds__(PHX_SHADE_BLOCK_G) __attribute__((amdgpu_waves_per_eu(PHX_SHADE_WAVES_G, 8))) k_shade_g(DevScene sc, PassBuffers pb, int q, int sq, uint32_t sample0) {
  constexpr int BLOCK = PHX_SHADE_BLOCK_G, ITEMS = PHX_SHADE_ITEMS_G, WINDOW = BLOCK * ITEMS, NB = PHX_SHADE_BUCKETS;
  static_assert(WINDOW <= 65536 && BLOCK >= NB + 2 && NB == 64, "perm holds 16-bit positions; one wave scans the NB material buckets");
  __shared__ float4 ring_a[3 * 2 * PHX_RING_BLK];  // survivors: (o, path | SPECULAR << 31), (d, RNG key), (beta, depth)
  __shared__ float4 ring_b[3 * 2 * PHX_RING_BLK];  // NEE rays: (o, path), (d, tmax), (beta * Li)
  __shared__ RingCtl ring_ctl[2];
  // a wave takes the next 64 sorted slots of the window from this counter, not slots [k x BLOCK + 64 w, + 64) of a round k: nothing orders the
  // waves inside a window since the ring append, so the fast ones take more
  __shared__ uint32_t slice_next;
  if (threadIdx.x < sizeof(ring_ctl) / 4u) reinterpret_cast<uint32_t*>(ring_ctl)[threadIdx.x] = 0u;  // visible after the first barrier every thread reaches
  __shared__ uint32_t bucket[NB + 2];  // [material mod NB], [NB] misses, [NB + 1] slots past the end of the queue
  __shared__ uint16_t perm[WINDOW];
  if (pb.stats->watchdog | pb.stats->ring_watchdog) return;  // (k_shade above: a step whose trace did not finish is not shaded; the frame fails)
  // the hit's pool index (0xffffffff = miss) at its sorted position, kept beside the permutation (16 KB of LDS): a round requests the hit triangle's
  // shade record, vertex normals and corner UVs WITH the hit record and the ray instead of after the hit record has landed
  __shared__ uint32_t tri_sorted[WINDOW];
  const uint32_t count = pb.counters[q * CNT_STRIDE];
  if (blockIdx.x == 0 && threadIdx.x == 0) zero_cursors(pb.counters);  // the next k_trace pulls its chunks from here
  DevTexScene tx{};  // TEX / ENV: the scene's texture tables, pointers in SGPRs (constant address space: s_load)
  if constexpr (TEX || ENV) {
    const __attribute__((address_space(4))) DevTexScene* ctx = (const __attribute__((address_space(4))) DevTexScene*)sc.tex;
    if constexpr (TEX) { tx.elem_uv = ctx->elem_uv; tx.textures = ctx->textures; tx.texels = ctx->texels; tx.lobe_tex = ctx->lobe_tex; tx.any_emit_tex = ctx->any_emit_tex; }
    else { tx.textures = ctx->textures; tx.texels = ctx->texels; }
    if constexpr (ENV) { tx.env_tex = ctx->env_tex; tx.env_mapping = ctx->env_mapping; }
  }
  PHX_PHASE_DECL
#if PHX_SHADE_TIMING
  unsigned long long ph_rounds = 0, ph_windows = 0;
#endif
  // The sort keys of a window: two dependent gathers per hit — the hit record's triangle, that triangle's material.  (Fetching them one
  // window AHEAD — the triangles while the last round of the previous window waits in its append, the materials right after it, parked in
  // 4 KB of LDS — changed nothing: 34.6-35.1 ms either way, profiles/r05_c_shade_prefetch3_ab.log.)  0xfffffffe = slot past the end of the queue.
  auto request_tris = [&](uint32_t b, uint32_t (&tri)[ITEMS]) {
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
      const uint32_t i = b + k * BLOCK + threadIdx.x;
      tri[k] = i < count ? pb.hit_tt[i].y : 0xfffffffeu;  // 4 B at an 8-B stride (a 16-B stride until the hit record was split: every sector came in for a quarter of its bytes)
    }
  };
  auto request_keys = [&](const uint32_t (&tri)[ITEMS], uint32_t (&key)[ITEMS]) {
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
      key[k] = tri[k] == 0xfffffffeu ? NB + 1u : tri[k] != 0xffffffffu ? (f2u(sc.elem_shade[tri[k]].w) & (NB - 1u)) : (uint32_t)NB;  // the material word of the 16-byte shade record (four to a sector; the shading rounds read the same records)
    }
  };
  for (uint32_t base = blockIdx.x * WINDOW; base < count; base += gridDim.x * WINDOW) {
    PHX_PHASE(5)  // (the barrier at the end of the previous window, loop overhead)
    // ---- counting sort of the window by material, through LDS
    if (threadIdx.x < NB + 2) bucket[threadIdx.x] = 0;
    if (threadIdx.x == 0) slice_next = 0u;
    __syncthreads();
    uint32_t keys[ITEMS], tri_[ITEMS];
    request_tris(base, tri_);
    if constexpr (FIRST) {
      // the camera entries: queue order IS pixel order (a wave = 64 samples of one pixel: one material, a few on a silhouette) — no sort, the
      // identity permutation; the slots past the end of the queue are the window's last ones as they are after a sort
#pragma unroll
      for (int k = 0; k < ITEMS; ++k) tri_sorted[k * BLOCK + threadIdx.x] = tri_[k];
#pragma unroll
      for (int k = 0; k < ITEMS; ++k) perm[k * BLOCK + threadIdx.x] = (uint16_t)(k * BLOCK + threadIdx.x);
    } else {
    request_keys(tri_, keys);
    uint32_t ranks[ITEMS];
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) ranks[k] = atomicAdd(&bucket[keys[k]], 1u);
    __syncthreads();
    if (threadIdx.x < 64) {  // exclusive scan of the bucket counts by one wave
      const uint32_t c = bucket[threadIdx.x];
      uint32_t incl = c;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) { const uint32_t up = __shfl_up(incl, d); if ((int)threadIdx.x >= d) incl += up; }
      bucket[threadIdx.x] = incl - c;
      if (threadIdx.x == 63) { const uint32_t misses = bucket[NB]; bucket[NB] = incl; bucket[NB + 1] = incl + misses; }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
      const uint32_t at = bucket[keys[k]] + ranks[k];
      perm[at] = (uint16_t)(k * BLOCK + threadIdx.x);
      tri_sorted[at] = tri_[k];
    }
    }
    __syncthreads();
    PHX_PHASE(0)  // the window's sort by material
#if PHX_SHADE_TIMING
    ++ph_windows;
#endif
    // ---- the window in sorted order, in slices of 64 sorted slots handed out by an LDS counter; the live slots are a prefix of the sorted
    // window, so are the live slices (the slots past the end of the queue sort behind every live one)
    // The records of the NEXT slice — hit, ray, shade record — are REQUESTED right before this one's append: the phase probe of round 5
    // (profiles/r05_c_shade_phases.md) found a wave waiting 27 % of its time for exactly these loads and 24 % in the append; at the append a
    // thread holds almost nothing but its outputs, so the registers of the next records cost no occupancy there, and the two waits overlap.
    // (Round 3 requested them at the START of a round and held them across the closure code: 5-12 VGPRs where the kernel has none to spare,
    // 1.2 of 42.7 ms: profiles/r03_q_prefetch_ab.log.)
    uint32_t next_i = 0, next_tri = 0xffffffffu; bool next_live = false;
    // the hit's barycentrics are read where something consumes them: the corner UVs' interpolation (TEX) and a smooth face's normal
    const bool want_uv = TEX || sc.elem_normals != nullptr;  // wave-uniform; either one makes the scene's hit_uv stream exist (scene_commit.cpp)
    float next_t = 0.f; float2 next_uv = make_float2(0.f, 0.f);
    float4 next_a = make_float4(0.f, 0.f, 0.f, 0.f), next_b = next_a, next_S = next_a;
    const uint32_t nslices = (min((uint32_t)WINDOW, count - base) + 63u) >> 6;
    auto take_slice = [&]() -> uint32_t {
      uint32_t s_ = 0;
      if (__lane_id() == 0) s_ = __hip_atomic_fetch_add(&slice_next, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      return PHX_UNI(s_);
    };
    auto sorted_slot = [&](uint32_t k) { return k * 64u + __lane_id(); };
    auto request_round = [&](uint32_t k) {
      next_live = false;
      if (k < nslices) {
        next_i = base + perm[sorted_slot(k)];
        next_live = next_i < count;
        if (next_live) {
          next_t = u2f(pb.hit_tt[next_i].x);  // the pool index of this record is in LDS already (tri_sorted)
          if (want_uv) next_uv = pb.hit_uv[next_i];
          if (!FIRST) { next_a = pb.ro[q][next_i]; next_b = pb.rd[q][next_i]; }
          next_tri = tri_sorted[sorted_slot(k)];  // the shade record does not wait for the hit record: its index is in LDS (four registers across the append)
          if (next_tri != 0xffffffffu) next_S = sc.elem_shade[next_tri];
        }
      }
    };
    // second stage, requested right after the append, travelling while this slice's queue entries are stored: the path state — since round 6 a
    // queue record like the ray, no longer a gather by path id: four registers that need not live across the append
    float4 next_bd = make_float4(1.0f, 1.0f, 1.0f, u2f(0u));  // FIRST: state_t::reset: beta = 1, depth = 0
    auto request_round_dependents = [&]() { if (!FIRST && next_live) next_bd = pb.qs[q][next_i]; };
    // 35.9 / 35.3 / 34.8 ms for no stage / the first / both (profiles/r05_c_shade_prefetch_ab.log).  With per-hit closure weights — glass — either
    // stage costs the kernel 16 B of scratch and buys nothing: 41.7-42.1 ms with, 41.9-42.2 without on the glass showroom
    // (profiles/r05_c_shade_prefetch_glass_ab.log): those instantiations request each record where it is consumed, as the round-4 kernel did
    constexpr bool PREFETCH = !PERHIT;
    uint32_t k = take_slice(), k_next = 0u;
    if constexpr (PREFETCH) { request_round(k); request_round_dependents(); }
    for (; k < nslices; k = k_next) {  // wave-uniform
      const uint32_t i = PREFETCH ? next_i : base + perm[sorted_slot(k)];
      const bool live = PREFETCH ? next_live : i < count;
      // Live ranges are kept short on purpose (the kernel is register-bound: 128 VGPRs as one block of code): radiance and the
      // normals channel are written as soon as the hit is known; the light's record is re-read after the closure evaluation instead
      // of being held across it.
      bool alive = false, want_shadow = false, hit_surface = false;
      uint32_t path = 0, depth = 0, key = 0;
      v3 p, n, wo, beta;
      float2 st = make_float2(0.0f, 0.0f);  // TEX: the hit's texture coordinates
      uint32_t mat = 0;  // the hit's material: an INDEX — bsdf_f / bsdf_sample read the recipe through the scalar cache, one distinct material of the wave at a time
      if (live) {
        float4 a, b, bd;
        float ht; float2 huv = make_float2(0.f, 0.f);  // the hit's distance and barycentrics
        if constexpr (PREFETCH) { ht = next_t; huv = next_uv; }
        else { ht = u2f(pb.hit_tt[i].x); if (want_uv) huv = pb.hit_uv[i]; }
        // the hit's pool index comes from the sort phase (LDS), so its shade record, vertex normals and corner UVs are requested HERE, beside the
        // hit record and the ray (one memory round trip less on the critical path of a round; the texel gathers then wait on u, v only)
        uint32_t tri = 0xffffffffu; float4 S = make_float4(0.f, 0.f, 0.f, 0.f);  // S: (geometric normal, material | smooth << 31), DevScene::elem_shade
        VertexNormals VN_early{v3(0.0f), v3(0.0f), v3(0.0f)};
        CornerUVs UV_early{};  // TEX
        if constexpr (PREFETCH) {
          tri = next_tri; S = next_S;
          if (tri != 0xffffffffu) { VN_early = request_vertex_normals(sc, tri); if constexpr (TEX) UV_early = request_corner_uvs(tx.elem_uv, tri); }
        } else {
          tri = tri_sorted[sorted_slot(k)];
          if (tri != 0xffffffffu) {
            S = sc.elem_shade[tri]; VN_early = request_vertex_normals(sc, tri);
            if constexpr (TEX) UV_early = request_corner_uvs(tx.elem_uv, tri);
          }
        }
        if (FIRST) {
          v3 co, cd;
          camera_ray<LENS>(sc, pb, i, sample0, co, cd);
          a = make_float4(co.x, co.y, co.z, u2f(i)); b = make_float4(cd.x, cd.y, cd.z, FLT_MAX);
          bd = make_float4(1.0f, 1.0f, 1.0f, u2f(0u));  // state_t::reset: beta = 1, depth = 0
        } else {
          if constexpr (PREFETCH) { a = next_a; b = next_b; bd = next_bd; } else { a = pb.ro[q][i]; b = pb.rd[q][i]; bd = pb.qs[q][i]; }
        }
        const uint32_t pbits = f2u(a.w);
        path = pbits & 0x7fffffffu;
        const bool specular = (pbits >> 31) != 0;
        beta = v3(bd.x, bd.y, bd.z);
        depth = f2u(bd.w);
        if (FIRST) {  // the path's RNG key: computed here once, then carried in the ray record's fourth word (k_shade above)
          const uint32_t pix = path / pb.num_samples, s = path - pix * pb.num_samples;
          const uint32_t xy = pb.pix_xy[pix];
          key = path_key(pb.seed, (xy >> 16) * sc.width + (xy & 0xffffu), sample0 + s);
        } else {
          key = f2u(b.w);
        }
        const v3 o(a.x, a.y, a.z), d(b.x, b.y, b.z);
        v3 add_e(0.0f); bool add_rad = false;
        if (tri != 0xffffffffu) {
          hit_surface = true;
          VertexNormals VN;  // (these two copies compute nothing, but the register allocation depends on them: EXPERIMENTS.md, "Retired A/B knobs")
          CornerUVs UV{};
          VN = VN_early; if constexpr (TEX) UV = UV_early;
          if constexpr (TEX) st = hit_st(UV, huv.x, huv.y);
          const uint32_t pm = f2u(S.w);
          p = o + d * ht;             // hits.p = p + wi*d
          wo = -d;                    // hits.wi = -wi
          n = shading_normal(VN, (pm >> 31) != 0, v3(S.x, S.y, S.z), huv.x, huv.y);
          mat = pm & 0x7fffffffu;  // material_t::evaluate (material.cpp:419-458): the closure recipe at this hit
          if (pb.pn && (FIRST || depth == 0)) pb.pn[path] = make_float4(n.x, n.y, n.z, 1.0f);
          if (depth == 0 || specular) {  // spt.hpp:177-179
            const DevMaterial& m = sc.materials[mat]; add_e = v3(m.ex, m.ey, m.ez); add_rad = true;
            if constexpr (TEX) if (tx.any_emit_tex) add_e = hit_emission(tx.textures, tx.texels, emit_tex_table(sc), mat, add_e, st);  // an emitter's image at the hit's (s, t)
          }
        } else {
          // miss: environment lighting (deferred_shading_kernel.hpp:65-70, spt.hpp:199-202); the slot is MASKED|SHADOW in the
          // reference's shadow stream (spt.hpp:138-141): rays_masked = rays_closest - rays_shadow
          if (sc.env_material >= 0) {
            const DevMaterial& m = sc.materials[sc.env_material]; add_e = v3(m.ex, m.ey, m.ez);
            // ENV: e = emission * texel at the ray's direction (environment_node.osl: environment(filename, I)); the binary64 mapping runs
            // on this branch only
            // ... and, under SC_LIGHTS_ENV (wave-uniform), only at depth 0 or behind a specular bounce, the gate of surface emission above:
            // everywhere else next-event estimation has sampled the image already
            if constexpr (ENV) {
              if ((sc.any_tex & SC_LIGHTS_ENV) && !(depth == 0 || specular)) add_e = v3(0.0f);
              else add_e = env_emission(tx.textures, tx.texels, tx.env_tex, tx.env_mapping, d, add_e);
            }
          }
          add_rad = true;
          if (FIRST && pb.pn) pb.pn[path] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
        // out += beta * e with the beta the ray arrived with.  Radiance is only read-modified-written when this step adds something:
        // with e == 0 and a finite beta `out` is unchanged bit for bit (it is never -0)
        if (FIRST) {  // r = 0 + beta * e: every path's radiance is written here, nothing is read
          const v3 rad = v3(0.0f) + beta * add_e;
          pb.pr[path] = make_float4(rad.x, rad.y, rad.z, 0.0f);
        } else if (add_rad && !(isfinite(beta.x) && isfinite(beta.y) && isfinite(beta.z) && add_e.x == 0.0f && add_e.y == 0.0f && add_e.z == 0.0f)) {
          const float4 rr = pb.pr[path];
          const v3 rad = v3(rr.x, rr.y, rr.z) + beta * add_e;
          pb.pr[path] = make_float4(rad.x, rad.y, rad.z, 0.0f);
        }
      }
      PHX_PHASE(1)  // hit record, ray, path state, shade record, normals: requested and landed; emission added
      // the hit's tangent frame (orthogonal_base_t): once per hit, for the NEE evaluation and the BSDF sample
      const Frame fr(hit_surface ? n : v3(0.0f, 1.0f, 0.0f));
      // ---- next-event estimation: sampler_t::fresh_light_samples + light_sampler_t (sampling.cpp:160-179, spt.hpp:95-149)
      v3 sh_o, sh_d, contrib; float sh_t = 0.0f;  // the NEE ray waits in registers for the survivor: both queues are appended in one go below
      {
        if (hit_surface) {
          const uint32_t b0 = depth * DIMS_PER_STEP;
          const float pick = draw_f32(key, b0 + DIM_LIGHT_PICK), lu = draw_f32(key, b0 + DIM_LIGHT_U), lv = draw_f32(key, b0 + DIM_LIGHT_V);
          uint32_t l, ti, lt; float remapped;
          if constexpr (ENV) light_pick_env(sc, pick, lu, l, ti, lt, remapped); else light_pick(sc, pick, lu, l, ti, lt, remapped);  // the triangle by index (the reference) or by area (PHX_LIGHTS_BY_AREA)
          const float x = sqrtf(remapped);
          const float bu = 1 - x, bv = lv * x;     // triangle_t::sample, mesh.cpp:318-324
          // PHX_LIGHT_INCLUDE_ENVIRONMENT: the pick landed on the environment's entry (l == num_lights happens under SC_LIGHTS_ENV only)
          // (`ENV ? .. : constant` conditions: an instantiation without ENV compiles the block it always had)
          bool env_pick = false, env_ok = false;
          if constexpr (ENV) {
            env_pick = l == sc.num_lights;
            if (env_pick) {  // a direction of the image by its tables; the ray runs to infinity, from the side of the surface d leaves on
              const __attribute__((address_space(4))) DevTexScene* ctx = (const __attribute__((address_space(4))) DevTexScene*)sc.tex;
              const DevTexture ET = tx.textures[tx.env_tex];
              uint32_t ei, ej; float es, et, epdf;
              env_ok = env_sample(ctx->env_cdf, ET.width, ET.height, tx.env_mapping, ctx->env_p, lu, lv, ei, ej, es, et, sh_d, epdf);
              const float side = sdot(n, sh_d) < 0.0f ? -0.0001f : 0.0001f;
              sh_o = v3(p.x + n.x * side, p.y + n.y * side, p.z + n.z * side);
              sh_t = 1.0f / epdf;  // 1 / (p_env * pdf_omega) crosses bsdf_f in the register that holds a mesh sample's distance; tmax is set behind it
            }
          }
          if (ENV ? !env_pick : true) {
          {
            const DevLightTri& LT = sc.light_tris[lt];
            const v3 la(LT.ax, LT.ay, LT.az), lb(LT.bx, LT.by, LT.bz), lc(LT.cx, LT.cy, LT.cz);
            const v3 P = bu * la + bv * lb + (1 - bu - bv) * lc;
            sh_o = v3(p.x + n.x * 0.0001f, p.y + n.y * 0.0001f, p.z + n.z * 0.0001f);
            sh_d = P - sh_o;
          }
          const float l2 = sdot(sh_d, sh_d);
          sh_t = sqrtf(l2) - 0.0001f;
          const float oolen = 1.0f / sqrtf(l2);
          sh_d = v3(sh_d.x * oolen, sh_d.y * oolen, sh_d.z * oolen);
          }
          if (ENV ? (env_pick ? env_ok : sdot(n, sh_d) >= 0.0f) : sdot(n, sh_d) >= 0.0f) {
            // li(), spt.hpp:212-255 — evaluated before the occlusion test; k_trace adds it if the ray is unoccluded.  bsdf_f's lobe loop reads the
            // recipe through the scalar cache: -0.6 % shade time, 128 -> 121 VGPRs; in the per-hit (glass) instantiations too, which have the registers
            // since the ring append: closed showroom -4.4 %, glass showroom -2.9 % shade time (profiles/r06_i_perhit_knobs_ab.log)
            v3 f(0.0f);
            if constexpr (TEX) {  // the material's lobes with the texels at (s, t); the lookups read the hit's own row of lobe_tex
              const TexHit th{tx.textures, tx.texels, tx.lobe_tex + 8 * (size_t)mat, st.x, st.y};
              PHX_FOR_EACH_MATERIAL_OF_THE_WAVE(mat, cm, f = (bsdf_f<false, 8, PERHIT, true, MASK>(cm, n, fr, sh_d, wo, th)));
            } else {
              PHX_FOR_EACH_MATERIAL_OF_THE_WAVE(mat, cm, f = (bsdf_f<false, 8, PERHIT>(cm, n, fr, sh_d, wo)));
            }
            // the light's record again (L1-resident), behind an empty asm so that the first read is not kept alive across bsdf_f
            asm volatile("" : "+v"(l), "+v"(lt));
            if constexpr (ENV) {
              if (env_pick) {  // le: the radiance a BSDF ray in this direction would add at its miss; no factor 4, no n.d gate (bsdf_f decided)
                const DevMaterial& em = sc.materials[sc.env_material];
                const v3 le = env_emission(tx.textures, tx.texels, tx.env_tex, tx.env_mapping, sh_d, v3(em.ex, em.ey, em.ez));
                // bsdf_f carries the SIGNED cosine n.d, which the mesh lights' gate keeps positive; here it may be negative (a transmissive
                // lobe lit from below), and the estimate takes |n.d| as the BSDF sample's weight does
                const float sign = sdot(n, sh_d) < 0.0f ? -1.0f : 1.0f;
                contrib = beta * ((le * (f * sign)) * sh_t);
                sh_t = FLT_MAX;
                want_shadow = !(f.x == 0.0f && f.y == 0.0f && f.z == 0.0f);  // (a direction the closures do not see costs no ray)
              }
            }
            if (ENV ? !env_pick : true) {
            const DevLight& L = sc.lights[l];
            const DevLightTri& LT = sc.light_tris[lt];
            const v3 ln = LT.smooth ? shading_normal(sc, LT.prim, true, v3(LT.bx - LT.ax, LT.by - LT.ay, LT.bz - LT.az), v3(LT.cx - LT.ax, LT.cy - LT.ay, LT.cz - LT.az), bu, bv)
                                    : v3(LT.nx, LT.ny, LT.nz);
            v3 le(L.ex, L.ey, L.ez);
            if constexpr (TEX) if (tx.any_emit_tex) { float2 lst; le = light_emission(tx.elem_uv, tx.textures, tx.texels, emit_tex_table(sc), L, LT, bu, bv, lst); }  // material->evaluate(.., light_st, ..).e, spt.hpp:237-254
            const float pdf = L.lpdf * sh_t * sh_t / fabsf(dot(ln, -sh_d));
            const v3 li = ((le * 4.0f) * f) * (1.0f / pdf);
            contrib = beta * li;
            want_shadow = true;
            }
          }
        }
      }
      PHX_PHASE(2)  // next-event estimation: light sample, bsdf_f, li
      // ---- integrate: ++depth, russian roulette, bsdf sampling (spt.hpp:188-190, 257-328)
      {
        v3 nxt_d; uint32_t next_specular = 0; float off = 0.0f;
        if (hit_surface) {
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
            float pdf; uint32_t fl;
            const float u1 = draw_f32(key, b1 + DIM_BSDF_U), u2 = draw_f32(key, b1 + DIM_BSDF_V);
            v3 f;  // bsdf_sample picks its lobe per lane: through the scalar path it is 2-3 % slower (profiles/r04_j_shade_scalar_ab.log)
            if constexpr (TEX) f = bsdf_sample<false, 8, PERHIT, true, MASK>(sc.materials[mat], n, fr, u1, u2, wo, nxt_d, pdf, fl, TexHit{tx.textures, tx.texels, tx.lobe_tex + 8 * (size_t)mat, st.x, st.y});
            else f = bsdf_sample<false, 8, PERHIT>(sc.materials[mat], n, fr, u1, u2, wo, nxt_d, pdf, fl);
            if ((f.x == 0.0f && f.y == 0.0f && f.z == 0.0f) || pdf == 0.0f) {
              alive = false;
            } else {
              const float weight = dot(n, nxt_d);
              beta = beta * (f * (fabsf(weight) / pdf));
              off = (weight < 0.0f) ? -0.0001f : 0.0001f;
              next_specular = (fl & B_SPECULAR) ? 1u : 0u;
            }
          }
        }
        // both queues are appended here, after roulette and sampling (appending the NEE ray before them — shorter live ranges — was right
        // while the kernel fought for occupancy; at 4 waves per SIMD either way the 10 registers are free: 43.1 -> 41.5 ms, profiles/r03_zzc_append2_ab.log)
        PHX_PHASE(3)  // roulette, bsdf_sample
        k_next = take_slice();
        if constexpr (PREFETCH) request_round(k_next);  // in flight across the append (the append waits for LDS traffic only)
        {
          const v3 nxt_o = p + n * off;
          ring_append<3>(want_shadow, make_float4(sh_o.x, sh_o.y, sh_o.z, u2f(path)), make_float4(sh_d.x, sh_d.y, sh_d.z, sh_t), make_float4(contrib.x, contrib.y, contrib.z, 0.0f),
                         &ring_ctl[1], ring_b, &pb.counters[CNT_SHADOW + sq * CNT_STRIDE], pb.so, pb.sd, pb.sc, &pb.stats->ring_watchdog);
          ring_append<3>(alive, make_float4(nxt_o.x, nxt_o.y, nxt_o.z, u2f(path | (next_specular << 31))), make_float4(nxt_d.x, nxt_d.y, nxt_d.z, u2f(key)),
                         make_float4(beta.x, beta.y, beta.z, u2f(depth)),  // the path's state travels with its ray: only the next shade of a surviving path reads it
                         &ring_ctl[0], ring_a, &pb.counters[(q ^ 1) * CNT_STRIDE], pb.ro[q ^ 1], pb.rd[q ^ 1], pb.qs[q ^ 1], &pb.stats->ring_watchdog);
        }
        PHX_PHASE(4)  // the append: slot reservation, records to LDS, commit; for one wave in BLK / 64 rounds the flush of a block
        if constexpr (PREFETCH) request_round_dependents();
        PHX_PHASE(5)  // the stores of the two queue entries (waited for: the probe charges them here, the product build does not wait)
#if PHX_SHADE_TIMING
        ++ph_rounds;
#endif
      }
    }
    __syncthreads();  // perm and bucket are rewritten by the next window
  }
  // what the workgroup's last windows left in the rings: every complete block has been flushed by the wave that completed it (before that
  // wave reached the barrier above); the open block goes out with its exact count, the survivors' by wave 0, the NEE rays' by wave 1
  __syncthreads();
  if (threadIdx.x < 128u) {
    const uint32_t w = threadIdx.x >> 6;
    const uint32_t head = ring_ctl[w].head, left = head & (PHX_RING_BLK - 1u), first = ((head / PHX_RING_BLK) & 1u) * PHX_RING_BLK;
    // (a ring that timed out is NOT flushed: a wave that gave up has reserved slots it never wrote, and whatever LDS held there — records of two
    // blocks ago, or nothing at all — must not reach a queue, where a path id is an index.  The frame is reported as failed anyway.  The
    // ring-watchdog twin library faulted the GPU on exactly this until the guard was added: tests/test_gpu_parity.py::test_append_ring_timeout_…)
    if (left && !ring_ctl[w].dead) {
      if (w == 0u) ring_flush<3>(ring_a, first, left, &pb.counters[(q ^ 1) * CNT_STRIDE], pb.ro[q ^ 1], pb.rd[q ^ 1], pb.qs[q ^ 1]);
      else ring_flush<3>(ring_b, first, left, &pb.counters[CNT_SHADOW + sq * CNT_STRIDE], pb.so, pb.sd, pb.sc);
    }
  }
#if PHX_SHADE_TIMING
  if ((threadIdx.x & 63u) == 0u) {  // probe build only: s_memtime ticks per phase, summed over the waves (DevStats fields of the count build)
    for (int k = 0; k < 6; ++k) atomicAdd(&pb.stats->stack_pushes[k], ph_acc[k]);
    atomicAdd(&pb.stats->stack_pushes[6], ph_rounds); atomicAdd(&pb.stats->stack_pushes[7], ph_windows);
  }
#endif
}

// ---- launches ---------------------------------------------------------------------------------------
// k_shade / k_shade_g walk the queue with a fixed grid: PHX_SHADE_GRID workgroups per resident slot (never more than the queue's
// capacity needs)
static uint32_t shade_grid(const DevScene& sc, uint32_t capacity, uint32_t per_wg, uint32_t block) {
  static const int mul = [] { const char* v = getenv("PHX_SHADE_GRID"); const int x = v ? atoi(v) : 4; return x < 1 ? 4 : x; }();
  const uint32_t resident = sc.num_cus * (2048u / block);
  const uint32_t need = (capacity + per_wg - 1) / per_wg;
  return std::max(1u, std::min(need, resident * (uint32_t)mul));
}
template <bool PERHIT, bool FIRST, bool LENS, bool TEX, bool ENV, bool MASK>
static uint64_t shade_g(dim3 g, dim3 b, hipStream_t stream, const DevScene& sc, const PassBuffers& pb, int q, int sq, uint32_t sample0) {
  static_assert(!MASK || (PERHIT && TEX), "image masks are per-hit weights with a texel lookup");
  constexpr uint32_t family = MASK ? (ENV ? PHX_SHADE_FAMILY_MASK_ENV : PHX_SHADE_FAMILY_MASK)
                                   : PHX_SHADE_FAMILY_GENERAL + ((PERHIT ? PHX_SHADE_G_PERHIT : 0) | (TEX ? PHX_SHADE_G_TEX : 0) | (ENV ? PHX_SHADE_G_ENV : 0));
  constexpr uint32_t bit = family * PHX_SHADE_PASSES + shade_pass<FIRST, LENS>();
  static_assert(bit < PHX_SHADE_KERNELS, "phx_stats::shade_kernels: a kernel without a bit");
  hipLaunchKernelGGL((k_shade_g<PERHIT, FIRST, LENS, TEX, ENV, MASK>), g, b, 0, stream, sc, pb, q, sq, sample0);
  return 1ull << bit;
}
uint64_t launch_shade(hipStream_t stream, const DevScene& sc, const PassBuffers& pb, int q, int sq, uint32_t capacity, uint32_t sample0, int camera_rays) {
  const bool lens = camera_rays && sc.aperture_radius != 0.0f;  // camera_t::is_pinhole, entities/camera.hpp:37
  if (sc.diffuse_only) return launch_shade_lambert(stream, sc, pb, q, sq, capacity, sample0, camera_rays, lens);
  const dim3 g(shade_grid(sc, capacity, PHX_SHADE_BLOCK_G * PHX_SHADE_ITEMS_G, PHX_SHADE_BLOCK_G)), b(PHX_SHADE_BLOCK_G);
  auto general = [&](auto PERHIT, auto TEX, auto ENV, auto MASK) {
    return with_pass(camera_rays != 0, lens, [&](auto FIRST, auto LENS) {
      return shade_g<decltype(PERHIT)::value, decltype(FIRST)::value, decltype(LENS)::value, decltype(TEX)::value, decltype(ENV)::value, decltype(MASK)::value>(g, b, stream, sc, pb, q, sq, sample0);
    });
  };
  const bool env = (sc.any_tex & SC_TEX_ENV) != 0;  // an environment image: the same kernels with the lookup on the miss branch
  // image masks on closure mixes: per-hit weights with a texel lookup (PERHIT, TEX and MASK together)
  if (sc.any_tex & SC_TEX_MASK) return with_flag(env, [&](auto ENV) { return general(std::true_type{}, std::true_type{}, ENV, std::true_type{}); });
  return with_flag(env, [&](auto ENV) {
    return with_flag((sc.any_tex & SC_TEX_LOBES) != 0, [&](auto TEX) {  // textured scenes: the same kernel with the texel lookups compiled in
      return with_flag(sc.any_per_hit != 0, [&](auto PERHIT) { return general(PERHIT, TEX, ENV, std::false_type{}); });
    });
  });
}

}  // namespace phx
