// trace.hip — the traversal kernels of the wavefront path tracer and their launches (see kernels.h for the HBM layout and the
// map of kernels to files).  One ray per lane, 64-lane wavefronts.
//
//   k_trace_primary  the trace for the camera rays of a pass, the one coherent launch of a frame: a wave walks the tree once
//               for a packet of 64..256 rays (interval slab test per node, the reference's triangle test per ray)
//   k_trace     stream_mbvh_kernel_t::trace (reference src/kernels/cpu/stream_bvh_kernel.cpp:18-161) re-thought per lane:
//               BVH8 nodelets, (base,mask) group stack in LDS, closest-hit and any-hit rays in one persistent launch,
//               lanes refilled from chunks each wave pulls for itself
//   k_trace_rays  the stage-level hook (phx_dev_trace): one ray per lane with the plain traverse8 loop of bvh8.h
#include "shade_common.h"

namespace phx {

#define PHX_PERM_LUT_BYTES 2048u  /* k_trace: the octant permutations of the hit masks come from a table in LDS (8 octants x 256 masks) instead of 2 x 15 VALU instructions */
#ifndef PHX_COUNT
#define PHX_COUNT 0  /* 1: instrumented build that counts node visits and triangle tests (bench.py's device-layout byte model) */
#endif

// ---- trace ----------------------------------------------------------------------------------------
template <int LEVELS>
struct LdsStack {
  uint2* base;  // &lds[threadIdx.x]; entry k lives at base[k * PHX_BLOCK]: conflict-free 8-byte accesses
  int sp;
  __device__ __forceinline__ void push(uint32_t b, uint32_t h) { base[sp * PHX_BLOCK] = make_uint2(b, h); ++sp; }
  __device__ __forceinline__ void pop(uint32_t& b, uint32_t& h) { --sp; const uint2 e = base[sp * PHX_BLOCK]; b = e.x; h = e.y; }
  __device__ __forceinline__ bool empty() const { return sp == 0; }
};

// ---- wave-level streaming traversal -------------------------------------------------------------------
// A wave64 that runs one ray per lane to completion wastes most of its lanes: ray lengths differ widely
// (measured: ~20 % VALU lane utilisation with the plain per-lane loop).  Here every lane is a small state
// machine and the wave iterates "one node visit, one triangle test, pop/finish" with all lanes in whatever
// state they are in; a lane whose ray has finished is REFILLED from the workgroup's range of the queue as
// soon as REFILL_MIN lanes are idle (cursor in LDS: one ds_add per refill, no global atomics).
// Visiting order, box test and triangle test are those of traverse8 (bvh8.h), so results are identical.
// One stream serves BOTH queues: lanes are refilled from the workgroup's shadow-ray range first, then from
// its closest-hit range; the any-hit / closest-hit distinction is a per-lane flag, so a launch has a single
// drain phase (the tail where rays run out and lanes idle) instead of one per queue.
// The chunks of the persistent launch are handed out in two levels.  A WORKGROUP takes 16 chunks' worth of
// consecutive rays from the global cursor at a time; its waves take their chunks from that range through a 64-bit word in LDS
// (next | end << 32: one ds_add returns a consistent pair).  The wave that finds the range used up fetches the next one
// (try-lock in LDS, re-check under the lock); waves that lose the race go on traversing and ask again at their next refill.
// Sixteen waves of one CU then work on neighbouring pixels, and the global cursor takes 1/16 of the atomics.
// (Round 2 also carried a static XCD-aware split of the queues and per-wave global chunks; both lost to this scheme on every
// workload and were removed in round 3 — the history is in EXPERIMENTS.md, Part B section 3.)
#ifndef PHX_WG_CHUNKS
#define PHX_WG_CHUNKS 16u  /* chunks in a workgroup's range (fewer when the queue is too short to give every workgroup four ranges) */
#endif
#ifndef PHX_SPILL_FROM_LEVELS
#define PHX_SPILL_FROM_LEVELS 10u  /* trees with this many stack levels or more keep only PHX_SPILL_LDS_LEVELS of them in LDS */
#endif
#ifndef PHX_SPILL_LDS_LEVELS
#define PHX_SPILL_LDS_LEVELS 7u
#endif
#ifndef PHX_STACK_PACKED
// Deep trees (the SPILL plan: >= 10 stack levels, 7 of them in LDS) keep 5-byte stack entries in LDS — (child base : 24 | pending inner hits : 8)
// as a dword + the node's valid mask as a byte, four levels of a lane sharing one dword — instead of 8-byte ones; the 21 KB this frees per
// workgroup stage 256 more nodelets (281 -> 537).  Measured (profiles/r06_f_packed_stack_ab.log): k_trace -2.3 % on BASELINE config 4 (10 M
// triangles), -4.0 % on the closed showroom (depth 13); trees whose stacks fit LDS gain nothing from more staged nodelets (100 k: +0.7 %, the
// second LDS access per push / pop; 1 M: +-0) and keep 8-byte entries.  Pools of < 2^24 elements only (1 GB; larger ones: 8-byte entries).
// 0 = never (the nopack twin library), 1 = the SPILL plan.
#define PHX_STACK_PACKED 1
#endif
#ifndef PHX_TRACE_WATCHDOG
#define PHX_TRACE_WATCHDOG (1u << 22)  /* loop iterations after which a k_trace wave exits with DevStats::watchdog set (a launch needs ~1e4): every wave reaches its exit */
#endif
struct DynQueue {            // the launch is persistent and every WAVE pulls chunks of both queues on its own
  uint32_t n0, n1, c0, c1;   // queue lengths and chunk sizes (0 shadow, 1 closest), wave-uniform
  uint32_t r0, r1;           // rays in a workgroup's range
  uint32_t num_waves;
  uint32_t* cursor;          // pb.counters + CNT_CURSOR: two global cursors, zeroed by the kernel that filled the queues
};
template <int BLOCK, bool SPILL /* the stack's deep levels live in HBM */, bool PACKED /* 5-byte stack entries in LDS */,
          bool UV /* the scene reads barycentrics: keep (u, v) of the closest hit and store pb.hit_uv beside pb.hit_tt */>
__device__ __forceinline__ void trace_stream(const DevScene& sc, const PassBuffers& pb, int q,
                                             uint32_t* cursor /* LDS: the workgroup's ranges */, uint2* stack_base, uint8_t* stack_valid /* PHX_STACK_PACKED: this thread's dword of the valid-mask rows */, uint32_t lds_levels,
                                             uint2* spill_base /* this thread's column of sc.stack_spill */, uint32_t refill_min,
                                             const uint4* __restrict__ top /* nodelets staged in LDS */, uint32_t ntop,
                                             const DynQueue dq, const uint8_t* __restrict__ perm_lut) {
  const uint32_t lane = __lane_id();
  bool active = false, any = false;
  uint32_t phase = 0;  // wave-uniform: 0 = shadow range, 1 = closest range, 2 = drained
  RayCtx r; r.o = v3(0.f); r.d = v3(0.f); r.idx = r.idy = r.idz = 0.f; r.oct_inv = 0;
  float tbest = 0.f, hu = 0.f, hv = 0.f;
  uint32_t htri = 0xffffffffu, hprim = 0, idx = 0, ng_base = 0, ng_hits = 0, path = 0;
  // triangle group of the lane: tg_base = pool index of the first child of the node the triangles hang below; tg = that node's
  // valid mask (bits 0..7) | hit leaf slots still to test (8..15); (tq_base, tq) is a second such group, waiting
  constexpr uint32_t TG_PENDING = 0xff00u;
  uint32_t tg_base = 0, tg = 0, tq_base = 0, tq = 0;  // tq: the second group (valid | pending << 8), 0 = none
  int sp = 0;
  const float4* __restrict__ ro = pb.ro[q];
  const float4* __restrict__ rd = pb.rd[q];
  uint32_t dlo = 0, dhi = 0;  // the wave's current chunk [dlo, dhi)
  // Element i of the pool.  Every instantiation but the unpacked SPILL one runs on pools of < 2^26 elements only (trace_plan), whose byte offsets
  // fit 32 bits: the fetch is then global_load v, s[pool] with ONE 32-bit shift per lane, where the 64-bit address costs a 64-bit shift and a
  // 64-bit add per lane and fetch (-1.3 % of k_trace, profiles/r08_ktrace_select_ab.log)
  constexpr bool OFF32 = !(SPILL && !PACKED);
  auto pool_elem = [&](uint32_t i) {
    if constexpr (OFF32) return reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(sc.pool) + (i << 6));
    else return reinterpret_cast<const uint4*>(sc.pool) + (size_t)i * 4u;
  };
#if PHX_COUNT
  uint32_t cnt_lds[2] = {0, 0}, cnt_mem[2] = {0, 0}, cnt_tri[2] = {0, 0};  // instrumented build: this lane's traversal work
  uint32_t cnt_iter = 0, cnt_nb = 0, cnt_tb = 0, cnt_refill = 0;              // ... and the wave's (wave-uniform)
  uint32_t cnt_idle = 0, cnt_pend = 0;
  uint32_t cnt_push[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  // pending (ray, triangle) pairs of the WAVE when its triangle block runs — each lane tests one of its own per execution; a block that
  // handed pairs to idle lanes could test up to 64 (profiles/r06_tri_handoff.md) — summed, and as a histogram
  uint32_t cnt_pairs = 0, cnt_pairs_hist[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#endif
  uint32_t guard = 0;  // wave-uniform (an SGPR): iterations of this wave
  for (;;) {
    if (++guard > PHX_TRACE_WATCHDOG) { if (lane == 0) atomicAdd(&pb.stats->watchdog, 1ull); break; }
    // ---- refill idle lanes from the workgroup's cursors
    const unsigned long long idle = __ballot(!active);
    if (phase < 2u && (uint32_t)__popcll(idle) >= refill_min) {
#if PHX_COUNT
      ++cnt_refill;
#endif
      const uint32_t leader = (uint32_t)__ffsll((long long)idle) - 1u;
      uint32_t hi, base;
      {
        if (dlo >= dhi) {  // chunk used up: take the next one out of the workgroup's range
          const uint32_t c = phase == 0u ? dq.c0 : dq.c1, qn = phase == 0u ? dq.n0 : dq.n1;
          uint32_t got_lo = 0, got_hi = 0, st = 1;  // st: 0 a chunk, 1 ask again later, 2 this queue is exhausted
          if (lane == leader) {
            unsigned long long* pack = reinterpret_cast<unsigned long long*>(cursor) + phase;
            uint32_t* fetching = cursor + 4 + phase; uint32_t* done = cursor + 6 + phase;
            const unsigned long long old = __hip_atomic_fetch_add(pack, (unsigned long long)c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            const uint32_t s0 = (uint32_t)old, e0 = (uint32_t)(old >> 32);
            if (s0 < e0) { got_lo = s0; got_hi = min(s0 + c, e0); st = 0; }
            else if (__hip_atomic_load(done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) st = 2;
            else if (atomicCAS(fetching, 0u, 1u) == 0u) {
              __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
              const unsigned long long cur = __hip_atomic_load(pack, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
              if ((uint32_t)cur < (uint32_t)(cur >> 32)) st = 1;  // another wave refilled the range in the meantime
              else if (__hip_atomic_load(done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) st = 2;
              else {
                const uint32_t cwg = phase == 0u ? dq.r0 : dq.r1;
                // the next range of this XCD's segment of the queue; when that is used up, of the next segment that has one (cursor[8 + phase])
                uint32_t nb = qn, seg_end = qn, sgm = cursor[8 + phase];
                for (uint32_t tries = 0; tries < CNT_SEGS; ++tries, sgm = (sgm + 1u) & (CNT_SEGS - 1u)) {
                  const uint32_t lo_s = (uint32_t)((unsigned long long)qn * sgm / CNT_SEGS), hi_s = (uint32_t)((unsigned long long)qn * (sgm + 1u) / CNT_SEGS);
                  const uint32_t homes = (gridDim.x + CNT_SEGS - 1u - sgm) / CNT_SEGS;  // workgroups whose first range lies in this segment
                  const unsigned long long at = (unsigned long long)lo_s + (unsigned long long)homes * cwg + atomicAdd(&dq.cursor[(phase * CNT_SEGS + sgm) * CNT_STRIDE], cwg);
                  if (at < hi_s) { nb = (uint32_t)at; seg_end = hi_s; break; }
                }
                cursor[8 + phase] = sgm;
                if (nb >= seg_end) { __hip_atomic_store(done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); st = 2; }
                else {
                  const uint32_t end = min(nb + cwg, seg_end);
                  got_lo = nb; got_hi = min(nb + c, end); st = 0;  // the fetching wave keeps the range's first chunk
                  __hip_atomic_store(pack, (unsigned long long)(nb + c) | ((unsigned long long)end << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
              }
              __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
              __hip_atomic_store(fetching, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
          }
          st = (uint32_t)__builtin_amdgcn_readfirstlane((int)__shfl((int)st, (int)leader));
          if (st == 2u) {  // this queue is exhausted
            phase = PHX_UNI(phase + 1u);
            if (phase < 2u || __ballot(active) != 0ull) { if (phase < 2u) continue; } else break;
          } else if (st == 0u) {
            dlo = (uint32_t)__builtin_amdgcn_readfirstlane((int)__shfl((int)got_lo, (int)leader));
            dhi = (uint32_t)__builtin_amdgcn_readfirstlane((int)__shfl((int)got_hi, (int)leader));
          } else if (__ballot(active) == 0ull) { __builtin_amdgcn_s_sleep(4); continue; }  // nothing to do but wait for the fetching wave (the watchdog counts these sleeps too: a separate counter for them cost 2 % of the kernel, profiles/r04_t_spin_ab.log)
        }
        if (phase >= 2u) { hi = 0; base = 0; }
        else {
          const uint32_t take = PHX_UNI(min((uint32_t)__popcll(idle), dhi - dlo));
          base = dlo; hi = dlo + take; dlo = PHX_UNI(dlo + take);
        }
      }
      if (!active) {
        // rank of this idle lane in pair-major order (0, 32, 1, 33, ...): consecutive rays go to the two lanes of a pair
        const uint32_t l5 = lane & 31u, below = (1u << l5) - 1u, ilo = (uint32_t)idle, ihi = (uint32_t)(idle >> 32);
        const uint32_t my = base + (uint32_t)__popc(ilo & below) + (uint32_t)__popc(ihi & below) + (lane >= 32u ? ((ilo >> l5) & 1u) : 0u);
        if (my < hi) {
          {
            float4 a, b;
            if (phase == 0u) { a = pb.so[my]; b = pb.sd[my]; } else { a = ro[my]; b = rd[my]; }
            r = make_ray_ctx(v3(a.x, a.y, a.z), v3(b.x, b.y, b.z));
            tbest = phase == 0u ? b.w : FLT_MAX; path = f2u(a.w);  // a closest-hit ray always starts at FLT_MAX (spt.hpp:301-305): the queue's fourth word carries the path's RNG key instead
          }
          hu = 0.f; hv = 0.f; htri = 0xffffffffu; hprim = 0; idx = my;
          ng_base = 0; ng_hits = 0x80000000u; tg = 0; tq = 0; sp = 0;  // the root as a one-child group (bvh8.h: traverse8)
          any = phase == 0u;
          active = true;
        }
      }
      if (phase < 2u && __ballot(active) == 0ull) continue;  // nothing in flight yet: go fetch from the next range
    }
    if (!__ballot(active)) break;
#if PHX_COUNT
    ++cnt_iter;
    cnt_idle += (uint32_t)__popcll(__ballot(!active));
#endif
    // ---- one node visit.  A lane's node work (ng_base, ng_hits, the stack) and its triangle work (tg_base, tg: the hit leaf
    // slots of ONE visited node; a second such group waits in the lane's LDS slot) are independent: a lane whose last node left
    // triangles to test goes on to its next node in the same iteration, and sits the node block out only when both triangle
    // groups are taken.  (Until round 4 a lane with pending triangles sat out: 8.6 of 64 lanes in every iteration.)  Triangles
    // are then tested LATER relative to the node visits than in traverse8 — against a tbest that is at most smaller — and the
    // boxes are culled against a tbest that is at most larger: the lane meets a superset of traverse8's triangles, and the closest
    // hit with its tie rule does not depend on which superset (bvh8.h).
    const bool node_ok = active && ng_hits > 0x00ffffffu && (any ? !(tg & TG_PENDING) : tq == 0u);  // an any-hit ray tests what it has first: a hit ends it
#if PHX_COUNT
    if (__ballot(node_ok)) ++cnt_nb;
    cnt_pend += (uint32_t)__popcll(__ballot(active && !node_ok && (tg & TG_PENDING)));
#endif
    if (node_ok) {
      const uint32_t bit = 31u - (uint32_t)__clz((int)ng_hits);
      const uint32_t rest = ng_hits & ~(1u << bit);
      if (rest > 0x00ffffffu) {
#if PHX_COUNT
        ++cnt_push[sp < 7 ? sp : 7];
#endif
        // SPILL: the top lds_levels entries of the stack live in LDS, the rare deeper ones in HBM (sc.stack_spill)
        if (!SPILL || (uint32_t)sp < lds_levels) {
          if constexpr (PACKED) {
            reinterpret_cast<uint32_t*>(stack_base)[sp * BLOCK] = (ng_base & 0x00ffffffu) | (rest & 0xff000000u);
            stack_valid[((uint32_t)sp >> 2) * (BLOCK * 4u) + ((uint32_t)sp & 3u)] = (uint8_t)rest;   // four levels share a lane's dword: the access pattern of a 4-byte column
          } else stack_base[sp * BLOCK] = make_uint2(ng_base, rest);
        }
        else spill_base[(size_t)((uint32_t)sp - lds_levels) * sc.spill_stride] = make_uint2(ng_base, rest);
        ++sp;
      }
      const uint32_t slot = (bit - 24u) ^ r.oct_inv;
      const uint32_t ni = ng_base + (uint32_t)__popc(ng_hits & 0xffu & ~(0xffffffffu << slot));
      uint32_t w[16];
#if PHX_COUNT
      if (ni < ntop) ++cnt_lds[any ? 1 : 0]; else ++cnt_mem[any ? 1 : 0];
#endif
      // top-of-tree nodelets are staged in LDS: four ds_read_b128 instead of four L1 requests per lane.  The LDS lanes go
      // first: both groups write the same registers, so the second group waits for the first one's data — a few dozen cycles
      // for LDS, several hundred for the L1/L2 path if it went first.
      const bool in_lds = ni < ntop;
      {
        const uint4* s4 = top + (in_lds ? ni : 0u) * (PHX_NODE_LDS_BYTES / 16u);  // every lane reads (element 0 when its node is not staged)
#pragma unroll
        for (int k = 0; k < 4; ++k) { const uint4 v = s4[k]; w[4 * k] = v.x; w[4 * k + 1] = v.y; w[4 * k + 2] = v.z; w[4 * k + 3] = v.w; }
      }
      if (!in_lds) {
        const uint4* s4 = pool_elem(ni);
#pragma unroll
        for (int k = 0; k < 4; ++k) { const uint4 v = s4[k]; w[4 * k] = v.x; w[4 * k + 1] = v.y; w[4 * k + 2] = v.z; w[4 * k + 3] = v.w; }
      }
      const uint32_t hm = node_hitmask(w, sc.grid, r, tbest, [&](uint32_t m) { return (uint32_t)perm_lut[(r.oct_inv << 8) | m]; });
      ng_base = w[3];                // the children of the node just visited: nodelets and triangle records, in slot order
      ng_hits = hm & 0xff0000ffu;    // pending inner children | valid mask
      const uint32_t tnew = (hm >> 8) & TG_PENDING;  // hit leaf slots of this node -> bits 8..15
      if (tnew) {
        const uint32_t g = (hm & 0xffu) | tnew;       // valid mask | pending triangles
        if (!(tg & TG_PENDING)) { tg_base = w[3]; tg = g; }
        else { tq_base = w[3]; tq = g; }
      }
    }
    // ---- one triangle test per lane that has one pending
    const bool tpend = active && (tg & TG_PENDING);
#if PHX_COUNT
    if (__ballot(tpend)) {
      ++cnt_tb;
      const uint32_t mine = active ? (uint32_t)__popc((tg >> 8) & 0xffu) + (uint32_t)__popc((tq >> 8) & 0xffu) : 0u;  // <= 16
      uint32_t pairs = 0;
      for (uint32_t b = 0; b < 5u; ++b) pairs += (uint32_t)__popcll(__ballot((mine >> b) & 1u)) << b;
      cnt_pairs += pairs;
      ++cnt_pairs_hist[pairs <= 8u ? 0 : pairs <= 16u ? 1 : pairs <= 24u ? 2 : pairs <= 32u ? 3 : pairs <= 48u ? 4 : pairs <= 64u ? 5 : pairs <= 96u ? 6 : 7];
    }
#endif
    if (tpend) {
      const uint32_t k = 23u - (uint32_t)__clz((int)(tg & TG_PENDING));  // slot of the highest pending triangle (bits 8..15 -> 7..0)
      tg &= ~(0x100u << k);
      const uint32_t ti = tg_base + (uint32_t)__popc(tg & 0xffu & ~(0xffffffffu << k));
      const uint4* t4 = pool_elem(ti);
      const uint4 t0 = t4[0], t1 = t4[1], t2 = t4[2];  // three of the record's four words: v0, e0, e1, prim
      TriRec T;
      T.v0x = u2f(t0.x); T.v0y = u2f(t0.y); T.v0z = u2f(t0.z); T.e0x = u2f(t0.w);
      T.e0y = u2f(t1.x); T.e0z = u2f(t1.y); T.e1x = u2f(t1.z); T.e1y = u2f(t1.w);
      T.e1z = u2f(t2.x); T.prim = t2.y;
      float us, vs, ds;
#if PHX_COUNT
      ++cnt_tri[any ? 1 : 0];
#endif
      if (mt_intersect(T, r.o, r.d, tbest, hprim, us, vs, ds)) {
        tbest = ds; htri = ti; hprim = T.prim;
        if constexpr (UV) { hu = us; hv = vs; }  // UV = false: us, vs feed the accept test only, and two VGPRs leave the loop
        if (any) active = false;  // occluded: nothing to add
      }
      if (!(tg & TG_PENDING) && tq != 0u) { tg_base = tq_base; tg = tq; tq = 0u; }  // this group is done and another one waits
    }
    // ---- pop the next node group; a ray is finished when neither nodes nor triangles are left
    if (active && ng_hits <= 0x00ffffffu) {
      if (sp == 0) {
        if (!(tg & TG_PENDING)) {
          if (any) {  // unoccluded: out += beta * li (spt.hpp:184-186); one shadow ray per path and step
            const float4 cc = pb.sc[idx];
            float4 rr = pb.pr[path];
            rr.x += cc.x; rr.y += cc.y; rr.z += cc.z;
            pb.pr[path] = rr;
          } else {
            pb.hit_tt[idx] = make_uint2(f2u(tbest), htri);
            if constexpr (UV) pb.hit_uv[idx] = make_float2(hu, hv);
          }
          active = false;
        }
      } else {
        --sp;
        uint2 e;
        if (!SPILL || (uint32_t)sp < lds_levels) {
          if constexpr (PACKED) {
            const uint32_t word = reinterpret_cast<uint32_t*>(stack_base)[sp * BLOCK];
            const uint32_t vb = stack_valid[((uint32_t)sp >> 2) * (BLOCK * 4u) + ((uint32_t)sp & 3u)];
            e = make_uint2(word & 0x00ffffffu, (word & 0xff000000u) | vb);
          } else e = stack_base[sp * BLOCK];
        }
        else e = spill_base[(size_t)((uint32_t)sp - lds_levels) * sc.spill_stride];
        ng_base = e.x; ng_hits = e.y;
      }
    }
  }
#if PHX_COUNT
  for (int k = 0; k < 2; ++k) {
    atomicAdd(&pb.stats->node_visits_lds[k], (unsigned long long)cnt_lds[k]);
    atomicAdd(&pb.stats->node_visits_mem[k], (unsigned long long)cnt_mem[k]);
    atomicAdd(&pb.stats->tri_tests[k], (unsigned long long)cnt_tri[k]);
  }
  for (int k = 0; k < 8; ++k) if (cnt_push[k]) atomicAdd(&pb.stats->stack_pushes[k], (unsigned long long)cnt_push[k]);
  if (lane == 0) {
    atomicAdd(&pb.stats->tri_block_execs, (unsigned long long)cnt_tb);
    atomicAdd(&pb.stats->wave_iters, (unsigned long long)cnt_iter);
    atomicAdd(&pb.stats->node_block_execs, (unsigned long long)cnt_nb);
    atomicAdd(&pb.stats->refills, (unsigned long long)cnt_refill);
    atomicAdd(&pb.stats->idle_lane_iters, (unsigned long long)cnt_idle);
    atomicAdd(&pb.stats->tri_pending_lane_iters, (unsigned long long)cnt_pend);
    atomicAdd(&pb.stats->tri_pairs_pending, (unsigned long long)cnt_pairs);
    for (int k = 0; k < 8; ++k) if (cnt_pairs_hist[k]) atomicAdd(&pb.stats->tri_pairs_hist[k], (unsigned long long)cnt_pairs_hist[k]);
  }
#endif
}

// Trace kernel: closest-hit rays of ray queue `q` (if do_closest) and any-hit rays of the shadow queue `sq`
// filled by the previous k_shade (if do_shadow) in ONE launch, so that late bounces with few rays still fill
// the chip.  Queue lengths are only known on the device.
//   The launch is persistent — exactly the resident workgroups — and work is handed out in two levels:
//   a workgroup takes a range of 16 x 64 consecutive rays from a global cursor (its first range is its own by
//   position), its waves take 64-ray chunks out of that range through a word in LDS.  Fine chunks keep the drain phase short,
//   and the global cursor sees one returning atomic per 1024 rays instead of one per chunk (which the wave has to wait for:
//   with per-wave global chunks 512 rays were the optimum, 64-ray chunks were atomic-bound).  A wave
//   drains once per launch, not once per slice, and a slow image region is shared by everyone.
// Dynamic LDS layout: [ntop pool elements x 80 B][levels x BLOCK stack entries x 8 B][12 cursor words][2 KB octant table].
template <int BLOCK, bool SPILL = false, bool PACKED = false, bool UV = false>
__global__ void __launch_bounds__(BLOCK, 8) k_trace(DevScene sc, PassBuffers pb, int q, int sq, int do_closest, int do_shadow, uint32_t refill_min,
                                                 uint32_t ntop, uint32_t levels, uint32_t min_chunks, uint32_t target_chunks) {
  extern __shared__ uint4 smem[];
  uint4* top = smem;
  uint2* stack = reinterpret_cast<uint2*>(smem + ntop * (PHX_NODE_LDS_BYTES / 16u));
  // PACKED: [levels x BLOCK dwords][ceil(levels / 4) x BLOCK dwords of valid bytes]: 4 + 1 bytes per entry
  uint32_t* stack_words = reinterpret_cast<uint32_t*>(stack);
  uint32_t* valid_rows = stack_words + levels * BLOCK;
  uint32_t* cursor = PACKED ? valid_rows + ((levels + 3u) >> 2) * BLOCK : reinterpret_cast<uint32_t*>(stack + levels * BLOCK);
  uint8_t* perm_lut = reinterpret_cast<uint8_t*>(cursor + 12);  // PHX_PERM_LUT_BYTES: 8 octants x 256 masks (cursor: 12 words)
  const uint32_t n_closest = do_closest ? pb.counters[q * CNT_STRIDE] : 0u;
  const uint32_t n_shadow = do_shadow ? pb.counters[CNT_SHADOW + sq * CNT_STRIDE] : 0u;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    // the queues k_shade will append to next: the other ray queue and the other shadow queue
    if (do_closest) { pb.counters[(q ^ 1) * CNT_STRIDE] = 0; pb.counters[CNT_SHADOW + (sq ^ 1) * CNT_STRIDE] = 0; }
    if (n_closest) atomicAdd(&pb.stats->rays_closest, (unsigned long long)n_closest);
    if (n_shadow) atomicAdd(&pb.stats->rays_shadow, (unsigned long long)n_shadow);
    // the host sizes the grids of the NEXT steps' shade launches by this length (queues never grow from one step to the next): a k_shade
    // grid sized for the queue's capacity launches 230 k workgroups at every step, nearly all of them empty from the third step on
    if (do_closest && pb.qlen_out) { __hip_atomic_store(pb.qlen_out, n_closest, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); }
  }
  if (n_shadow == 0u && n_closest == 0u) return;
  DynQueue dq{};
  dq.n0 = n_shadow; dq.n1 = n_closest;
  dq.num_waves = gridDim.x * (BLOCK / 64);
  dq.cursor = pb.counters + CNT_CURSOR;
  // ~min_chunks chunks per wave for mid-size queues, 64 .. target_chunks*64 rays each
  auto chunk_of = [&](uint32_t n) { return min(max((n / (dq.num_waves * max(min_chunks, 1u)) + 63u) & ~63u, 64u), target_chunks * 64u); };
  dq.c0 = chunk_of(n_shadow); dq.c1 = chunk_of(n_closest);
  // a workgroup's range: PHX_WG_CHUNKS chunks, fewer when the queue could not give every workgroup four such ranges
  auto range_of = [&](uint32_t n, uint32_t c) { return c * min(max(n / (gridDim.x * c * 4u), 1u), PHX_WG_CHUNKS); };
  dq.r0 = range_of(n_shadow, dq.c0); dq.r1 = range_of(n_closest, dq.c1);
  if (threadIdx.x == 0) {  // the workgroup's first range is its own by position; read by the waves after the barrier below
    unsigned long long* pack = reinterpret_cast<unsigned long long*>(cursor);
    for (uint32_t p = 0; p < 2u; ++p) {
      const uint32_t cwg = p == 0u ? dq.r0 : dq.r1, qn = p == 0u ? n_shadow : n_closest;
      const uint32_t sgm = blockIdx.x & (CNT_SEGS - 1u), kth = blockIdx.x / CNT_SEGS;  // the kth range of this XCD's segment
      const uint32_t lo_s = (uint32_t)((unsigned long long)qn * sgm / CNT_SEGS), hi_s = (uint32_t)((unsigned long long)qn * (sgm + 1u) / CNT_SEGS);
      const uint32_t lo = (uint32_t)min((unsigned long long)lo_s + (unsigned long long)kth * cwg, (unsigned long long)hi_s), hi = min(lo + cwg, hi_s);
      cursor[8 + p] = sgm;
      pack[p] = (unsigned long long)lo | ((unsigned long long)hi << 32);
      cursor[4 + p] = 0u; cursor[6 + p] = 0u;
    }
  }
  // stage the top of the tree (the pool is stored breadth first: its first ntop elements ARE the top levels); a staged element
  // keeps an 80-byte stride in LDS (PHX_NODE_LDS_BYTES, bvh8.h)
  const uint4* g4 = reinterpret_cast<const uint4*>(sc.pool);
  for (uint32_t i = threadIdx.x; i < ntop * 4u; i += BLOCK) top[(i >> 2) * (PHX_NODE_LDS_BYTES / 16u) + (i & 3u)] = g4[i];
  for (uint32_t i = threadIdx.x; i < PHX_PERM_LUT_BYTES; i += BLOCK) perm_lut[i] = (uint8_t)perm_xor8(i & 0xffu, i >> 8);
  __syncthreads();
  if constexpr (PACKED)
    trace_stream<BLOCK, SPILL, true, UV>(sc, pb, q, cursor, reinterpret_cast<uint2*>(stack_words + threadIdx.x), reinterpret_cast<uint8_t*>(valid_rows + threadIdx.x), levels,
                                     sc.stack_spill + (size_t)blockIdx.x * BLOCK + threadIdx.x, refill_min, top, ntop, dq, perm_lut);
  else
    trace_stream<BLOCK, SPILL, false, UV>(sc, pb, q, cursor, stack + threadIdx.x, nullptr, levels, sc.stack_spill + (size_t)blockIdx.x * BLOCK + threadIdx.x,
                                      refill_min, top, ntop, dq, perm_lut);
}

// stage-level hook (phx_dev_trace): one ray per lane run to completion with the plain traverse8 loop of bvh8.h.  The per-lane
// stack lives in dynamic LDS sized by the depth of the tree (<= PHX_MAX_BVH_DEPTH levels x 256 lanes x 8 B = 128 KB).
template <bool ANY>
__global__ void __launch_bounds__(PHX_BLOCK) k_trace_rays(DevScene sc, uint32_t n, const float4* ro, const float4* rd, float4* hit) {
  extern __shared__ uint2 ray_stack[];
  const uint32_t i = blockIdx.x * PHX_BLOCK + threadIdx.x;
  if (i >= n) return;
  const float4 a = ro[i], b = rd[i];
  LdsStack<0> st{ray_stack + threadIdx.x, 0};
  Hit h;
  traverse8<ANY>(sc.pool, sc.grid, v3(a.x, a.y, a.z), v3(b.x, b.y, b.z), b.w, h, st);
  hit[i] = make_float4(h.t, h.u, h.v, u2f(h.tri == 0xffffffffu ? 0xffffffffu : sc.tris[h.tri].prim));  // primitive in scene_t::triangles() order
}

// ---- primary rays as packets ---------------------------------------------------------------------------------------------------
// The camera rays of a pass are the one coherent launch of a frame: path ids are pixel-major, so the 64 rays of a wave are 64
// samples of ONE pixel (or of a few neighbouring ones when a pass holds fewer than 64 samples per pixel) and walk the same nodes.
// k_trace runs them like any other rays — every lane tests all eight child boxes of every node it visits, ~290 VALU instructions
// per visit, and the launch sits at the ALU cost of that: 12.9 ms of the 72 ms bench frame.  Here a wave walks the tree ONCE for
// its 64 rays: a node is tested against the packet's interval of origins and reciprocal directions — eight lanes, one child box
// each, interval arithmetic on the same slab test — and every lane runs the reference's triangle test on each triangle the packet
// reaches.  The packet's bounds contain what every lane would get from the same expression with its own ray (a product of two intervals
// contains every member's product, rounding included, because rounding is monotonic); k_trace's node_hit8 evaluates the slab
// distances in another order, so the two differ by roundings, which 2^-16 of the distance on both ends is there to cover (node_hit8
// itself pads by 2^-20).  The lanes then meet a superset of the triangles they meet in k_trace, and the closest hit with its
// lowest-primitive tie rule does not depend on which superset (bvh8.h); that the films are identical bit for bit is tested, not assumed
// (EXPERIMENTS.md Part B section 4).  A wave whose rays do not share a direction octant (a pixel on one of the film's axes) falls back to the
// per-lane walk of bvh8.h.
// wave-wide min / max through DPP (four shifts inside the rows of 16, two row broadcasts; the result lands in lane 63): 13 instructions,
// where six __shfl_xor rounds would be twelve trips through the LDS crossbar
template <bool MAX>
__device__ __forceinline__ float wave_reduce_f(float x) {
#define PHX_DPP_STEP(ctrl, rows) { const float t = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, x), __builtin_bit_cast(int, x), ctrl, rows, 0xf, false)); x = MAX ? fmaxf(x, t) : fminf(x, t); }
  PHX_DPP_STEP(0x111, 0xf) PHX_DPP_STEP(0x112, 0xf) PHX_DPP_STEP(0x114, 0xf) PHX_DPP_STEP(0x118, 0xf)  // row_shr:1, 2, 4, 8
  PHX_DPP_STEP(0x142, 0xa) PHX_DPP_STEP(0x143, 0xc)                                                      // row_bcast:15 -> rows 1, 3; row_bcast:31 -> rows 2, 3
#undef PHX_DPP_STEP
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), 63));
}
__device__ __forceinline__ float wave_min_f(float x) { return wave_reduce_f<false>(x); }
__device__ __forceinline__ float wave_max_f(float x) { return wave_reduce_f<true>(x); }
// What a node test needs of the packet, per axis (wave-uniform).  With s = +1 / -1 the common sign of the rays' direction on the axis,
// a ray's slab distance to the plane at c is (s (c - o)) * |1/d|: both factors are monotonic in what varies over the packet, so
//   entry  >=  fma(s, c_near, kn) * (that >= 0 ? bmin : bmax),   kn = -s * (the origin coordinate that makes s (c - o) smallest)
//   exit   <=  fma(s, c_far,  kf) * (that >= 0 ? bmax : bmin),   kf = -s * (the one that makes it largest)
// and, rounding being monotonic, the bounds hold for the rounded values every lane would compute from its own ray.
struct PacketBounds { float s[3], kn[3], kf[3], bmin[3], bmax[3]; };
__device__ __forceinline__ void packet_axis(PacketBounds& B, int a, float o_lo, float o_hi, float ia_lo, float ia_hi /* this lane's rays: origin and |1/d| ranges */,
                                            bool down /* the rays run towards -axis */) {
  const float omin = wave_min_f(o_lo), omax = wave_max_f(o_hi);
  B.bmin[a] = wave_min_f(ia_lo); B.bmax[a] = wave_max_f(ia_hi);
  B.s[a] = down ? -1.0f : 1.0f;
  B.kn[a] = down ? omin : -omax;   // s = -1: s (c - o) = o - c is smallest at omin, and -s * omin = omin
  B.kf[a] = down ? omax : -omin;
}
typedef unsigned int phx_u4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(4))) phx_u4* phx_const_u4p;  // "constant" address space: a wave-uniform address is read through the scalar cache
// bit s of the result: child slot s of the node may be hit by some ray of the packet (every lane returns the same mask)
__device__ __forceinline__ uint32_t packet_node_hit8(const uint32_t* w, const SceneGrid& g, const PacketBounds& B, uint32_t oct_inv, float tmax_wave, uint32_t& valid) {
  float px, py, pz;
  node_origin_decode(w[0], w[1], g, px, py, pz, valid);
  const uint32_t e = w[2];
  const float sx = u32_as_f32((e & 0xffu) << 23), sy = u32_as_f32(((e >> 8) & 0xffu) << 23), sz = u32_as_f32(((e >> 16) & 0xffu) << 23);
  // lane j (mod 8) takes child slot j: byte j of each of the six 8-byte plane rows (one 64-bit shift each; a select between the two
  // words of a row would be turned into an indexed read of w[], i.e. scratch memory)
  const uint32_t sh = (__lane_id() & 7u) * 8u;
  auto plane = [&](int row) { return (float)((uint32_t)((((unsigned long long)w[row + 1] << 32) | (unsigned long long)w[row]) >> sh) & 0xffu); };
  const float lox = fmaf(plane(4), sx, px), hix = fmaf(plane(10), sx, px);
  const float loy = fmaf(plane(6), sy, py), hiy = fmaf(plane(12), sy, py);
  const float loz = fmaf(plane(8), sz, pz), hiz = fmaf(plane(14), sz, pz);
  const bool nx = !(oct_inv & 4u), ny = !(oct_inv & 2u), nz = !(oct_inv & 1u);  // the packet's rays all run down this axis
  const float anx = fmaf(B.s[0], nx ? hix : lox, B.kn[0]), afx = fmaf(B.s[0], nx ? lox : hix, B.kf[0]);
  const float any_ = fmaf(B.s[1], ny ? hiy : loy, B.kn[1]), afy = fmaf(B.s[1], ny ? loy : hiy, B.kf[1]);
  const float anz = fmaf(B.s[2], nz ? hiz : loz, B.kn[2]), afz = fmaf(B.s[2], nz ? loz : hiz, B.kf[2]);
  const float tnx = anx * (anx >= 0.0f ? B.bmin[0] : B.bmax[0]), tfx = afx * (afx >= 0.0f ? B.bmax[0] : B.bmin[0]);
  const float tny = any_ * (any_ >= 0.0f ? B.bmin[1] : B.bmax[1]), tfy = afy * (afy >= 0.0f ? B.bmax[1] : B.bmin[1]);
  const float tnz = anz * (anz >= 0.0f ? B.bmin[2] : B.bmax[2]), tfz = afz * (afz >= 0.0f ? B.bmax[2] : B.bmin[2]);
  float tn = fmaxf(fmaxf(tnx, tny), tnz), tf = fminf(fminf(tfx, tfy), tfz);
  const float pad = 1.52587890625e-05f;  // 2^-16 of the distance on both ends: the lanes' own tests (node_hit8) differ from this one by roundings
  tn = tn - fabsf(tn) * pad; tf = tf + fabsf(tf) * pad;
  const bool hit = tn <= tf && tf >= 0.0f && tn <= tmax_wave;
  return (uint32_t)__ballot(hit) & 0xffu & valid;  // empty slots carry inverted boxes AND are masked out
}

#define PHX_PRIMARY_BLOCK 256
#ifndef PHX_PRIMARY_WAVES
#define PHX_PRIMARY_WAVES 5  /* waves per SIMD the register allocator leaves room for: 95 VGPRs with 4 rays per lane (4: 98; 6: 80 + 48 B of scratch); 3.65 -> 3.35 ms */
#endif
// RPL rays per lane: a packet is 64 x RPL consecutive paths (ray k of lane l is path base + 64 k + l).  The node tests are per packet,
// so they are shared by more rays; the host picks RPL so that a packet stays inside one pixel's samples (launch_trace_primary).
template <int RPL, bool LENS = false /* thin-lens camera: camera_ray<true> */, bool UV = false /* store pb.hit_uv too (k_trace) */>
__global__ void __launch_bounds__(PHX_PRIMARY_BLOCK) __attribute__((amdgpu_waves_per_eu(PHX_PRIMARY_WAVES, 8))) k_trace_primary(DevScene sc, PassBuffers pb, uint32_t npaths, uint32_t sample0, int q, int sq) {
  extern __shared__ uint2 primary_lds[];  // [4 waves x PHX_MAX_BVH_DEPTH] one shared stack per wave, then [levels x 256] per-lane stacks of the fallback walk
  uint2* lane_stacks = primary_lds + (PHX_PRIMARY_BLOCK / 64) * PHX_MAX_BVH_DEPTH;
  if (blockIdx.x == 0 && threadIdx.x == 0) {  // what k_trace does at the start of a step (no shadow rays yet in step 0)
    pb.counters[(q ^ 1) * CNT_STRIDE] = 0; pb.counters[CNT_SHADOW + (sq ^ 1) * CNT_STRIDE] = 0;
    atomicAdd(&pb.stats->rays_closest, (unsigned long long)npaths);
  }
  const uint32_t lane = __lane_id(), wave = threadIdx.x >> 6;
  // (Dealing the workgroups to the XCDs in bands of the image — XCD x the x-th eighth of the packets — is SLOWER here: 3.35 -> 3.76 ms,
  // profiles/r04_o_xcd_primary_ab.log: bands of the image cost differently, and a plain grid has no way to steal.)
  const uint32_t base = (blockIdx.x * (PHX_PRIMARY_BLOCK / 64) + wave) * (64u * RPL);
  if (base >= npaths) return;
  uint32_t idx[RPL];
  RayCtx r[RPL];
  float tbest[RPL], hu[RPL], hv[RPL];
  uint32_t htri[RPL], hprim[RPL];
  bool mixed = false;
#pragma unroll
  for (int k = 0; k < RPL; ++k) {
    idx[k] = base + 64u * k + lane;
    v3 co, cd;
    camera_ray<LENS>(sc, pb, min(idx[k], npaths - 1u), sample0, co, cd);  // rays past the end repeat the last one and write nothing
    r[k] = make_ray_ctx(co, cd);
    tbest[k] = FLT_MAX; hu[k] = 0.0f; hv[k] = 0.0f; htri[k] = 0xffffffffu; hprim[k] = 0;
  }
  const uint32_t oct = PHX_UNI(r[0].oct_inv);
#pragma unroll
  for (int k = 0; k < RPL; ++k) mixed = mixed || r[k].oct_inv != oct;
  if (__ballot(mixed) != 0ull) {
#pragma unroll
    for (int k = 0; k < RPL; ++k) {
      LdsStack<0> st{lane_stacks + threadIdx.x, 0};
      Hit h;
      // a NaN ray (LENS: a lens sample with a zero coordinate) hits nothing, but the conservative box test ignores NaNs: no walk of the whole tree
      if constexpr (LENS) { const float chk = (r[k].o.x + r[k].o.y + r[k].o.z) + (r[k].d.x + r[k].d.y + r[k].d.z); if (!(fabsf(chk) <= FLT_MAX)) continue; }
      traverse8<false>(sc.pool, sc.grid, r[k].o, r[k].d, FLT_MAX, h, st);
      tbest[k] = h.t; htri[k] = h.tri;
      if constexpr (UV) { hu[k] = h.u; hv[k] = h.v; }
    }
#if PHX_COUNT
    if (lane == 0) { atomicAdd(&pb.stats->primary_packets, 1ull); atomicAdd(&pb.stats->primary_fallbacks, 1ull); }
#endif
  } else {
    PacketBounds B;
    {
      v3 olo = r[0].o, ohi = r[0].o, ilo(fabsf(r[0].idx), fabsf(r[0].idy), fabsf(r[0].idz)), ihi = ilo;
#pragma unroll
      for (int k = 1; k < RPL; ++k) {
        olo = v3(fminf(olo.x, r[k].o.x), fminf(olo.y, r[k].o.y), fminf(olo.z, r[k].o.z)); ohi = v3(fmaxf(ohi.x, r[k].o.x), fmaxf(ohi.y, r[k].o.y), fmaxf(ohi.z, r[k].o.z));
        const v3 ia(fabsf(r[k].idx), fabsf(r[k].idy), fabsf(r[k].idz));
        ilo = v3(fminf(ilo.x, ia.x), fminf(ilo.y, ia.y), fminf(ilo.z, ia.z)); ihi = v3(fmaxf(ihi.x, ia.x), fmaxf(ihi.y, ia.y), fmaxf(ihi.z, ia.z));
      }
      packet_axis(B, 0, olo.x, ohi.x, ilo.x, ihi.x, !(oct & 4u)); packet_axis(B, 1, olo.y, ohi.y, ilo.y, ihi.y, !(oct & 2u)); packet_axis(B, 2, olo.z, ohi.z, ilo.z, ihi.z, !(oct & 1u));
    }
    float tmax_wave = FLT_MAX;  // the farthest closest-hit distance of the packet so far
    uint32_t ng_base = 0, ng_hits = 0x80000000u;  // the root as a one-child group (bvh8.h: traverse8)
    uint32_t sp = 0, guard = 0;
#if PHX_COUNT
    uint32_t cnt_nodes = 0, cnt_tris = 0, cnt_lanes = 0;
#endif
    uint2* stack = primary_lds + wave * PHX_MAX_BVH_DEPTH;
    for (;;) {
      if (++guard > PHX_TRACE_WATCHDOG) { if (lane == 0) atomicAdd(&pb.stats->watchdog, 1ull); break; }
      const uint32_t bit = 31u - (uint32_t)__clz((int)ng_hits);
      const uint32_t rest = ng_hits & ~(1u << bit);
      if (rest > 0x00ffffffu) { if (lane == 0) stack[sp] = make_uint2(ng_base, rest); ++sp; }
      const uint32_t slot = (bit - 24u) ^ oct;
      const uint32_t ni = PHX_UNI(ng_base + (uint32_t)__popc(ng_hits & 0xffu & ~(0xffffffffu << slot)));
      uint32_t w[16];
      {
        const phx_const_u4p s4 = (phx_const_u4p)(sc.pool) + (size_t)ni * 4u;  // the pool is never written while a frame runs
#pragma unroll
        for (int k = 0; k < 4; ++k) { const phx_u4 v = s4[k]; w[4 * k] = v.x; w[4 * k + 1] = v.y; w[4 * k + 2] = v.z; w[4 * k + 3] = v.w; }
      }
      uint32_t valid;
#if PHX_COUNT
      ++cnt_nodes;
#endif
      const uint32_t hit8 = packet_node_hit8(w, sc.grid, B, oct, tmax_wave, valid);
      const uint32_t imask = w[2] >> 24;
      ng_base = PHX_UNI(w[3]);
      ng_hits = PHX_UNI((perm_xor8(hit8 & imask, oct) << 24) | valid);
      uint32_t th = PHX_UNI(hit8 & ~imask);
      while (th != 0u) {
        const uint32_t k = 31u - (uint32_t)__clz((int)th);
        th &= ~(1u << k);
        const uint32_t ti = PHX_UNI(ng_base + (uint32_t)__popc(valid & ~(0xffffffffu << k)));
        const phx_const_u4p t4 = (phx_const_u4p)(sc.pool) + (size_t)ti * 4u;
        const phx_u4 t0 = t4[0], t1 = t4[1], t2 = t4[2];
        TriRec T;
        T.v0x = u2f(t0.x); T.v0y = u2f(t0.y); T.v0z = u2f(t0.z); T.e0x = u2f(t0.w);
        T.e0y = u2f(t1.x); T.e0z = u2f(t1.y); T.e1x = u2f(t1.z); T.e1y = u2f(t1.w);
        T.e1z = u2f(t2.x); T.prim = t2.y;
        bool any_better = false;
        float tworst = 0.0f;
#pragma unroll
        for (int m = 0; m < RPL; ++m) {
          float us, vs, ds;
          const bool better = mt_intersect(T, r[m].o, r[m].d, tbest[m], hprim[m], us, vs, ds);
          if (better) { tbest[m] = ds; htri[m] = ti; hprim[m] = T.prim; if constexpr (UV) { hu[m] = us; hv[m] = vs; } }
          any_better = any_better || better;
          tworst = fmaxf(tworst, tbest[m]);
        }
#if PHX_COUNT
        ++cnt_tris; cnt_lanes += (uint32_t)__popcll(__ballot(any_better));
#endif
        if (__ballot(any_better) != 0ull) tmax_wave = wave_max_f(tworst);
      }
      if (ng_hits <= 0x00ffffffu) {
        if (sp == 0u) break;
        --sp;
        const uint2 e = stack[sp];
        ng_base = PHX_UNI(e.x); ng_hits = PHX_UNI(e.y);
      }
    }
#if PHX_COUNT
    if (lane == 0) {
      atomicAdd(&pb.stats->primary_packets, 1ull);
      atomicAdd(&pb.stats->primary_node_tests, (unsigned long long)cnt_nodes);
      atomicAdd(&pb.stats->primary_tri_tests, (unsigned long long)cnt_tris);
      atomicAdd(&pb.stats->primary_tri_lanes_hit, (unsigned long long)cnt_lanes);
    }
#endif
  }
#pragma unroll
  for (int k = 0; k < RPL; ++k)
    if (idx[k] < npaths) {
      pb.hit_tt[idx[k]] = make_uint2(f2u(tbest[k]), htri[k]);
      if constexpr (UV) pb.hit_uv[idx[k]] = make_float2(hu[k], hv[k]);
    }
}

// ---- launches ---------------------------------------------------------------------------------------
namespace {
struct TraceEnv {
  int grid_mul, wg_cap;
  uint32_t refill, block_env, ntop_env, min_chunks, target_chunks, lds_levels_env;
};
const TraceEnv& trace_env() {
  static const TraceEnv e = [] {
    // knobs are experiment switches, but a typo must not become a launch shape the kernels were never built for: negative values
    // fall back to the default and the workgroup size has to be one the kernels are instantiated for
    auto geti = [](const char* n, int d) { const char* v = getenv(n); const int x = v ? atoi(v) : d; return x < 0 ? d : x; };
    TraceEnv t;
    t.refill = (uint32_t)geti("PHX_REFILL", 12); t.grid_mul = std::max(1, geti("PHX_TRACE_DYN_GRID", 1));
    // 1024-thread workgroups: the CU's LDS holds two copies of the top of the tree instead of eight, so each copy is 4x larger
    t.block_env = (uint32_t)geti("PHX_TRACE_BLOCK", 0); t.ntop_env = (uint32_t)geti("PHX_NTOP", 0);
    if (t.block_env != 0 && t.block_env != 256 && t.block_env != 512 && t.block_env != 1024) t.block_env = 0;
    t.lds_levels_env = (uint32_t)geti("PHX_LDS_LEVELS", 0);  // stack levels kept in LDS (0 = chosen by trace_plan)
    if (t.lds_levels_env > PHX_MAX_BVH_DEPTH) t.lds_levels_env = 0;
    if (t.refill < 1 || t.refill > 64) t.refill = 12;
    t.min_chunks = (uint32_t)geti("PHX_MIN_CHUNKS", 8);
    t.wg_cap = geti("PHX_TRACE_WG_CAP", 0);  // experiment: at most this many k_trace workgroups per CU (leaves wave slots to another stream)
    // 64-ray chunks out of a workgroup's range of 16 (k_trace ms per frame at 100 k: 60.8 — with one global atomic per WAVE and
    // chunk the best was 63.7 at 512 rays: 128 rays 75.7, 256 66.7, 384 64.4, 768 63.9, 1024 64.2; profiles/r02_n_knob_sweep.log,
    // r02_o_wg_cursor.log)
    t.target_chunks = (uint32_t)std::max(1, geti("PHX_TARGET_CHUNKS", 1));
    return t;
  }();
  return e;
}
template <typename F>
void for_each_trace_kernel(F&& f) {
  auto both = [&](auto UV) {  // every instantiation launch_trace / launch_trace_primary can pick, with and without the barycentrics
    constexpr bool uv = decltype(UV)::value;
    f(reinterpret_cast<const void*>(&k_trace<256, false, false, uv>)); f(reinterpret_cast<const void*>(&k_trace<512, false, false, uv>)); f(reinterpret_cast<const void*>(&k_trace<1024, false, false, uv>));
    f(reinterpret_cast<const void*>(&k_trace<1024, true, false, uv>)); f(reinterpret_cast<const void*>(&k_trace<1024, true, true, uv>));
    f(reinterpret_cast<const void*>(&k_trace_primary<1, false, uv>)); f(reinterpret_cast<const void*>(&k_trace_primary<2, false, uv>)); f(reinterpret_cast<const void*>(&k_trace_primary<4, false, uv>));
    f(reinterpret_cast<const void*>(&k_trace_primary<1, true, uv>)); f(reinterpret_cast<const void*>(&k_trace_primary<2, true, uv>)); f(reinterpret_cast<const void*>(&k_trace_primary<4, true, uv>));
  };
  both(std::false_type{}); both(std::true_type{});
  f(reinterpret_cast<const void*>(&k_trace_rays<true>)); f(reinterpret_cast<const void*>(&k_trace_rays<false>));
  const void* guides[4];  // guides.hip: k_guides keeps k_trace_rays' per-lane stack
  for (uint32_t k = 0, n = guides_kernels(guides); k < n; ++k) f(guides[k]);
}
}  // namespace

bool launch_counts_traversal_work() { return PHX_COUNT != 0; }

// Allow every traversal kernel the CU's full 160 KB of LDS as dynamic shared memory ON THE CURRENT DEVICE.  The attribute is
// per device and per kernel, so the host calls this once for each phx_device it makes (device.cpp: phx_dev_make).
hipError_t init_kernels_on_current_device() {
  hipError_t rc = hipSuccess;
  for_each_trace_kernel([&](const void* k) {
    const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess && rc == hipSuccess) rc = e;
  });
  return rc;
}

// k_trace addresses the pool with 32-bit byte offsets (trace_stream: pool_elem) in every instantiation but <1024, SPILL, unpacked>, which keeps
// 64-bit addresses: a pool of 2^26 elements or more (4 GB) runs that one whatever its depth (with every level in LDS it never touches the spill
// area, and such a pool is never packed: PHX_STACK_PACKED needs < 2^24 elements)
static bool trace_pool_is_wide(const DevScene& sc) { return sc.num_elems >= (1u << 26); }

// What a k_trace launch on this scene looks like: workgroup size, nodelets staged in LDS, stack levels, LDS bytes.
TracePlan trace_plan(const DevScene& sc) {
  const TraceEnv& E = trace_env();
  TracePlan P{};
  // stack entries needed = BVH depth - 1: one pending sibling group per level above the deepest node (the root "group" has a
  // single member and the deepest nodes have no inner children); tests/test_host_bvh8.py checks the bound
  P.levels = std::max(2u, sc.stack_levels > 1u ? sc.stack_levels - 1u : 1u);
  // ... of which the top lds_levels live in LDS and the rest in HBM (k_trace<1024, SPILL>).  A lane's stack is rarely deep
  // (100 k triangles, 8 levels: 6.5 pushes per ray, 0.011 of them land at depth 5 or below; 1 M, 9 levels: 0.013 at depth 6 or
  // below), but the test on every push and pop costs what the freed LDS buys back on trees whose stacks fit (profiles/README.md):
  // spilling is for trees so deep that the stacks alone would force smaller workgroups and fewer resident waves.
  P.lds_levels = P.levels;
  if (!E.block_env) {
    const uint32_t want = E.lds_levels_env ? E.lds_levels_env : (P.levels >= PHX_SPILL_FROM_LEVELS ? PHX_SPILL_LDS_LEVELS : P.levels);
    P.lds_levels = std::max(2u, std::min(P.levels, want));
  }
  const bool spill = P.lds_levels < P.levels;
  const bool wide = trace_pool_is_wide(sc);
  // nodelets staged in LDS: whatever the per-lane stacks leave of the workgroup's share of the CU's 160 KB at full occupancy
  // (32 waves per CU); 9 (root + one level) when the stacks alone do not fit, and occupancy then follows from the LDS
  // 5-byte stack entries (PHX_STACK_PACKED): for the SPILL plan, when the pool's indices fit 24 bits
  P.packed = PHX_STACK_PACKED && spill && sc.num_elems < (1u << 24) ? 1u : 0u;
  auto stack_bytes = [&](uint32_t lv, uint32_t blk) { return P.packed ? (lv + ((lv + 3u) >> 2)) * blk * 4u : lv * blk * 8u; };
  auto plan = [&](uint32_t blk, uint32_t& ntop_out, uint32_t& lds_out) {  // -> workgroups per CU for this block size
    uint32_t ntop_req = E.ntop_env;
    if (!ntop_req) {
      const uint32_t share = 160u * 1024u / (2048u / blk), stacks = stack_bytes(P.lds_levels, blk) + 48u + PHX_PERM_LUT_BYTES;
      ntop_req = share > stacks + 9u * PHX_NODE_LDS_BYTES ? (share - stacks) / PHX_NODE_LDS_BYTES : 9u;
    }
    ntop_out = std::min(ntop_req, sc.num_elems);
    lds_out = ntop_out * PHX_NODE_LDS_BYTES + stack_bytes(P.lds_levels, blk) + 48u + PHX_PERM_LUT_BYTES;
    return std::min(160u * 1024u / lds_out, 2048u / blk);
  };
  // 1024-thread workgroups share one copy of the staged nodelets among 16 waves; a deep tree (levels >= 10: the stacks alone
  // exceed the CU's LDS at full occupancy) is better served by smaller workgroups, whose LDS granularity wastes less
  P.block = E.block_env && !wide ? E.block_env : 1024u;
  if (E.block_env || spill || wide) P.wg_per_cu = plan(P.block, P.ntop, P.lds_bytes);  // spilling exists for 1024-thread workgroups only
  else {
    uint32_t best_waves = 0;
    for (uint32_t blk = 1024u; blk >= 256u; blk >>= 1) {
      uint32_t nt, l; const uint32_t wgs = plan(blk, nt, l);
      if (wgs * (blk / 64u) > best_waves) { best_waves = wgs * (blk / 64u); P.block = blk; P.ntop = nt; P.lds_bytes = l; P.wg_per_cu = wgs; }
    }
  }
  if (E.wg_cap > 0 && P.wg_per_cu > (uint32_t)E.wg_cap) P.wg_per_cu = (uint32_t)E.wg_cap;
  if (P.wg_per_cu == 0) P.wg_per_cu = 1;  // deeper than the LDS can hold even with 256 threads: the launch will report the error
  P.spill_threads = spill ? sc.num_cus * P.wg_per_cu * (uint32_t)E.grid_mul * P.block : 0u;
  return P;
}

void launch_trace(hipStream_t stream, const DevScene& sc, const PassBuffers& pb, int q, int sq, int do_closest, int do_shadow, uint32_t capacity) {
  const TraceEnv& E = trace_env();
  const TracePlan P = trace_plan(sc);
  const uint32_t block = P.block, ntop = P.ntop, lds = P.lds_bytes, levels = P.lds_levels;
  uint32_t grid = sc.num_cus * P.wg_per_cu * (uint32_t)E.grid_mul;  // persistent: the resident workgroups
  const uint32_t need = (((capacity + block - 1) / block + 7u) / 8u) * 8u;
  grid = std::max(8u, std::min(grid, need));
  const dim3 g(grid), b(block);
  auto go = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, g, b, lds, stream, sc, pb, q, sq, do_closest, do_shadow, E.refill, ntop, levels, E.min_chunks, E.target_chunks);
  };
  // UV: the pass has a barycentrics stream exactly when the committed scene reads them (scene_commit.cpp), so its presence picks the instantiation
  with_flag(pb.hit_uv != nullptr, [&](auto UV) {
    constexpr bool uv = decltype(UV)::value;
    if (P.lds_levels < P.levels || trace_pool_is_wide(sc)) { if (P.packed) go(&k_trace<1024, true, true, uv>); else go(&k_trace<1024, true, false, uv>); }  // deep tree: 1024-thread workgroups, the stack's deep levels in HBM
    else if (block == 256) go(&k_trace<256, false, false, uv>);
    else if (block == 512) go(&k_trace<512, false, false, uv>);
    else go(&k_trace<1024, false, false, uv>);
  });
}
void launch_trace_primary(hipStream_t stream, const DevScene& sc, const PassBuffers& pb, uint32_t npaths, uint32_t sample0, int q, int sq) {
  static const int rpl_env = [] { const char* v = getenv("PHX_PRIMARY_RPL"); return v ? atoi(v) : 0; }();  // experiment: 1, 2 or 4 rays per lane
  const size_t lds = ((size_t)std::max(2u, std::min(sc.stack_levels, (uint32_t)PHX_MAX_BVH_DEPTH)) * PHX_PRIMARY_BLOCK + (PHX_PRIMARY_BLOCK / 64) * PHX_MAX_BVH_DEPTH) * sizeof(uint2);
  // path ids are pixel-major (pixel * samples_of_this_pass + sample): 256 consecutive paths are samples of ONE pixel when the pass holds
  // a multiple of 256 samples per pixel; otherwise 128 paths, i.e. the samples of a few pixels next to each other in a tile row
  // (measured, profiles/r03_zo_primary_packets.log: 4 rays per lane beat 2 only inside one pixel; 2 beat 1 from 16 samples per pixel up)
  uint32_t rpl = pb.num_samples % 256u == 0 ? 4u : pb.num_samples >= 16u ? 2u : 1u;
  if (rpl_env == 1 || rpl_env == 2 || rpl_env == 4) rpl = (uint32_t)rpl_env;
  const dim3 g((npaths + PHX_PRIMARY_BLOCK * rpl - 1) / (PHX_PRIMARY_BLOCK * rpl)), b(PHX_PRIMARY_BLOCK);
  // thin lens: the rays of a packet leave from a disc, not a point (the packet's bounds know origins apart)
  with_flag(sc.aperture_radius != 0.0f, [&](auto LENS) {
    with_flag(pb.hit_uv != nullptr, [&](auto UV) {  // (launch_trace: the barycentrics stream exists when the scene reads them)
      auto go = [&](auto RPL) { hipLaunchKernelGGL((k_trace_primary<decltype(RPL)::value, decltype(LENS)::value, decltype(UV)::value>), g, b, lds, stream, sc, pb, npaths, sample0, q, sq); };
      if (rpl == 4) go(std::integral_constant<int, 4>{}); else if (rpl == 2) go(std::integral_constant<int, 2>{}); else go(std::integral_constant<int, 1>{});
    });
  });
}
void launch_trace_rays(hipStream_t stream, const DevScene& sc, uint32_t n, const float4* ro, const float4* rd, float4* hit, int any) {
  const dim3 g(blocks_for(n)), b(PHX_BLOCK);
  const size_t lds = (size_t)std::max(2u, std::min(sc.stack_levels, (uint32_t)PHX_MAX_BVH_DEPTH)) * PHX_BLOCK * sizeof(uint2);
  if (any) hipLaunchKernelGGL((k_trace_rays<true>), g, b, lds, stream, sc, n, ro, rd, hit);
  else hipLaunchKernelGGL((k_trace_rays<false>), g, b, lds, stream, sc, n, ro, rd, hit);
}

}  // namespace phx
