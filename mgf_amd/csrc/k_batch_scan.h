// The sensor trace of a rollout (mgf_batch_rollout_observe, mgf_batch_rollout_observe_dev; host_batch_scan.inc): row t of the ray
// sensors' answers written behind tick t, inside the step's launch train.  (Part of the kernel set described in kernels.h.)
//
// The call is defined by the loop  actuate_dev(u[t]) | step(1) | gather_state_dev(row t) | [read_touches_dev(row t)] |
// cast_sensors_dev(mask, row t)  and these two launches ride in the train behind k_batch_rollout_record and the touch trace's launch
// (k_batch_rollout.h, k_batch_trace.h), so that act[k] is final when it is read here.
// NO COLLIDER GATHER: k_batch_query_gather copies words 0 and 3 of bpk, the tick's packed copy of the bodies, into col0 / col1.
// Behind tick t's k_batch_solve, bpk IS what that gather would copy for a world that completed tick t, and x / q are the rows
// cast_sensors_dev would read.  So the cast stages straight from bpk.
//   k_batch_scan_rays         bs_rays (k_batch_sensor.h) - the sensors' loader, bq_ray_front's staging split, walk, reduction, terrain
//                             walk and stores, each written once - over a third policy of the bodies: TickBodies, which is PlainBodies
//                             whose staging reads bpk[4 g] and bpk[4 g + 3] where bq_stage reads col0[g] and col1[g].  It writes the
//                             full hit and the particle into the handle's scratch (7 words a sensor each), never into the caller's
//                             rows.  UNGATED: in a pass that runs tick t again it also casts for the worlds that are not at tick t.
//                             That reads resident, finite data - bpk, x, q of a world that sits undone or finished - through loops
//                             bounded by body and node counts, and nobody reads what it wrote for them (the rows' gate, below).
//                             A gate would have to stand inside bq_ray_front, which stays as it is.  The cost is a pass's worth of
//                             casts per capacity re-run; that cost is not measured (the timed windows have no re-run).
//   k_batch_scan_rows<FORMAT> a lane per sensor in the caller's order, no barrier and no LDS.  Sensor i's world k is the rig's `worlds`
//                             section, the one k_batch_query_ray_obstacles is given by a cast.  The gate is k_batch_rollout_record's
//                             and k_batch_trace_touch's, for the reasons in their headers:
//                               on = done[k] == t + 1 && act[k] <= t + 1     world k completed tick t in THIS pass
//                             and it matters all the more here: TickUndo puts x and q of an undone world back but NOT bpk, so the
//                             scratch of a world that sits undone at tick t holds a cast of tick t - 1's poses against tick t's
//                             colliders.  A lane that is off stores nothing.  A lane that is on takes the scratch record up
//                             (q_ray_load), runs - where the mask asks for obstacles and the batch has any (`obstacles`, uniform) -
//                             k_batch_query_ray_obstacles' body over its world's obstacles with the stored particle, the
//                             zero-direction rule included, and stores entry t * n_sensor + i of the caller's rows: the seven words
//                             of mgf_ray_hit (MGF_ROLLOUT_SENSOR_HIT), or one f32 (MGF_ROLLOUT_SENSOR_DEPTH) - the hit's t, or the
//                             particle's dt where nothing is hit (k_batch_camera_depth's rule).  These are its only global stores.
// The hit record of the scratch is written by the first lane of every sensor of every work item in every launch (bq_ray_front stores a
// no-hit record too), so a row never reads scratch of an earlier tick.
// -DMGF_SCAN_GATE=0 compiles the rows' gate to `true` (tools/build_variant.sh): the build that shows the capacity re-run test of
// tests/test_gpu_world_batch_scan.py catching a row written from the wrong tick (Rollout sensor traces).
#pragma once
#include "k_batch_sensor.h"

#ifndef MGF_SCAN_GATE
#define MGF_SCAN_GATE 1
#endif

namespace mgf {

constexpr int kScanHit = 0, kScanDepth = 1;  // MGF_ROLLOUT_SENSOR_HIT / _DEPTH

// the bodies of a work item's world as tick t built them: PlainBodies over bpk words 0 and 3
struct TickBodies : PlainBodies {
  const float4* bpk;
  __device__ __forceinline__ TickBodies(const BatchWorkArgs& a, const float4* pk) : PlainBodies(a), bpk(pk) {}
  __device__ __forceinline__ void stage(uint32_t g0, uint32_t n, float4* s_dyn) {
    for (uint32_t i = threadIdx.x; i < n; i += kBatchBlock) { s_dyn[i] = bpk[4 * ((size_t)g0 + i)]; s_dyn[n + i] = bpk[4 * ((size_t)g0 + i) + 3]; }
    __syncthreads();
    c0 = s_dyn; c1 = s_dyn + n;
  }
};

// LDS (dynamic): 32 bytes a body, kBatchQueryRed words - as k_batch_sensor_ray.  A.out / A.parts: the handle's scratch; A.col0 / A.col1 are not read.
__global__ __launch_bounds__(kBatchBlock) void k_batch_scan_rays(BatchSensorArgs A, const float4* bpk) {
  extern __shared__ float4 s_dyn[];
  bs_rays(A, TickBodies(A, bpk), s_dyn);
}

struct BatchScanRowsArgs {
  const int32_t* hits;      // the scratch k_batch_scan_rays wrote: 7 words a sensor, by the caller's index
  const ParticleIn* parts;  // ... and the particles
  const int32_t* worlds;    // sensor i's world (the rig's `worlds` section)
  BatchObstacles O;
  const uint4* tdesc;
  const uint32_t* done;     // ticks of this call world k has completed (BatchArgs::done)
  const uint32_t* act;      // ticks whose actuation world k has behind it, final behind k_batch_rollout_record
  void* out;                // row 0 of the caller's trace
  uint32_t tick, n_sensor, obstacles;
};

template <int FORMAT>
__global__ __launch_bounds__(kBatchBlock) void k_batch_scan_rows(BatchScanRowsArgs A) {
  const uint32_t i = blockIdx.x * kBatchBlock + threadIdx.x, t = A.tick;
  const bool in = i < A.n_sensor;
  const uint32_t k = in ? (uint32_t)A.worlds[i] : 0u;
  const bool on = in && (!MGF_SCAN_GATE || (A.done[k] == t + 1u && A.act[k] <= t + 1u));  // the tick gate, a lane's own
  if (on) {
    const ParticleIn q = A.parts[i];
    QueryBest best = q_ray_load(A.hits + 7 * (size_t)i);
    if (A.obstacles) {
      const uint32_t obst = A.tdesc[2 * (size_t)k + 1].w, ob0 = batch_obst_first(obst), ob1 = ob0 + batch_obst_count(obst);
      if (q_ray_castable(ld3(q.d))) {  // (no direction, or one outside the band: no hit, by definition - k_query.h)
#pragma unroll 1
        for (uint32_t e = ob0; e < ob1; ++e) q_ray_obstacle(batch_obstacle_of(A.O, e), e - ob0, q, nullptr, best);
      }
    }
    const size_t at = (size_t)t * A.n_sensor + i;  // row t, the caller's index
    if (FORMAT == kScanDepth) static_cast<float*>(A.out)[at] = best.have ? best.t : q.dt;
    else q_ray_store(static_cast<int32_t*>(A.out) + 7 * at, best);
  }
}

}  // namespace mgf
