// Body-mounted ray sensors of a batch (mgf_batch_set_sensors, mgf_batch_cast_sensors, mgf_batch_cast_sensors_dev; host_batch_sensor.inc).
// (Part of the kernel set described in kernels.h.)
//
// A sensor is a ray fixed in the frame of a body: (world, body, p, d, dt, flags).  Its particle in world coordinates is
//   P = x + rotate(q, p)      D = rotate(q, d)      dt unchanged
// with x and q the body's rows as mgf_batch_read_state returns them (x WITHOUT delta: the pose the last tick built the collider of, the
// one a query sees), rotate dev_math.h's (Rotation::rotate_vector), the sum a plain V3 add, every operation a separate f32 one.  Its
// answer is what k_batch_query_ray writes for that particle against that world, with `body` ignored if MGF_SENSOR_IGNORE_SELF is set.
//   k_batch_sensor_ray   a workgroup per work item of the rig's table - built on the host when the rig is set (BatchQueryPlan: a world's
//                        sensors in the caller's order, up to 256 an item) - and k_batch_query_ray's work split: the world's col0 / col1
//                        staged in dynamic LDS, 256 / (count rounded up to a power of two) lanes a sensor.  What differs is where the
//                        particle comes from: every live lane loads its sensor's record and the body's x and q and forms P and D.
//                        Then bq_ray_item's loop, unchanged - bq_ray_far, q_ray_comp, QueryBest::offer, bq_reduce - and the sensor's
//                        first lane walks the terrain, stores the hit and, where there is somewhere to store it, the particle
// The obstacles are k_batch_query_ray_obstacles' (k_batch_query.h), unchanged, over the stored particles and the rig's worlds.
// The front is this kernel's own and not a fourth SRC of bq_ray_item: that template's kernels stay as they are, instruction for
// instruction.  As there, no lane leaves ahead of a __syncthreads: the only exit is behind bq_reduce.
#pragma once
#include "k_batch_query.h"

namespace mgf {

struct SensorIn { int32_t world, body; float p[3], d[3], dt; int32_t flags; };  // mgf_batch_sensor
static_assert(sizeof(SensorIn) == 40, "the rig goes up as the caller's records");

// BatchQueryArgs' `ignore` is not read: a sensor's ignore value follows from its record
struct BatchSensorArgs : BatchQueryArgs {
  const float4* x;      // the bodies' rows (Bodies::x, ::q), world k's at [w_off[k], w_off[k + 1])
  const float4* q;
  const SensorIn* rig;  // by the caller's index; world and body checked on the host: world = the work item's, body < the world's length
  float* parts;         // by the caller's index: 7 words a sensor (mgf_particle); null: not stored
};

// LDS (dynamic): 32 bytes a body, kBatchQueryRed words - as k_batch_query_ray.
__global__ __launch_bounds__(kBatchBlock) void k_batch_sensor_ray(BatchSensorArgs A) {
  extern __shared__ float4 s_dyn[];
  BatchWork W(A, A.mask & MGF_QUERY_BODIES);
  const uint32_t n = W.n;
  float4 *s_c0 = s_dyn, *s_c1 = s_dyn + n, *s_red = s_dyn + 2 * (size_t)n;
  bq_stage(A, W.g0, n, s_c0, s_c1);
  W.split(A, W.shift());
  const uint32_t qi = W.qi;
  V3 p = mk3(0.0f, 0.0f, 0.0f), d = p;
  float dt = 0.0f;
  int32_t ign = -1, mask = 0;
  if (W.live) {
    const SensorIn s = A.rig[qi];
    const size_t g = (size_t)W.g0 + (uint32_t)s.body;
    const float4 bx = A.x[g], bq = A.q[g];
    const Quat rot = mkq(bq.x, mk3(bq.y, bq.z, bq.w));
    p = xyz(bx) + rotate(rot, ld3(s.p)); d = rotate(rot, ld3(s.d)); dt = s.dt;
    ign = (s.flags & MGF_SENSOR_IGNORE_SELF) ? s.body : -1;
    mask = A.mask;
    if (d.x == 0.0f && d.y == 0.0f && d.z == 0.0f) mask = 0;  // (no direction: no hit, by definition - k_query_ray)
  }
  QueryBest best;
  if (mask & MGF_QUERY_BODIES) {
    const float dd = dot(d, d);
    for (uint32_t i = W.sub; i < n; i += W.L) {
      if ((int32_t)i == ign) continue;
      const float4 a = s_c0[i], b = s_c1[i];
      if (bq_ray_far(a, b, p, d, dd, dt)) continue;
      V3 ip; float t;
      if (q_ray_comp(p, d, dt, a, b, &ip, &t)) best.offer(ip, t, MGF_HIT_BODY, i, 0u);
    }
  }
  bq_reduce(best, W, s_red);
  if (W.sub != 0u || !W.live) return;
  if (mask & MGF_QUERY_TERRAIN) {
    const BatchTerrain M = batch_terrain_of(A.T, W.it.x);  // (the work item's world: wave-uniform loads)
    if (M.n_nodes) q_ray_terrain(M, p, d, dt, nullptr, best);
  }
  q_ray_store(A.out + 7 * (size_t)qi, best);
  if (A.parts) {
    float* o = A.parts + 7 * (size_t)qi;
    o[0] = p.x; o[1] = p.y; o[2] = p.z; o[3] = d.x; o[4] = d.y; o[5] = d.z; o[6] = dt;
  }
}

}  // namespace mgf
