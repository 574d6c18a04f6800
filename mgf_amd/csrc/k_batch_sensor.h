// Body-mounted ray sensors of a batch (mgf_batch_set_sensors, mgf_batch_cast_sensors, mgf_batch_cast_sensors_dev; host_batch_sensor.inc).
// (Part of the kernel set described in kernels.h.)
//
// A sensor is a ray fixed in the frame of a body: (world, body, p, d, dt, flags).  Its particle in world coordinates is
//   P = x + rotate(q, p)      D = rotate(q, d)      dt unchanged
// with x and q the body's rows as mgf_batch_read_state returns them (x WITHOUT delta: the pose the last tick built the collider of, the
// one a query sees), rotate dev_math.h's (Rotation::rotate_vector), the sum a plain V3 add, every operation a separate f32 one.  Its
// answer is what k_batch_query_ray writes for that particle against that world, with `body` ignored if MGF_SENSOR_IGNORE_SELF is set.
//   k_batch_sensor_ray   a workgroup per work item of the rig's table - built on the host when the rig is set (BatchQueryPlan: a world's
//                        sensors in the caller's order, up to 256 an item) - through bq_ray_front (k_batch_query.h), the front of
//                        k_batch_query_ray: the staging, the lanes a sensor gets, the loop over the bodies, the reduction, the terrain
//                        walk and the stored hit are that function's, written once.  What is here is where the particle comes from -
//                        every live lane loads its sensor's record and the body's x and q and forms P and D - and, behind the hit, the
//                        particle stored by the sensor's first lane where there is somewhere to store it
// The obstacles are k_batch_query_ray_obstacles' (k_batch_query.h), unchanged, over the stored particles and the rig's worlds.
// Every exit and every barrier is bq_ray_front's: the loader and the store below hold neither.
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

// A work item of the rig's table through bq_ray_front, over either policy of the bodies: the loader that forms a sensor's particle,
// and the particle stored behind the hit where there is somewhere to store it
template <class Bodies>
__device__ __forceinline__ void bs_rays(const BatchSensorArgs& A, Bodies bodies, float4* s_dyn) {
  bq_ray_front<kItemTable>(
      A, bodies, BatchItemSrc(), s_dyn,
      [&](uint32_t qi, uint32_t g0) {
        const SensorIn s = A.rig[qi];
        const size_t g = (size_t)g0 + (uint32_t)s.body;
        const float4 bx = A.x[g], bq = A.q[g];
        const Quat rot = mkq(bq.x, mk3(bq.y, bq.z, bq.w));
        return BatchRay{xyz(bx) + rotate(rot, ld3(s.p)), rotate(rot, ld3(s.d)), s.dt, (s.flags & MGF_SENSOR_IGNORE_SELF) ? s.body : -1};
      },
      [&](uint32_t qi, V3 p, V3 d, float dt) {
        if (A.parts) {
          float* o = A.parts + 7 * (size_t)qi;
          o[0] = p.x; o[1] = p.y; o[2] = p.z; o[3] = d.x; o[4] = d.y; o[5] = d.z; o[6] = dt;
        }
      });
}

// LDS (dynamic): 32 bytes a body, kBatchQueryRed words - as k_batch_query_ray.
__global__ __launch_bounds__(kBatchBlock) void k_batch_sensor_ray(BatchSensorArgs A) {
  extern __shared__ float4 s_dyn[];
  bs_rays(A, PlainBodies(A), s_dyn);
}

}  // namespace mgf
