// Body-mounted feelers of a batch (mgf_batch_set_feelers, mgf_batch_cast_feelers, mgf_batch_cast_feelers_dev; host_batch_feeler.inc).
// (Part of the kernel set described in kernels.h.)
//
// A feeler is a sphere or capsule with a displacement, fixed in the frame of a body: (world, body, tag, flags, p, d, r, delta).  With x
// and q the body's rows as mgf_batch_read_state returns them (x WITHOUT delta: the pose the sensors use) its cast C is
//   shape   MGF_FEELER_OWN_SHAPE: the body's resident collider as it stands (what mgf_batch_read_colliders packs: col0 / col1)
//           else: tag and r the record's, P = x + rotate(q, p), D = rotate(q, d) whatever the tag
//   delta   MGF_FEELER_WORLD_DELTA: the record's; else rotate(q, delta)
// rotate dev_math.h's (Rotation::rotate_vector), the sum a plain V3 add, every operation a separate f32 one - as k_batch_sensor_ray
// forms its particle.  Its answer is what k_batch_query_sweep_bodies (and the two passes behind it) write for C against that world, with
// `body` ignored if MGF_FEELER_IGNORE_SELF is set.
//   k_batch_feeler_bodies   a workgroup per work item of the rig's table - built on the host when the rig is set (BatchQueryPlan: a
//                           world's feelers in the caller's order, up to 256 an item, 256 / next_pow2(count) lanes a feeler) - through
//                           bq_sweep_front (k_batch_query.h), the front of k_batch_query_sweep_bodies: the staging, the lanes a feeler
//                           gets, the walk over the bodies (q_sweep_far, then comp_mcomp, then SweepBest::offer), the reduction and the
//                           stored hit (q_sweep_store) are that function's, written once.  What is here is where the cast comes from -
//                           every live lane loads its record and the body's x and q and forms C - and, behind the hit, C stored by
//                           the feeler's first lane - always, into the caller's array or the handle's
// The terrain faces and the obstacles are k_batch_query_sweep_faces' / _sweep_obstacles' (k_batch_query.h), unchanged, over the stored
// casts and the rig's worlds.  Every exit and every barrier is bq_sweep_front's: the loader and the store below hold neither.
#pragma once
#include "k_batch_query.h"

namespace mgf {

struct FeelerIn { int32_t world, body, tag, flags; float p[3], d[3], r, delta[3]; int32_t reserved[2]; };  // mgf_batch_feeler
static_assert(sizeof(FeelerIn) == 64, "the rig goes up as the caller's records");

// BatchQueryArgs' `ignore` and `T` are not read: a feeler's ignore value follows from its record, the terrain is a later pass's
struct BatchFeelerArgs : BatchQueryArgs {
  const float4* x;       // the bodies' rows (Bodies::x, ::q), world k's at [w_off[k], w_off[k + 1])
  const float4* q;
  const FeelerIn* rig;   // by the caller's index; world, body, tag and flags checked on the host
  MovingIn* casts;       // by the caller's index: 11 words a feeler (mgf_moving_component); never null
};

// A work item of the rig's table through bq_sweep_front, over either policy of the bodies (k_batch_feeler_bodies, and its part-aware
// form in k_batch_part_query.h): the loader that forms a feeler's cast, and the cast stored behind the hit.  MGF_FEELER_OWN_SHAPE: the
// body's collider row as mgf_batch_read_colliders packs it, read from col0 / col1 themselves, not from the staged rows - a mask without
// bodies stages none, and the part rows stage a reject sphere, which is no shape of the body (for a body of several parts the row is
// a radius-0 sphere at the centre of mass).
template <class Bodies>
__device__ __forceinline__ void bf_casts(const BatchFeelerArgs& A, Bodies bodies, float4* s_dyn) {
  bq_sweep_front<kItemTable>(
      A, bodies, BatchItemSrc(), s_dyn,
      [&](uint32_t qi, uint32_t g0) {
        const FeelerIn f = A.rig[qi];
        const size_t g = (size_t)g0 + (uint32_t)f.body;
        const float4 bx = A.x[g], bq = A.q[g];
        const Quat rot = mkq(bq.x, mk3(bq.y, bq.z, bq.w));
        BatchCast c;
        V3 P, D;
        if (f.flags & MGF_FEELER_OWN_SHAPE) {  // (k_pack_colliders' words)
          const float4 a = A.col0[g], b = A.col1[g];
          c.m.tag = (int)f2u(b.w); c.m.r = a.w;
          P = xyz(a); D = xyz(b);
        } else {
          c.m.tag = f.tag; c.m.r = f.r;
          P = xyz(bx) + rotate(rot, ld3(f.p)); D = rotate(rot, ld3(f.d));
        }
        const V3 v = (f.flags & MGF_FEELER_WORLD_DELTA) ? ld3(f.delta) : rotate(rot, ld3(f.delta));
        c.m.p[0] = P.x; c.m.p[1] = P.y; c.m.p[2] = P.z;
        c.m.d[0] = D.x; c.m.d[1] = D.y; c.m.d[2] = D.z;
        c.m.delta[0] = v.x; c.m.delta[1] = v.y; c.m.delta[2] = v.z;
        c.ign = (f.flags & MGF_FEELER_IGNORE_SELF) ? f.body : -1;
        return c;
      },
      [&](uint32_t qi, const MovingIn& m) { A.casts[qi] = m; });
}

// LDS (dynamic): 32 bytes a body, kBatchQueryRed words - as k_batch_query_sweep_bodies.
__global__ __launch_bounds__(kBatchBlock) void k_batch_feeler_bodies(BatchFeelerArgs A) {
  extern __shared__ float4 s_dyn[];
  bf_casts(A, PlainBodies(A), s_dyn);
}

}  // namespace mgf
