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
//                           world's feelers in the caller's order, up to 256 an item, 256 / next_pow2(count) lanes a feeler).  The
//                           world's colliders staged as bq_stage does - whatever the mask: an OWN_SHAPE feeler reads its body's - then
//                           every live lane loads its record and the body's x and q and forms C; the walk over the bodies is
//                           bq_sweep_item's (q_sweep_far, then comp_mcomp, then SweepBest::offer), the reduction bq_reduce; the feeler's
//                           first lane stores the hit (q_sweep_store) and, always, C - into the caller's array or the handle's
// bq_sweep_item itself stays as it is: k_batch_query_sweep_bodies and its _dev forms keep their register figures (tests/util.py), so
// the loop over the bodies stands here a second time, in bf_sweep_front - a front with a loader, as bq_ray_front is.
// The terrain faces and the obstacles are k_batch_query_sweep_faces' / _sweep_obstacles' (k_batch_query.h), unchanged, over the stored
// casts and the rig's worlds.  Every exit and every barrier is bf_sweep_front's: the loader and the store below hold neither.
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

// A live feeler's cast in world coordinates and the body of its world it does not meet (-1: none): what a loader hands bf_sweep_front
struct BatchCast { MovingIn m; int32_t ign; };

// A workgroup's work item of casts formed by a loader - load(qi, g0, s_c0, s_c1) -> BatchCast, run by the live lanes behind the
// staging - and what else a cast's first lane does behind the stored hit - done(qi, m).  Neither holds a barrier nor leaves the kernel.
// The colliders are staged whatever the mask (the loader may read them); the bodies are walked where the mask asks for them.
// The only exit is behind bq_reduce: a whole workgroup reaches both barriers.
template <class Load, class Done>
__device__ __forceinline__ void bf_sweep_front(const BatchQueryArgs& A, float4* s_dyn, Load&& load, Done&& done) {
  BatchWork W(A, true);
  const uint32_t n = W.n;
  float4 *s_c0 = s_dyn, *s_c1 = s_dyn + n, *s_red = s_dyn + 2 * (size_t)n;
  bq_stage(A, W.g0, n, s_c0, s_c1);
  W.split(A, W.shift());
  const uint32_t qi = W.qi;
  SweepBest best;
  BatchCast c;
  if (W.live) {
    c = load(qi, W.g0, s_c0, s_c1);
    if (A.mask & MGF_QUERY_BODIES) {
      const SweepCast K = bq_sweep_cast(c.m);
      const int32_t ign = c.ign;
      for (uint32_t i = W.sub; i < n; i += W.L) {
        if ((int32_t)i == ign) continue;
        const Comp t = to_comp(s_c0[i], s_c1[i]);
        if (q_sweep_far(t, K)) continue;
        Contact k;
        if (comp_mcomp(t, K.s, K.v, &k)) best.offer(k, MGF_HIT_BODY, i, 0u, 0u);
      }
    }
  }
  bq_reduce(best, W, s_red);
  if (W.sub != 0u || !W.live) return;
  q_sweep_store(A.out + 13 * (size_t)qi, best);
  done(qi, c.m);
}

// LDS (dynamic): 32 bytes a body, kBatchQueryRed words - as k_batch_query_sweep_bodies.
__global__ __launch_bounds__(kBatchBlock) void k_batch_feeler_bodies(BatchFeelerArgs A) {
  extern __shared__ float4 s_dyn[];
  bf_sweep_front(
      A, s_dyn,
      [&](uint32_t qi, uint32_t g0, const float4* s_c0, const float4* s_c1) {
        const FeelerIn f = A.rig[qi];
        const size_t g = (size_t)g0 + (uint32_t)f.body;
        const float4 bx = A.x[g], bq = A.q[g];
        const Quat rot = mkq(bq.x, mk3(bq.y, bq.z, bq.w));
        BatchCast c;
        V3 P, D;
        if (f.flags & MGF_FEELER_OWN_SHAPE) {  // (k_pack_colliders' words)
          const float4 a = s_c0[f.body], b = s_c1[f.body];
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

}  // namespace mgf
