// Box zones of a batch: the count and the first k bodies of every box, a fixed-width record (mgf_batch_set_zones, mgf_batch_read_zones,
// mgf_batch_read_zones_dev, mgf_batch_overlap_first_dev; host_batch_zone.inc).  (Part of the kernel set described in kernels.h.)
//
// A zone is an axis-aligned box whose centre is fixed in the frame of a body, or in the world: (world, body, p, r, flags).  Its box is
//   c = x + rotate(q, p)      r = r            (body = -1: c = p)
// with x and q the body's rows as for a sensor (k_batch_sensor.h: x WITHOUT delta), every operation a separate f32 one.  Its record, for
// a call's k, is 1 + k words: the number of bodies of its world whose tight box BoundedBy<AABB> overlaps it (Overlaps<AABB>) - the
// list mgf_batch_overlap_aabb_many reports, `body` left out if MGF_SENSOR_IGNORE_SELF is set - then the first min(count, k) of them in
// ascending index, then -1.  A fixed width needs no total: count and fill are one pass, and nothing waits for the host.
//   k_batch_zone_first<SRC>  a workgroup per work item = (world, up to 256 zones), through bo_front (k_batch_observe.h) - the front of
//                            k_batch_observe_overlap: the world's tight boxes in LDS once, a zone's lanes in one wave, a hit's rank
//                            from the wave's ballot.  What this kernel brings: a zone's box and the body it does not hold, and a hit
//                            of rank < k stores its index at word 1 + rank: the first k in ascending order with no sort and no
//                            atomic.  Behind the front the group's first lane stores the count and, where asked, the box; the
//                            group's lanes store -1 into the words the list left.
//                            SRC = kItemTable: the rig's table, built on the host when the rig is set (BatchQueryPlan); the box is
//                            formed from the record and the body's x and q.  SRC = kItemFixed: every world has `per` boxes, the
//                            caller's, the work item follows from blockIdx.x (bq_item), the order is the identity.
// A loader holds no barrier and does not leave the kernel, nor does the store behind a hit; there is no return at all.  The ignored
// body is dropped before the ballot (bo_front<.., true>).
// No workgroup waits for another.
#pragma once
#include "k_batch_observe.h"

namespace mgf {

struct ZoneIn { int32_t world, body; float p[3], r[3]; int32_t flags, reserved; };  // mgf_batch_zone
static_assert(sizeof(ZoneIn) == 40, "the rig goes up as the caller's records");

struct BatchZoneArgs : BatchWorkArgs {
  const float4* x;        // kItemTable: the bodies' rows (Bodies::x, ::q), world k's at [w_off[k], w_off[k + 1])
  const float4* q;
  const ZoneIn* rig;      // kItemTable, by the caller's index; world and body checked on the host: body = -1, or < the world's length
  const float* boxes;     // kItemFixed, by the caller's index: c.xyz, r.xyz
  const int32_t* ignore;  // kItemFixed, by the caller's index: only ever compared with a body index; null: none for all
  uint32_t k;             // the body indices a record holds (<= MGF_BATCH_MAX_BODIES)
  int32_t* out;           // by the caller's index: 1 + k words a zone
  float* boxes_out;       // by the caller's index: c.xyz, r.xyz as formed; null: not stored
};

// The two loaders of a zone's box - the caller's (kItemFixed), and the one formed from the rig's record and the body's x and q
// (kItemTable) - and the box as stored where asked for: written once, for this kernel and for every kernel built on a zone's box in
// the headers that include this one
__device__ __forceinline__ BatchBox bz_fixed(const BatchZoneArgs& A, uint32_t qi) {
  return BatchBox{{ld3(A.boxes + 6 * (size_t)qi), ld3(A.boxes + 6 * (size_t)qi + 3)}, A.ignore ? A.ignore[qi] : -1};
}
__device__ __forceinline__ BatchBox bz_mounted(const BatchZoneArgs& A, uint32_t qi, uint32_t g0) {
  const ZoneIn s = A.rig[qi];
  BatchBox b;
  b.Q.c = ld3(s.p); b.Q.r = ld3(s.r);
  if (s.body >= 0) {
    const size_t g = (size_t)g0 + (uint32_t)s.body;
    const float4 bx = A.x[g], bq = A.q[g];
    b.Q.c = xyz(bx) + rotate(mkq(bq.x, mk3(bq.y, bq.z, bq.w)), ld3(s.p));
  }
  b.ign = (s.flags & MGF_SENSOR_IGNORE_SELF) ? s.body : -1;
  return b;
}
__device__ __forceinline__ void bz_box_out(float* boxes_out, uint32_t qi, const Box& Q) {
  float* bo = boxes_out + 6 * (size_t)qi;
  bo[0] = Q.c.x; bo[1] = Q.c.y; bo[2] = Q.c.z; bo[3] = Q.r.x; bo[4] = Q.r.y; bo[5] = Q.r.z;
}

// k_batch_zone_first<SRC> and its part-aware form (k_batch_part_query.h), written once over the bodies' policy
template <int SRC, class Bodies>
__device__ __forceinline__ void bz_first(const BatchZoneArgs& A, const Bodies& bodies, const BatchItemSrc& S, float4* s_dyn) {
  BatchWork W(A, true, bq_item<SRC>(A, S));
  const uint32_t k = A.k;
  BatchBox z;
  const auto fixed = [&](uint32_t qi, uint32_t) { return bz_fixed(A, qi); };
  const auto mounted = [&](uint32_t qi, uint32_t g0) { return bz_mounted(A, qi, g0); };
  const auto record = [&]() { return A.out + (size_t)(1u + k) * W.qi; };  // (of a live lane, W split)
  const auto store = [&](bool hit, uint32_t i, uint32_t rank) {
    if (hit && rank < k) record()[1u + rank] = (int32_t)i;
  };
  const uint32_t m = SRC == kItemFixed ? bo_front<true, true>(A, bodies, W, s_dyn, z, fixed, store) : bo_front<false, true>(A, bodies, W, s_dyn, z, mounted, store);
  if (W.live) {
    const uint32_t sub = W.sub;
    int32_t* o = record();
    if (sub == 0u) o[0] = (int32_t)m;
    for (uint32_t s = min(m, k) + sub; s < k; s += W.L) o[1u + s] = -1;
    if (sub == 0u && A.boxes_out) bz_box_out(A.boxes_out, W.qi, z.Q);
  }
}

// LDS (dynamic): 32 bytes a body.
template <int SRC>
__global__ __launch_bounds__(kBatchBlock) void k_batch_zone_first(BatchZoneArgs A, BatchItemSrc S) {
  extern __shared__ float4 s_dyn[];
  bz_first<SRC>(A, PlainBodies(A), S, s_dyn);
}

}  // namespace mgf
