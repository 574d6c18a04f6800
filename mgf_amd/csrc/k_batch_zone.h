// Box zones of a batch: the count and the first k bodies of every box, a fixed-width record (mgf_batch_set_zones, mgf_batch_read_zones,
// mgf_batch_read_zones_dev, mgf_batch_overlap_first_dev; host_batch_zone.inc).  (Part of the kernel set described in kernels.h.)
//
// A zone is an axis-aligned box whose centre is fixed in the frame of a body, or in the world: (world, body, p, r, flags).  Its box is
//   c = x + rotate(q, p)      r = r            (body = -1: c = p)
// with x and q the body's rows as for a sensor (k_batch_sensor.h: x WITHOUT delta), every operation a separate f32 one.  Its record, for
// a call's k, is 1 + k words: the number of bodies of its world whose tight box BoundedBy<AABB> overlaps it (Overlaps<AABB>) - the
// list mgf_batch_overlap_aabb_many reports, `body` left out if MGF_SENSOR_IGNORE_SELF is set - then the first min(count, k) of them in
// ascending index, then -1.  A fixed width needs no total: count and fill are one pass, and nothing waits for the host.
//   k_batch_zone_first<SRC>  a workgroup per work item = (world, up to 256 zones), through bz_front - k_batch_observe_overlap's split,
//                            written for a record instead of a list: the tight boxes of the world's colliders col0 / col1 staged in LDS
//                            once; a zone gets min(64, 256 / (count rounded up to a power of two)) lanes of one wave, which take the
//                            bodies in chunks of that many, ascending; a hit's rank is the hits of the chunks before plus the hits
//                            below its lane in the wave's ballot, and a hit of rank < k stores its index at word 1 + rank: the first
//                            k in ascending order with no sort and no atomic.  Behind the loop the group's first lane stores the
//                            count and, where asked, the box; the group's lanes store -1 into the words the list left.
//                            SRC = kItemTable: the rig's table, built on the host when the rig is set (BatchQueryPlan); the box is
//                            formed from the record and the body's x and q.  SRC = kItemFixed: every world has `per` boxes, the
//                            caller's, the work item follows from blockIdx.x (bq_item), the order is the identity.
// What a loader brings is where a box comes from - load(qi, g0) -> BatchZone, run by the live lanes behind the staging.  It holds no
// barrier and does not leave the kernel.  Every lane of a wave makes every trip of the loop (n and L are the work item's); there is no
// return at all.  The ignored body is dropped before the ballot; a NaN box hits nothing because box_overlaps is false for it.
// No workgroup waits for another.
#pragma once
#include "k_batch_query.h"

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

// a live zone's box in world coordinates and the body of its world it does not hold (-1: none): what a loader hands bz_front
struct BatchZone { Box Q; int32_t ign; };

template <int SRC, class Load>
__device__ __forceinline__ void bz_front(const BatchZoneArgs& A, const BatchItemSrc& S, float4* s_dyn, Load&& load) {
  BatchWork W(A, true, bq_item<SRC>(A, S));
  const uint32_t tid = threadIdx.x, g0 = W.g0, n = W.n, k = A.k;
  float4 *s_c = s_dyn, *s_r = s_dyn + n;
  for (uint32_t i = tid; i < n; i += kBatchBlock) {
    const Box tb = comp_bounds(to_comp(A.col0[(size_t)g0 + i], A.col1[(size_t)g0 + i]));
    s_c[i] = mk4(tb.c, 0.0f); s_r[i] = mk4(tb.r, 0.0f);
  }
  __syncthreads();
  W.template split<SRC == kItemFixed>(A, min(W.shift(), 6u));  // (a zone's lanes in one wave: the ballot)
  const uint32_t L = W.L, sub = W.sub, qi = W.qi;
  const bool live = W.live;
  Box Q; Q.c = mk3(0.0f, 0.0f, 0.0f); Q.r = Q.c;
  int32_t ign = -1;
  if (live) { const BatchZone z = load(qi, g0); Q = z.Q; ign = z.ign; }
  int32_t* o = A.out + (size_t)(1u + k) * qi;                     // (written by live lanes only)
  const uint32_t shift = (tid & 63u) - sub;                        // the first lane of the zone's group within the wave
  const uint64_t group = L == 64u ? ~0ull : ((1ull << L) - 1ull);  // the group's lanes, from that lane
  uint32_t m = 0;
  for (uint32_t i0 = 0; i0 < n; i0 += L) {  // (n and L are the work item's: every lane of the wave makes every trip)
    const uint32_t i = i0 + sub;
    bool hit = false;
    if (live && i < n && (int32_t)i != ign) {
      Box b; b.c = xyz(s_c[i]); b.r = xyz(s_r[i]);
      hit = box_overlaps(b, Q);
    }
    const uint64_t g = ((uint64_t)__ballot(hit) >> shift) & group;
    const uint32_t rank = m + (uint32_t)__popcll(g & ((1ull << sub) - 1ull));
    if (hit && rank < k) o[1u + rank] = (int32_t)i;
    m += (uint32_t)__popcll(g);
  }
  if (live) {
    if (sub == 0u) o[0] = (int32_t)m;
    for (uint32_t s = min(m, k) + sub; s < k; s += L) o[1u + s] = -1;
    if (sub == 0u && A.boxes_out) {
      float* bo = A.boxes_out + 6 * (size_t)qi;
      bo[0] = Q.c.x; bo[1] = Q.c.y; bo[2] = Q.c.z; bo[3] = Q.r.x; bo[4] = Q.r.y; bo[5] = Q.r.z;
    }
  }
}

// LDS (dynamic): 32 bytes a body.
template <int SRC>
__global__ __launch_bounds__(kBatchBlock) void k_batch_zone_first(BatchZoneArgs A, BatchItemSrc S) {
  extern __shared__ float4 s_dyn[];
  if (SRC == kItemFixed)
    bz_front<SRC>(A, S, s_dyn, [&](uint32_t qi, uint32_t) {
      BatchZone z;
      z.Q.c = ld3(A.boxes + 6 * (size_t)qi); z.Q.r = ld3(A.boxes + 6 * (size_t)qi + 3);
      z.ign = A.ignore ? A.ignore[qi] : -1;
      return z;
    });
  else
    bz_front<SRC>(A, S, s_dyn, [&](uint32_t qi, uint32_t g0) {
      const ZoneIn s = A.rig[qi];
      BatchZone z;
      z.Q.c = ld3(s.p); z.Q.r = ld3(s.r);
      if (s.body >= 0) {
        const size_t g = (size_t)g0 + (uint32_t)s.body;
        const float4 bx = A.x[g], bq = A.q[g];
        z.Q.c = xyz(bx) + rotate(mkq(bq.x, mk3(bq.y, bq.z, bq.w)), ld3(s.p));
      }
      z.ign = (s.flags & MGF_SENSOR_IGNORE_SELF) ? s.body : -1;
      return z;
    });
}

}  // namespace mgf
