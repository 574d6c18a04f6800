// Box zones of a batch, nearest first: the count and the k nearest bodies of every box, a fixed-width record (mgf_batch_read_zones_nearest,
// mgf_batch_read_zones_nearest_dev, mgf_batch_overlap_nearest_dev; host_batch_nearest.inc).  (Part of the kernel set described in kernels.h.)
//
// The zone, its box Q = (c, r) and its list are k_batch_zone.h's.  For body i of the list, m_i the centre of its tight box (the box the
// overlap test itself uses) and e = m_i - c,
//   d2_i = (e.x * e.x + e.y * e.y) + e.z * e.z        dot(e, e) of dev_math.h, every operation a separate f32 one
// which is never NaN for a listed body (a NaN difference fails Overlaps<AABB>) and lies in [+0, +inf]: its bits order as the floats do.
// The record, for a call's k (<= MGF_BATCH_ZONE_NEAREST_MAX_K), is 1 + k words: the full count, the first min(count, k) bodies of the list
// in ascending (d2, body index), then -1; where asked for, k f32 words beside it: their d2, then +inf.
//   k_batch_nearest<SRC>     a workgroup per work item = (world, up to 256 zones).  The count is bo_front's (k_batch_observe.h) with a hook
//                            that stores nothing: the world's tight boxes in LDS once, a zone's L lanes in one wave.  Behind it
//                            ceil(k / 4) passes of selection over the same LDS.  In a pass a lane strides over the world's bodies and
//                            keeps, ascending in four registers (NearestPick), the four least 64-bit keys (bits(d2) << 32) | index among
//                            the bodies that overlap, are not the ignored body and whose key is above the last one chosen; the zone's
//                            lanes merge their four with __shfl_xor over the offsets below L (the group is aligned in its wave: the
//                            exchange stays inside it; the four least of two ascending fours are min(a[i], b[3 - i]), then a sorting
//                            network); its first lane stores the indices and d2, or -1 and +inf once nothing is left.  A key names
//                            its body, so keys are distinct and "above the last" walks the list in order: no sort of the list, no
//                            atomic, no memory beyond the staged boxes - nothing grows with zones x k.  A trip has no branch: the
//                            body read is clamped to the world's last, the three tests of Overlaps<AABB> are box_overlaps' own
//                            operations on the difference e that d2 is made of, without its early exits, and everything a body must
//                            pass selects between its key and "none".
//                            SRC = kItemTable / kItemFixed and the two box loaders: as k_batch_zone_first's.
// k is a kernel argument and n and L are the work item's: every lane of a wave makes every trip of every loop; no loop leaves early on a
// lane's own condition, there is no barrier behind the front's and no return at all.  Cost: (1 + ceil(k / 4)) n / L trips a lane.
// No workgroup waits for another.
#pragma once
#include "k_batch_zone.h"

namespace mgf {

struct BatchNearestArgs : BatchZoneArgs {  // k: the bodies a record holds (<= MGF_BATCH_ZONE_NEAREST_MAX_K)
  float* dist2_out;                        // by the caller's index: k words a zone; null: not stored
};

constexpr uint64_t kNearestNone = ~0ull;   // above every key: a key's high word is at most the bits of +inf

// The four least keys a lane, or a zone's lanes, have seen in a pass, ascending; kNearestNone where there is none.  Registers only:
// every index is a name.
struct NearestPick {
  uint64_t t0, t1, t2, t3;
  static __device__ __forceinline__ void order(uint64_t& a, uint64_t& b) {
    const uint64_t lo = a < b ? a : b, hi = a < b ? b : a;
    a = lo; b = hi;
  }
  __device__ __forceinline__ void clear() { t0 = t1 = t2 = t3 = kNearestNone; }
  // x takes the place of the largest if it is below it, and sinks to its own
  __device__ __forceinline__ void put(uint64_t x) {
    t3 = x < t3 ? x : t3;
    order(t2, t3); order(t1, t2); order(t0, t1);
  }
  // the four least of this and o: of two ascending fours they are min(a[i], b[3 - i]), in no order; five exchanges sort four
  __device__ __forceinline__ void merge(const NearestPick& o) {
    t0 = t0 < o.t3 ? t0 : o.t3; t1 = t1 < o.t2 ? t1 : o.t2; t2 = t2 < o.t1 ? t2 : o.t1; t3 = t3 < o.t0 ? t3 : o.t0;
    order(t0, t1); order(t2, t3); order(t0, t2); order(t1, t3); order(t1, t2);
  }
  __device__ __forceinline__ NearestPick shfl(int off) const {
    NearestPick o;
    o.t0 = __shfl_xor((unsigned long long)t0, off); o.t1 = __shfl_xor((unsigned long long)t1, off);
    o.t2 = __shfl_xor((unsigned long long)t2, off); o.t3 = __shfl_xor((unsigned long long)t3, off);
    return o;
  }
};

// k_batch_nearest<SRC> and its part-aware form (k_batch_part_query.h), written once over the bodies' policy: the distances are measured
// from the centre of the box the policy staged
template <int SRC, class Bodies>
__device__ __forceinline__ void bn_nearest(const BatchNearestArgs& A, const Bodies& bodies, const BatchItemSrc& S, float4* s_dyn) {
  BatchWork W(A, true, bq_item<SRC>(A, S));
  const uint32_t k = A.k;
  BatchBox z;
  const auto fixed = [&](uint32_t qi, uint32_t) { return bz_fixed(A, qi); };
  const auto mounted = [&](uint32_t qi, uint32_t g0) { return bz_mounted(A, qi, g0); };
  const auto count_only = [](bool, uint32_t, uint32_t) {};
  const uint32_t m = SRC == kItemFixed ? bo_front<true, true>(A, bodies, W, s_dyn, z, fixed, count_only) : bo_front<false, true>(A, bodies, W, s_dyn, z, mounted, count_only);
  const uint32_t n = W.n, L = W.L, sub = W.sub;
  const bool live = W.live, first = live && sub == 0u;
  const float4 *s_c = s_dyn, *s_r = s_dyn + n;  // (as the front staged them)
  const Box Q = z.Q;
  const int32_t ign = z.ign;
  int32_t* o = A.out + (size_t)(1u + k) * W.qi;  // (of a live lane)
  float* od = A.dist2_out ? A.dist2_out + (size_t)k * W.qi : nullptr;
  const auto put = [&](uint32_t slot, uint64_t key) {  // (of the zone's first lane) slot < k: the record's word 1 + slot, its distance
    const bool none = key == kNearestNone;
    o[1u + slot] = none ? -1 : (int32_t)(uint32_t)key;
    if (od) od[slot] = none ? u2f(0x7F800000u) : u2f((uint32_t)(key >> 32));
  };
  uint64_t lo = 0ull;  // the least key a pass may choose: one above the last chosen
  for (uint32_t r0 = 0; r0 < k; r0 += 4u) {
    NearestPick best;
    best.clear();
#pragma unroll 2
    for (uint32_t i0 = 0; i0 < n; i0 += L) {  // (n and L are the work item's: every lane of the wave makes every trip)
      const uint32_t i = i0 + sub, at = min(i, n - 1u);
      const V3 bc = xyz(s_c[at]), br = xyz(s_r[at]);
      const V3 e = bc - Q.c;
      // box_overlaps(body, Q): its three tests, no early exit
      const float ax = fabs_rs(e.x), ay = fabs_rs(e.y), az = fabs_rs(e.z);
      const bool hit = (ax <= (br.x + Q.r.x)) & (ay <= (br.y + Q.r.y)) & (az <= (br.z + Q.r.z));
      const uint64_t key = ((uint64_t)f2u(dot(e, e)) << 32) | i;
      const bool ok = live & (i < n) & ((int32_t)i != ign) & hit & (key >= lo);
      best.put(ok ? key : kNearestNone);
    }
    for (uint32_t off = L >> 1; off > 0u; off >>= 1) best.merge(best.shfl((int)off));
    if (first) {
      put(r0, best.t0);
      if (r0 + 1u < k) put(r0 + 1u, best.t1);
      if (r0 + 2u < k) put(r0 + 2u, best.t2);
      if (r0 + 3u < k) put(r0 + 3u, best.t3);
    }
    lo = best.t3 == kNearestNone ? kNearestNone : best.t3 + 1ull;
  }
  if (first) {
    o[0] = (int32_t)m;
    if (A.boxes_out) bz_box_out(A.boxes_out, W.qi, Q);
  }
}

// LDS (dynamic): 32 bytes a body.
template <int SRC>
__global__ __launch_bounds__(kBatchBlock) void k_batch_nearest(BatchNearestArgs A, BatchItemSrc S) {
  extern __shared__ float4 s_dyn[];
  bn_nearest<SRC>(A, PlainBodies(A), S, s_dyn);
}

}  // namespace mgf
