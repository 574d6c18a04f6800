// Contact sensors of a batch: the last tick's constraint list folded per (body, partner), a record of fixed width (mgf_batch_set_touches,
// mgf_batch_read_touches, mgf_batch_read_touches_dev; host_batch_touch.inc).  (Part of the kernel set described in kernels.h.)
//
// A sensor is (world, body = x, other, flags).  Over the chain of x - the records of the world's list with a == x ascending, then those
// with b == x ascending: the order of k_batch_observe_contacts and of ContactConstraint::solve - the records whose partner passes the
// filter `other` are folded as mgf_body_contacts folds every record (impulse -/+ normal * ni, the sum of ni, the count; sequential f32,
// nothing fused), and the strongest of them - the first, replaced only by a later one with ni > its ni - gives partner, record, push
// and arm.  MGF_TOUCH_BODY_FRAME turns the three vectors by the conjugate of the body's q as it is on the device at the read.
//   k_batch_touch  a workgroup per work item = (world, up to 256 sensors) of the rig's sort by world (BatchQueryPlan), a LANE per sensor.
//                  Nothing is built in global memory - `rows` is not touched, so two work items of one world (a world with more than 256
//                  sensors) share nothing they write.  What is used of the list is what k_batch_observe_contacts uses: it is ascending in
//                  `a`, so the records with a == v are one range, found by a binary search of ceil(log2(C + 1)) steps.
//                    x is `a`:  the range of x, every record's partner b held against the filter.
//                    x is `b`:  other >= 0: the range of `other`, the records with b == x (nothing is assumed of b against a);
//                               MGF_TOUCH_STATIC: none - a record's `a` is a body;
//                               MGF_TOUCH_ANY / _ANY_BODY: the whole list.  The workgroup stages the list's `b` column in dynamic LDS a
//                               tile at a time (16 bytes a body of the batch's largest world, at least 256 words: a world's first share
//                               of the storage is four records a body, so a list that has not outgrown it is one tile), and every
//                               lane that needs it walks the tile four words a read, all lanes at one address - a broadcast - and
//                               folds the records it finds, ascending.  A work item none of whose sensors needs the column skips it
//                               (its fourth word, set on the host with the rig).
//                  The cost: a sensor reads 128 bytes a matching record and nothing of the others but, for the two filters that need the
//                  `b` occurrences, 4 bytes a record of the world's list from LDS; the workgroup reads the column once.
// A lane folds its matches one behind the other in registers: nothing of an answer depends on lane scheduling, on the other sensors
// of the work item or on the tile; there is no atomic, and no workgroup waits for another.  The only barriers are the tile loop's, and
// every lane of the workgroup makes every trip of it (C, the tile and the item's fourth word are the workgroup's).  There is no exit.
#pragma once
#include "k_batch_observe.h"

namespace mgf {

struct TouchIn { int32_t world, body, other, flags; };  // mgf_batch_touch
static_assert(sizeof(TouchIn) == 16, "the rig goes up as the caller's records");

// a report's four words of 16 bytes, at an address that is a multiple of 4
struct __attribute__((packed, aligned(4))) TouchWord { uint32_t x, y, z, w; };

struct BatchTouchArgs {
  const uint4* items;       // work item: (world, first, count <= 256, scan): the sensors at sorted positions [first, first + count); scan: one needs the `b` column
  const uint32_t* order;    // sorted position -> the caller's index
  const TouchIn* rig;       // by the caller's index; world, body and other checked on the host against the world's length
  const CRec* cons;         // world k's list at c_off[k], c_count[k] records
  const uint32_t* c_off;
  const uint32_t* c_count;
  const uint32_t* w_off;
  const float4* q;          // the bodies' rows (Bodies::q), world k's at [w_off[k], w_off[k + 1])
  uint32_t tile;            // words of dynamic LDS: a multiple of 4
  TouchWord* out;           // by the caller's index: four words a sensor (mgf_touch_report)
};

// the first record of the list with a >= v (the list is ascending in a)
__device__ __forceinline__ uint32_t touch_lower(const CRec* cons, uint32_t C, uint32_t v) {
  uint32_t lo = 0u, hi = C;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    const bool below = cons[mid].a < v;
    lo = below ? mid + 1u : lo;
    hi = below ? hi : mid;
  }
  return lo;
}

// What a lane holds of its sensor's fold; is_a: the body is `a` of the record taken, else `b`.
struct TouchFold {
  V3 imp;
  float sum, best_ni;
  uint32_t n, best_c;
  int32_t best_partner;
  bool best_a;
  __device__ __forceinline__ void take(const CRec* cons, uint32_t c, bool is_a, int32_t partner) {
    const CRec* r = &cons[c];
    const float ni = r->nimp;
    const V3 t = ld3(r->n) * ni;
    imp = is_a ? imp - t : imp + t;  // va -= impulse * inv_mass_a, solver.rs:243-247
    sum = sum + ni;
    if (n == 0u || ni > best_ni) { best_ni = ni; best_c = c; best_partner = partner; best_a = is_a; }  // (ties and NaN keep the earlier one)
    ++n;
  }
};

// LDS (dynamic): A.tile words.
__global__ __launch_bounds__(kBatchBlock) void k_batch_touch(BatchTouchArgs A) {
  extern __shared__ float4 s_dyn[];
  uint32_t* s_b = reinterpret_cast<uint32_t*>(s_dyn);
  const uint4 it = A.items[blockIdx.x];
  const uint32_t tid = threadIdx.x, k = it.x, g0 = A.w_off[k], C = A.c_count[k], tile = A.tile;
  const CRec* cons = A.cons + A.c_off[k];
  const bool live = tid < it.z;
  const uint32_t qi = live ? A.order[it.y + tid] : 0u;
  TouchIn s;
  s.world = 0; s.body = 0; s.other = MGF_TOUCH_STATIC; s.flags = 0;
  if (live) s = A.rig[qi];
  const uint32_t x = (uint32_t)s.body;
  const int32_t other = s.other;
  TouchFold F;
  F.imp = mk3(0.0f, 0.0f, 0.0f); F.sum = 0.0f; F.best_ni = 0.0f; F.n = 0u; F.best_c = 0u; F.best_partner = MGF_TOUCH_NONE; F.best_a = true;
  if (live) {
    for (uint32_t c = touch_lower(cons, C, x); c < C && cons[c].a == x; ++c) {  // x is `a`
      const uint32_t b = cons[c].b;
      const int32_t partner = b == kNone ? -1 : (int32_t)b;
      const bool match = other >= 0 ? partner == other : other == MGF_TOUCH_STATIC ? partner < 0 : other == MGF_TOUCH_ANY_BODY ? partner >= 0 : true;
      if (match) F.take(cons, c, true, partner);
    }
    if (other >= 0)
      for (uint32_t c = touch_lower(cons, C, (uint32_t)other); c < C && cons[c].a == (uint32_t)other; ++c)  // x is `b` of a record of `other`
        if (cons[c].b == x) F.take(cons, c, false, other);
  }
  const bool scan = live && (other == MGF_TOUCH_ANY || other == MGF_TOUCH_ANY_BODY);  // x is `b` of anybody's record
  if (it.w) {  // (the work item's, set on the host: every lane of the workgroup takes the same side)
    for (uint32_t c0 = 0; c0 < C; c0 += tile) {  // (C and tile are the workgroup's: every lane makes every trip)
      for (uint32_t i = tid; i < tile; i += kBatchBlock) s_b[i] = c0 + i < C ? cons[c0 + i].b : kNone;  // (no body is kNone)
      __syncthreads();
      if (scan) {
        const uint32_t m = min(tile, C - c0);
        for (uint32_t i = 0; i < m; i += 4u) {
          const float4 w = s_dyn[i >> 2];
          if (f2u(w.x) == x) F.take(cons, c0 + i, false, (int32_t)cons[c0 + i].a);
          if (f2u(w.y) == x) F.take(cons, c0 + i + 1u, false, (int32_t)cons[c0 + i + 1u].a);
          if (f2u(w.z) == x) F.take(cons, c0 + i + 2u, false, (int32_t)cons[c0 + i + 2u].a);
          if (f2u(w.w) == x) F.take(cons, c0 + i + 3u, false, (int32_t)cons[c0 + i + 3u].a);
        }
      }
      __syncthreads();
    }
  }
  if (live) {
    V3 imp = F.imp, push = mk3(0.0f, 0.0f, 0.0f), arm = push;
    int32_t record = -1;
    if (F.n) {
      const CRec* r = &cons[F.best_c];
      const V3 nn = ld3(r->n);
      push = F.best_a ? mk3(u2f(f2u(nn.x) ^ 0x80000000u), u2f(f2u(nn.y) ^ 0x80000000u), u2f(f2u(nn.z) ^ 0x80000000u)) : nn;
      arm = F.best_a ? ld3(r->ra) : ld3(r->rb);
      record = (int32_t)F.best_c;
      if (s.flags & MGF_TOUCH_BODY_FRAME) {
        const float4 bq = A.q[(size_t)g0 + x];
        const Quat inv = mkq(bq.x, mk3(-bq.y, -bq.z, -bq.w));
        imp = rotate(inv, imp); push = rotate(inv, push); arm = rotate(inv, arm);
      }
    }
    TouchWord* o = A.out + 4 * (size_t)qi;
    o[0] = TouchWord{F.n, (uint32_t)F.best_partner, (uint32_t)record, 0u};
    o[1] = TouchWord{f2u(imp.x), f2u(imp.y), f2u(imp.z), f2u(F.sum)};
    o[2] = TouchWord{f2u(push.x), f2u(push.y), f2u(push.z), f2u(F.best_ni)};
    o[3] = TouchWord{f2u(arm.x), f2u(arm.y), f2u(arm.z), 0u};
  }
}

}  // namespace mgf
