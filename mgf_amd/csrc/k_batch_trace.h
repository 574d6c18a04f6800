// The touch trace of a rollout (mgf_batch_rollout_touches, mgf_batch_rollout_touches_dev; host_batch_trace.inc): row t of the contact
// sensors' reports written behind tick t, inside the step's launch train.  (Part of the kernel set described in kernels.h.)
//
// The call is defined by the loop  actuate_dev(u[t]) | step(1) | gather_state_dev(row t) | read_touches_dev(touch + t * n_touch)  and
// this launch rides in the train behind k_batch_rollout_record (k_batch_rollout.h), so that act[k] is final when it is read here.
//   k_batch_trace_touch<FORMAT>   k_batch_touch's fold (k_batch_touch.h) of world k's list as tick t left it: a workgroup per work item =
//                                 (world, up to 256 sensors), a lane per sensor, TouchIn / TouchWord / TouchFold / touch_lower from
//                                 there and the kernel body restated line for line (-ffp-contract=off: the same bits; k_batch_touch.h
//                                 stays as it is).  A work item belongs to ONE world, so the train's gate is the workgroup's:
//                                   on = done[k] == t + 1 && act[k] <= t + 1     world k completed tick t in THIS pass - the condition
//                                                                                of k_batch_rollout_record, for the same reasons:
//                                   done[k] <= t             undone at or before tick t: skipped, written in the pass that completes t;
//                                   done[k] == t + 1, act[k] == t + 2    the world sits undone at tick t + 1 from an earlier pass: row t
//                                                            was written in the pass that completed t and is not written again.  (As
//                                                            the tick's kernels stand, a tick that does not fit is turned down before
//                                                            it writes a record or the count, so the row would come out the same; the
//                                                            trace does not lean on that.)
//                                   done[k] == n_ticks == act[k]         finished in an earlier pass: matches t == n_ticks - 1 alone and
//                                                            stores the bytes it stored then (list, q and rig are unchanged).
//                                 The gate is folded into the item's count and into C: a workgroup that is off has no live lane and
//                                 makes zero trips of the tile loop.  The kernel keeps the parent's shape - every lane makes every
//                                 trip (C, the tile and the item's fourth word are the workgroup's), the only barriers are the tile
//                                 loop's, no lane leaves ahead of another, nothing is added to a counter, and the only global stores
//                                 are the report's words: four TouchWords for MGF_ROLLOUT_TOUCH_FULL (mgf_touch_report), one for
//                                 MGF_ROLLOUT_TOUCH_SHORT (n_contacts, partner, normal_impulse, strongest_impulse of that report).
// The list's address and offsets (cons, c_off) are the PASS's: a capacity re-run moves the lists (batch_allot), so the host fills V in
// again for every pass (batch_step_run, host_batch.inc).
#pragma once
#include "k_batch_touch.h"

namespace mgf {

constexpr int kTraceTouchFull = 0, kTraceTouchShort = 1;  // MGF_ROLLOUT_TOUCH_FULL / _SHORT

struct BatchTraceTouchArgs {
  BatchTouchArgs V;      // k_batch_touch's view of the rig and the lists, rebuilt per pass; V.out: row 0 of the trace
  const uint32_t* done;  // ticks of this call world k has completed (BatchArgs::done)
  const uint32_t* act;   // ticks whose actuation world k has behind it (BatchRolloutArgs::act), final behind k_batch_rollout_record
  uint32_t tick, n_touch;
};

// LDS (dynamic): A.V.tile words.
template <int FORMAT>
__global__ __launch_bounds__(kBatchBlock) void k_batch_trace_touch(BatchTraceTouchArgs T) {
  extern __shared__ float4 s_dyn[];
  uint32_t* s_b = reinterpret_cast<uint32_t*>(s_dyn);
  const BatchTouchArgs& A = T.V;
  const uint4 it = A.items[blockIdx.x];
  const uint32_t tid = threadIdx.x, k = it.x, g0 = A.w_off[k], tile = A.tile, t = T.tick;
  const bool on = T.done[k] == t + 1u && T.act[k] <= t + 1u;  // the tick gate, the workgroup's
  const uint32_t C = on ? A.c_count[k] : 0u, count = on ? it.z : 0u;
  const CRec* cons = A.cons + A.c_off[k];
  const bool live = tid < count;
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
    for (uint32_t c0 = 0; c0 < C; c0 += tile) {  // (C and tile are the workgroup's: every lane makes every trip - none where the gate is off)
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
    const size_t at = (size_t)t * T.n_touch + qi;  // row t, the caller's index
    if (FORMAT == kTraceTouchShort) {
      A.out[at] = TouchWord{F.n, (uint32_t)F.best_partner, f2u(F.sum), f2u(F.best_ni)};
    } else {
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
      TouchWord* o = A.out + 4 * at;
      o[0] = TouchWord{F.n, (uint32_t)F.best_partner, (uint32_t)record, 0u};
      o[1] = TouchWord{f2u(imp.x), f2u(imp.y), f2u(imp.z), f2u(F.sum)};
      o[2] = TouchWord{f2u(push.x), f2u(push.y), f2u(push.z), f2u(F.best_ni)};
      o[3] = TouchWord{f2u(arm.x), f2u(arm.y), f2u(arm.z), 0u};
    }
  }
}

}  // namespace mgf
