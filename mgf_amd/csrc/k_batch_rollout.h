// Rollouts of a batch (mgf_batch_rollout, mgf_batch_rollout_dev; host_batch_rollout.inc): n_ticks ticks, a row of controls applied ahead
// of every tick and a row of state written behind it, inside the step's one host wait.
// (Part of the kernel set described in kernels.h.)
//
// The call is defined by the loop  actuate_dev(u[t]) | step(1) | gather_state_dev(row t)  and these two launches ride in the step's
// launch train, one ahead of a tick's kernels and one behind them.  The train is world-wise: a world whose tick did not fit its share
// of the storage is undone and sits at done[k]; every later launch of the pass skips it (A.done[k] != A.tick), and the host runs the
// train again from the smallest done[k].  Both kernels obey that gate, and a second word a world beside it:
//   act[k]   ticks whose actuation world k has behind it.  k_batch_front takes the undo snapshot at the start of the tick, BEHIND the
//            actuation: a world whose tick t is undone comes back with tick t's impulse in its velocities, and the force and torque rows
//            are not in the snapshot at all.  In the pass that runs tick t again done[k] == t as before, and a gate on done[k] alone would
//            apply u[t] a second time.  So: applied iff done[k] == t && act[k] == t, and act[k] moves to t + 1 in the launch BEHIND the
//            tick - k_batch_rollout_record, a lane per world - whether the tick held or not.  No lane of k_batch_rollout_act writes a
//            word another lane of that launch reads.
//   k_batch_rollout_act<MODE>   k_batch_actuate<MODE, false>'s work (k_batch_actuator.h) on row t of u: a lane per run of the rig's plan,
//                               the walk restated line for line (-ffp-contract=off: the same bits; k_batch_actuator.h stays as it is).
//                               A wave holds runs of several worlds, so the gate differs from lane to lane: it is folded into the run
//                               length - a lane whose world is not at (t, t) has cnt = 0 - and the loop keeps its shape: every lane of a
//                               wave makes the same number of trips (__any), no lane leaves ahead of another and no condition that
//                               is the same for the whole wave is evaluated inside it (tools/check_lane_masks.py).
//   k_batch_rollout_record      behind tick t's k_batch_solve.  Lane i < m: k_batch_dev_gather's rows (x + delta, q, v, omega) of body
//                               body[i] (null: body i) into row t of the outputs, iff the body's world - found in the offsets table by
//                               a binary search - has done[k] == t + 1 and act[k] <= t + 1: it completed tick t in THIS pass.  A world
//                               that was undone at tick t is written in the pass in which it completes t; a world that sits undone at
//                               tick t + 1 has act[k] == t + 2 and tick t + 1's impulse in its velocities, and is not written again;
//                               a world that finished the call in an earlier pass matches only t == n_ticks - 1, and stores the bytes
//                               it stored then.  An index outside the batch is counted once a tick (`count`: the first pass).
//                               Lane k < n_worlds: act[k] == t && done[k] >= t -> act[k] = t + 1.  act[k] is read by the lanes of the
//                               bodies while that lane writes it; both values, t and t + 1, admit the body, t + 2 never appears in
//                               this launch: what is written does not depend on which one a lane sees.
#pragma once
#include "k_batch_actuator.h"

namespace mgf {

struct BatchRolloutArgs {
  Bodies B;                       // every world's bodies
  const uint32_t* w_off;          // the worlds' first bodies (n_worlds + 1)
  const uint32_t* done;           // ticks of this call world k has completed (BatchArgs::done)
  uint32_t* act;                  // ticks whose actuation world k has behind it
  // the actuation: BatchActuateArgs' view of the rig
  const uint4* runs;              // run r: (world, body, first sorted position, count >= 1)
  const float4* rig;              // by the caller's index, three words a record
  const uint32_t* order;          // sorted position -> the caller's index
  const float* u;                 // [n_ticks][n_act]
  unsigned long long* a_skipped;  // counter "actuators_skipped"
  // the trace: BatchDevArgs' view of the outputs
  const int32_t* body;            // traced body i is body body[i] of the batch (flat index); null: body i
  float *x, *q, *v, *om;          // [n_ticks][m][3 | 4 | 3 | 3], null: not asked for
  unsigned long long* v_skipped;  // counter "device_skipped"
  uint32_t n_runs, n_act, m, total, n_worlds, tick, count;
};

template <int MODE>
__global__ __launch_bounds__(kBatchBlock) void k_batch_rollout_act(BatchRolloutArgs A) {
  const uint32_t r = blockIdx.x * kBatchBlock + threadIdx.x;
  const bool in = r < A.n_runs;
  const uint4 run = in ? A.runs[r] : make_uint4(0u, 0u, 0u, 0u);
  const bool live = in && A.done[run.x] == A.tick && A.act[run.x] == A.tick;  // the tick gate, a lane's own
  const uint32_t cnt = live ? run.w : 0u;
  const size_t g = live ? (size_t)A.w_off[run.x] + run.y : 0;
  const float* u = A.u + (size_t)A.tick * A.n_act;
  const Bodies& B = A.B;
  Quat rot = mkq(1.0f, mk3(0.0f, 0.0f, 0.0f));
  float4 k0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), k1 = k0, s2 = k0, s3 = k0;  // IMPULSE: srec words 0 and 1; FORCE: sp0 and sp1
  if (live) {
    const float4 bq = B.q[g];
    rot = mkq(bq.x, mk3(bq.y, bq.z, bq.w));
    if (MODE == ACTUATE_IMPULSE) { k0 = B.srec[4 * g]; k1 = B.srec[4 * g + 1]; s2 = B.srec[4 * g + 2]; s3 = B.srec[4 * g + 3]; }
    else { k0 = B.sp0[g]; k1 = B.sp1[g]; }
  }
  // IMPULSE: (v, omega) as batch_drive_apply unpacks them; FORCE: (force, torque)
  V3 lin = MODE == ACTUATE_IMPULSE ? mk3(k0.x, k0.y, k0.z) : xyz(k0);
  V3 ang = MODE == ACTUATE_IMPULSE ? mk3(k0.w, k1.x, k1.y) : xyz(k1);
  const float inv_mass = k1.z;
  const M3 I = m3_cols(mk3(k1.w, s2.x, s2.y), mk3(s2.z, s2.w, s3.x), mk3(s3.y, s3.z, s3.w));
  uint32_t n_skip = 0u;
  for (uint32_t j = 0u; __any(j < cnt); ++j) {
    if (j < cnt) {
      const size_t i = A.order[run.z + j];
      const float4 w0 = A.rig[3 * i], w1 = A.rig[3 * i + 1], w2 = A.rig[3 * i + 2];
      const uint32_t flags = f2u(w0.z);
      float c = u[i];
      if (c < w1.w) c = w1.w;
      if (c > w2.w) c = w2.w;
      const float s = w0.w * c;
      const V3 e = (flags & MGF_ACTUATOR_WORLD_DIR) ? xyz(w2) : rotate(rot, xyz(w2));
      V3 L, T;
      if (flags & MGF_ACTUATOR_TORQUE) {
        L = mk3(0.0f, 0.0f, 0.0f);
        T = e * s;
      } else {
        L = e * s;
        T = cross(rotate(rot, xyz(w1)), L);
      }
      if (!__builtin_isfinite(s)) {
        L = mk3(0.0f, 0.0f, 0.0f);
        T = L;
        ++n_skip;
      }
      if (MODE == ACTUATE_IMPULSE) {
        lin = lin + L * inv_mass;
        ang = ang + I * T;
      } else {
        lin = lin + L;
        ang = ang + T;
      }
    }
  }
  if (!live) return;
  if (MODE == ACTUATE_IMPULSE) {
    B.srec[4 * g] = make_float4(lin.x, lin.y, lin.z, ang.x);
    B.srec[4 * g + 1] = make_float4(ang.y, ang.z, k1.z, k1.w);
  } else {
    B.sp0[g] = mk4(lin, k0.w);
    B.sp1[g] = mk4(ang, k1.w);
  }
  if (n_skip) atomicAdd(A.a_skipped, (unsigned long long)n_skip);
}

__global__ __launch_bounds__(kBatchBlock) void k_batch_rollout_record(BatchRolloutArgs A) {
  const uint32_t i = blockIdx.x * kBatchBlock + threadIdx.x;
  const uint32_t t = A.tick;
  if (i < A.m) {
    const uint32_t gi = A.body ? (uint32_t)A.body[i] : i;
    if (gi >= A.total) {
      if (A.count) atomicAdd(A.v_skipped, 1ull);
    } else {
      // the body's world: the last k of [0, n_worlds) with w_off[k] <= gi (w_off[0] = 0, w_off[n_worlds] = total > gi; a world
      // without bodies shares its offset with the next and is passed over)
      uint32_t lo = 0u, hi = A.n_worlds;
      while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (A.w_off[mid] <= gi) lo = mid; else hi = mid;
      }
      if (A.done[lo] == t + 1u && A.act[lo] <= t + 1u) {
        const Bodies& B = A.B;
        const size_t g = gi, row = (size_t)t * A.m + i, r = 3 * row;
        if (A.x) { const V3 x = xyz(B.x[g]) + xyz(B.delta[g]); st3(A.x + r, x.x, x.y, x.z); }  // physics.rs:282, as k_batch_dev_gather
        if (A.q) { const float4 q = B.q[g]; float* o = A.q + 4 * row; o[0] = q.x; o[1] = q.y; o[2] = q.z; o[3] = q.w; }
        if (A.v || A.om) {
          const float4 s0 = B.srec[4 * g], s1 = B.srec[4 * g + 1];
          if (A.v) st3(A.v + r, s0.x, s0.y, s0.z);
          if (A.om) st3(A.om + r, s0.w, s1.x, s1.y);
        }
      }
    }
  }
  if (i < A.n_worlds && A.act[i] == t && A.done[i] >= t) A.act[i] = t + 1u;
}

}  // namespace mgf
