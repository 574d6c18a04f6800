// The skeleton of the joint solvers of a batch: one launch shape, one dataflow loop, for k_batch_joint_solve, k_batch_hinge_solve and
// k_batch_slider_solve (k_batch_joint.h, k_batch_hinge.h, k_batch_slider.h).  (Part of the kernel set described in kernels.h.)
//
// batch_joint_loop<Rows, GATED>: a workgroup per world that has joints of the kind, a lane per joint (at most kBatchBlock a world).  The
// world's named bodies are compacted to local SLOTS by the host plan (batch_joint_plan, host_batch_joint.inc); LDS holds 32 bytes a slot -
// srec words 0 and 1, (v, omega) as batch_drive_apply unpacks them - and one progress word a slot.  The lane runs its joint's setup from
// global memory - the state before the call - and keeps what Rows holds in registers for all sweeps.  The sweeps are k_batch_solve's
// dataflow: the per-world list order is a topological order of "joint j is body x's r-th joint", so the lane solves its joint of sweep
// `it` as soon as prog[sa] == it * deg[sa] + rank_a (and prog[sb] likewise), read with acquire loads at workgroup scope; it unpacks both
// bodies' (v, omega) once, applies ALL of the joint's rows with them in registers, packs them again and then release-stores both
// counters.  Ranks, degrees and slots are static and come from the plan: nothing is sorted or scanned here.  The earliest unsolved joint
// of a world is always ready, so the spin ends; it is bounded all the same (kBatchSpinLimit): a lane that gives up sets err[1] and the
// workgroup's flag, and the store-back is skipped - the world's velocities stay as the call found them.  That is a bug, never a wait for
// another workgroup: a workgroup waits for its own lanes alone.
// The loop has k_batch_solve's shape: every lane of a wave that still has a sweep to do takes every trip, the wave sleeps only where none
// of its lanes is ready (__any), and a lane that is not ready never holds back one that is.  GATED (a rollout) is the train's gate
// done[k] == tick && act[k] == tick (k_batch_rollout.h): the same for a whole workgroup, so it is an early return ahead of the first
// barrier, and a template argument so that nothing wave-uniform is evaluated inside the loop (DESIGN.md section 9,
// tools/check_lane_masks.py).  No float atomic, no scratch, vector stores only.
//
// Rows is the joint kind - JointRows, HingeRows, SliderRows, each in its kernel's file:
//   kWords, kFloats                          the record's words of 16 bytes (3 or 7); the impulse row's floats (3 or 8)
//   its members                              what the lane keeps in registers behind the setup, the accumulators among them; Rows{} is all zeros
//   bool setup(A, rec, i, g0, has_b)         SETUP of joint i from its record and the state before the call; true: the joint is skipped
//   void sweep(va, oa, vb, ob, has_b)        the rows of one turn, in the definition's order, over both bodies' velocities
//   void store(float* p)                     the impulse row
// Every member is __forceinline__ and every line a separate f32 operation (-ffp-contract=off).
#pragma once
#include "k_batch_spring.h"

namespace mgf {

constexpr uint32_t kJointNoSlot = 0xFFFFu;  // slot_b of a joint to a world anchor

struct BatchJointArgs {
  Bodies B;                     // every world's bodies
  const uint32_t* w_off;        // the worlds' first bodies
  const uint4* items;           // item w: (world, first sorted position, count | slots << 16, first slot)
  const float4* rig;            // by the caller's index, Rows::kWords words a record: (world, body, other, flags) (pa, beta) (pb, ..) ...
  const uint4* plan;            // sorted position -> (the caller's index, slot_a | slot_b << 16, rank_a | rank_b << 16, 0); slots local to the item
  const uint2* slots;           // slot -> (body, deg): the joints that name the body
  const float* w;               // the target table's row for this call: a float a joint, by the caller's index; null: the ball joints, which have none
  float* acc;                   // the handle's: Rows::kFloats floats a joint, the impulse over the call, by the caller's index
  float* out;                   // the caller's, the same rows; null: not asked for
  unsigned long long* skipped;  // joints that were skipped, cumulative (counters "joints_skipped", "hinges_skipped", "sliders_skipped")
  uint32_t* err;                // the handle's error words: [1] a lane gave up waiting for its turn
  const uint32_t* done;         // a rollout: ticks of the call world k has completed (BatchArgs::done); null: a call of its own
  const uint32_t* act;          // a rollout: ticks whose actuation world k has behind it (BatchRolloutArgs::act)
  float h;                      // the time step
  uint32_t iters, tick;
};

// One end of a joint as the state stands: q, x + delta (physics.rs:282, as k_batch_dev_gather), omega (srec words 0 and 1), im and I
// (srec words 1 to 3).  What a kernel does not read of it is never loaded.
struct JointEnd {
  Quat q;
  V3 x, om;
  float im;
  M3 I;
};

__device__ __forceinline__ JointEnd joint_end(const Bodies& B, size_t g) {
  const float4 q = B.q[g], s0 = B.srec[4 * g], s1 = B.srec[4 * g + 1], s2 = B.srec[4 * g + 2], s3 = B.srec[4 * g + 3];
  JointEnd e;
  e.q = mkq(q.x, mk3(q.y, q.z, q.w));
  e.x = xyz(B.x[g]) + xyz(B.delta[g]);
  e.om = mk3(s0.w, s1.x, s1.y);
  e.im = s1.z;
  e.I = m3_cols(mk3(s1.w, s2.x, s2.y), mk3(s2.z, s2.w, s3.x), mk3(s3.y, s3.z, s3.w));
  return e;
}

// other == -1, the far end is the world: at rest at the origin, im = 0, I = 0
__device__ __forceinline__ JointEnd joint_end_world() {
  JointEnd e;
  e.q = mkq(1.0f, mk3(0.0f, 0.0f, 0.0f));
  e.x = mk3(0.0f, 0.0f, 0.0f);
  e.om = e.x;
  e.im = 0.0f;
  e.I = m3_cols(e.x, e.x, e.x);
  return e;
}

// both ends of the record whose first word is w0, (world, body, other, flags); g0: the world's first body
__device__ __forceinline__ void joint_ends(const Bodies& B, size_t g0, float4 w0, bool has_b, JointEnd* a, JointEnd* b) {
  *a = joint_end(B, g0 + f2u(w0.y));
  *b = joint_end_world();
  if (has_b) *b = joint_end(B, g0 + f2u(w0.z));
}

__device__ __forceinline__ bool joint_finite(float a) { return __builtin_isfinite(a); }
__device__ __forceinline__ bool joint_finite3(V3 a) { return __builtin_isfinite(a.x) && __builtin_isfinite(a.y) && __builtin_isfinite(a.z); }
__device__ __forceinline__ bool joint_finite9(const M3& m) { return joint_finite3(m.c[0]) && joint_finite3(m.c[1]) && joint_finite3(m.c[2]); }

// The inverse of the 2 x 2 block (k11 k12; k21 k22) of a pair of rows; d2 == 0: the joint is skipped
struct JointInv2 {
  float d2, m11, m12, m21, m22;
};

__device__ __forceinline__ JointInv2 joint_inv2(float k11, float k12, float k21, float k22) {
  JointInv2 m;
  m.d2 = k11 * k22 - k12 * k21;
  m.m11 = k22 / m.d2;
  m.m12 = -k12 / m.d2;
  m.m21 = -k21 / m.d2;
  m.m22 = k11 / m.d2;
  return m;
}

// A motor row's impulse: lam = (w - rate) / Km, the sum am held in [-mmax, mmax]; what the clamp leaves of lam is returned
__device__ __forceinline__ float joint_motor_lam(float w, float rate, float Km, float mmax, float& am) {
  const float lam = (w - rate) / Km;
  float t = am + lam;
  if (t < -mmax) t = -mmax;
  if (t > mmax) t = mmax;
  const float out = t - am;
  am = t;
  return out;
}

// A limit row's impulse: lam = (lb - rate) / Km, the sum al held at or above 0 (side == -1) or at or below 0 (side == +1); any other
// side - a lock - is not clamped
__device__ __forceinline__ float joint_limit_lam(float lb, float rate, float Km, int32_t side, float& al) {
  const float lam = (lb - rate) / Km;
  float t = al + lam;
  if (side == -1) { if (t < 0.0f) t = 0.0f; }
  if (side == 1) { if (t > 0.0f) t = 0.0f; }
  const float out = t - al;
  al = t;
  return out;
}

template <class Rows, bool GATED>
__device__ __forceinline__ void batch_joint_loop(const BatchJointArgs& A) {
  extern __shared__ float4 s_dyn[];  // two words a slot: srec words 0 and 1; behind them a progress word a slot
  __shared__ uint32_t s_fail;
  const uint4 item = A.items[blockIdx.x];
  const uint32_t k = item.x, tid = threadIdx.x;
  if (GATED && !(A.done[k] == A.tick && A.act[k] == A.tick)) return;  // the tick gate: the workgroup's, ahead of the first barrier
  const uint32_t cnt = item.z & 0xFFFFu, ns = item.z >> 16;
  uint32_t* s_prog = reinterpret_cast<uint32_t*>(s_dyn + 2 * (size_t)ns);
  const size_t g0 = A.w_off[k];
  float4* srec = A.B.srec + 4 * g0;
  const uint2* slot = A.slots + item.w;
  for (uint32_t s = tid; s < ns; s += kBatchBlock) {
    const uint32_t body = slot[s].x;
    s_dyn[2 * s] = srec[4 * (size_t)body];
    s_dyn[2 * s + 1] = srec[4 * (size_t)body + 1];
    s_prog[s] = 0u;
  }
  if (tid == 0) s_fail = 0u;
  // the lane's joint: the plan's words, and the setup from the state before the call
  const bool mine = tid < cnt;
  uint32_t i = 0, sa = 0, sb = 0, need_a = 0, need_b = 0, deg_a = 0, deg_b = 0;
  bool has_b = false, skip = false;
  Rows R{};
  if (mine) {
    const uint4 pl = A.plan[item.y + tid];
    i = pl.x;
    sa = pl.y & 0xFFFFu; sb = pl.y >> 16;
    need_a = pl.z & 0xFFFFu; need_b = pl.z >> 16;
    has_b = sb != kJointNoSlot;
    deg_a = slot[sa].y;
    if (has_b) deg_b = slot[sb].y;
    skip = R.setup(A, A.rig + Rows::kWords * (size_t)i, i, g0, has_b);
    if (skip) atomicAdd(A.skipped, 1ull);
  }
  __syncthreads();
  {
    uint32_t it = 0, spins = 0;
    bool open = mine && A.iters != 0u;
    while (open) {
      bool ready = __hip_atomic_load(&s_prog[sa], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) == need_a;
      if (ready && has_b) ready = __hip_atomic_load(&s_prog[sb], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) == need_b;
      if (!__any(ready)) __builtin_amdgcn_s_sleep(1);  // (a wave-wide step of every trip: lanes that wait never hold back lanes of their wave that can run)
      if (ready) {
        if (!skip) {
          const float4 a0 = s_dyn[2 * sa], a1 = s_dyn[2 * sa + 1];
          V3 va = mk3(a0.x, a0.y, a0.z), oa = mk3(a0.w, a1.x, a1.y);
          float4 b0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b1 = b0;
          if (has_b) { b0 = s_dyn[2 * sb]; b1 = s_dyn[2 * sb + 1]; }
          V3 vb = mk3(b0.x, b0.y, b0.z), ob = mk3(b0.w, b1.x, b1.y);
          R.sweep(va, oa, vb, ob, has_b);
          s_dyn[2 * sa] = make_float4(va.x, va.y, va.z, oa.x);
          s_dyn[2 * sa + 1] = make_float4(oa.y, oa.z, a1.z, a1.w);
          if (has_b) {
            s_dyn[2 * sb] = make_float4(vb.x, vb.y, vb.z, ob.x);
            s_dyn[2 * sb + 1] = make_float4(ob.y, ob.z, b1.z, b1.w);
          }
        }
        __hip_atomic_store(&s_prog[sa], need_a + 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (has_b) __hip_atomic_store(&s_prog[sb], need_b + 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        spins = 0;
        ++it;
        need_a += deg_a;
        need_b += deg_b;
        if (it >= A.iters) open = false;
      } else if (++spins > kBatchSpinLimit) {
        A.err[1] = 1u;
        s_fail = 1u;
        open = false;
      }
    }
  }
  __syncthreads();
  if (s_fail != 0u) return;  // (the workgroup's: the world's velocities stay as the call found them)
  for (uint32_t s = tid; s < ns; s += kBatchBlock) {
    const uint32_t body = slot[s].x;
    srec[4 * (size_t)body] = s_dyn[2 * s];
    srec[4 * (size_t)body + 1] = s_dyn[2 * s + 1];
  }
  if (mine) {
    R.store(A.acc + Rows::kFloats * (size_t)i);
    if (A.out) R.store(A.out + Rows::kFloats * (size_t)i);
  }
}

}  // namespace mgf
