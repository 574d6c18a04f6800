// Ball joints between the bodies of a batch (mgf_batch_set_joints, mgf_batch_solve_joints, mgf_batch_solve_joints_dev, and ahead of
// every tick of a rollout; host_batch_joint.inc).
// (Part of the kernel set described in kernels.h.)
//
// A joint is a point-to-point constraint between two body-fixed points, or between one and a point of the world: (world, body, other,
// flags, pa, beta, pb, pad), three 16-byte words.  A call is sequential impulses over the resident velocities - every line a separate
// f32 operation, rotate, cross, dot, M3 * V3 and invert dev_math.h's.  SETUP per joint, from the state before the call:
//   ra = rotate(q_a, pa);  Pa = x_a + ra
//   other >= 0:  rb = rotate(q_b, pb);  Pb = x_b + rb;  im_b, I_b the body's        other == -1:  rb = 0;  Pb = pb;  im_b = 0;  I_b = 0
//   C = Pb - Pa;  s = beta / h;  bias = C * s
//   column k of K:  (e_k * im_a + cross(I_a * cross(ra, e_k), ra)) + (e_k * im_b + cross(I_b * cross(rb, e_k), rb));  Kinv = invert(K)
//   skipped: det == 0, or a word of ra, rb, bias or Kinv not finite - no velocity touched, a zero impulse, its place in the order kept
// SWEEPS, `iters` times over a world's joints in list order:
//   Va = v_a + cross(omega_a, ra);  Vb = v_b + cross(omega_b, rb)  (other == -1: Vb = 0);  P = Kinv * ((Vb - Va) + bias)
//   v_a = v_a + P * im_a;  omega_a = omega_a + I_a * cross(ra, P);  Pn = -P;  v_b = v_b + Pn * im_b;  omega_b = omega_b + I_b * cross(rb, Pn)
//   acc = acc + P
// One launch, k_batch_joint_solve<GATED>: a workgroup per world that has joints, a lane per joint (MGF_BATCH_MAX_WORLD_JOINTS =
// kBatchBlock).  The lane runs its joint's setup from global memory and keeps ra, rb, bias, Kinv, im and I of both ends in registers
// for all sweeps.  The world's jointed bodies are compacted to local SLOTS by the host plan; LDS holds 32 bytes a slot - srec words 0
// and 1, (v, omega) as batch_drive_apply unpacks them - and one progress word a slot.  The sweeps are k_batch_solve's dataflow: the
// per-world list order is a topological order of "joint j is body x's r-th joint", so the lane solves its joint of sweep `it` as soon
// as prog[sa] == it * deg[sa] + rank_a (and prog[sb] likewise), read with acquire loads at workgroup scope; it writes the velocities
// and then release-stores both counters.  Ranks, degrees and slots are static and come from the plan: nothing is sorted or scanned
// here.  The earliest unsolved joint of a world is always ready, so the spin ends; it is bounded all the same (kBatchSpinLimit): a
// lane that gives up sets err[1] and the workgroup's flag, and the store-back is skipped - the world's velocities stay as the call
// found them.  That is a bug, never a wait for another workgroup: a workgroup waits for its own lanes alone.
// The loop has k_batch_solve's shape: every lane of a wave that still has a sweep to do takes every trip, the wave sleeps only where
// none of its lanes is ready (__any), and a lane that is not ready never holds back one that is.  GATED (a rollout) is the train's gate
// done[k] == tick && act[k] == tick (k_batch_rollout.h): the same for a whole workgroup, so it is an early return ahead of the first
// barrier, and a template argument so that nothing wave-uniform is evaluated inside the loop (DESIGN.md section 9,
// tools/check_lane_masks.py).  No float atomic, no scratch, vector stores only.
#pragma once
#include "k_batch_spring.h"

namespace mgf {

constexpr uint32_t kJointNoSlot = 0xFFFFu;  // slot_b of a joint to a world anchor

struct BatchJointArgs {
  Bodies B;                     // every world's bodies
  const uint32_t* w_off;        // the worlds' first bodies
  const uint4* items;           // item w: (world, first sorted position, count | slots << 16, first slot)
  const float4* rig;            // by the caller's index, three words a record: (world, body, other, flags) (pa, beta) (pb, pad)
  const uint4* plan;            // sorted position -> (the caller's index, slot_a | slot_b << 16, rank_a | rank_b << 16, 0); slots local to the item
  const uint2* slots;           // slot -> (body, deg): the joints that name the body
  float* acc;                   // the handle's: three floats a joint, the impulse over the call, by the caller's index
  float* out;                   // the caller's, the same rows; null: not asked for
  unsigned long long* skipped;  // joints that were skipped, cumulative (counter "joints_skipped")
  uint32_t* err;                // the handle's error words: [1] a lane gave up waiting for its turn
  const uint32_t* done;         // a rollout: ticks of the call world k has completed (BatchArgs::done); null: a call of its own
  const uint32_t* act;          // a rollout: ticks whose actuation world k has behind it (BatchRolloutArgs::act)
  float h;                      // the time step
  uint32_t iters, tick;
};

__device__ __forceinline__ bool joint_finite3(V3 a) { return __builtin_isfinite(a.x) && __builtin_isfinite(a.y) && __builtin_isfinite(a.z); }

// column k of K for one end: e_k * im + cross(I * cross(r, e_k), r)
__device__ __forceinline__ V3 joint_k_col(V3 e, float im, const M3& I, V3 r) { return e * im + cross(I * cross(r, e), r); }

template <bool GATED>
__global__ __launch_bounds__(kBatchBlock) void k_batch_joint_solve(BatchJointArgs A) {
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
  // the lane's joint: setup from the state before the call
  const bool mine = tid < cnt;
  uint32_t i = 0, sa = 0, sb = 0, need_a = 0, need_b = 0, deg_a = 0, deg_b = 0;
  bool has_b = false, skip = false;
  V3 ra = mk3(0.0f, 0.0f, 0.0f), rb = ra, bias = ra, acc = ra;
  float im_a = 0.0f, im_b = 0.0f;
  M3 I_a = m3_cols(ra, ra, ra), I_b = I_a, Kinv = I_a;
  if (mine) {
    const Bodies& B = A.B;
    const uint4 pl = A.plan[item.y + tid];
    i = pl.x;
    sa = pl.y & 0xFFFFu; sb = pl.y >> 16;
    need_a = pl.z & 0xFFFFu; need_b = pl.z >> 16;
    has_b = sb != kJointNoSlot;
    deg_a = slot[sa].y;
    const float4 w0 = A.rig[3 * (size_t)i], w1 = A.rig[3 * (size_t)i + 1], w2 = A.rig[3 * (size_t)i + 2];
    const size_t ga = g0 + f2u(w0.y);
    const float4 qa = B.q[ga], a1 = B.srec[4 * ga + 1], a2 = B.srec[4 * ga + 2], a3 = B.srec[4 * ga + 3];
    const V3 xa = xyz(B.x[ga]) + xyz(B.delta[ga]);  // physics.rs:282, as k_batch_dev_gather
    ra = rotate(mkq(qa.x, mk3(qa.y, qa.z, qa.w)), xyz(w1));
    const V3 Pa = xa + ra;
    im_a = a1.z;
    I_a = m3_cols(mk3(a1.w, a2.x, a2.y), mk3(a2.z, a2.w, a3.x), mk3(a3.y, a3.z, a3.w));
    V3 Pb = xyz(w2);
    if (has_b) {
      deg_b = slot[sb].y;
      const size_t gb = g0 + f2u(w0.z);
      const float4 qb = B.q[gb], b1 = B.srec[4 * gb + 1], b2 = B.srec[4 * gb + 2], b3 = B.srec[4 * gb + 3];
      const V3 xb = xyz(B.x[gb]) + xyz(B.delta[gb]);
      rb = rotate(mkq(qb.x, mk3(qb.y, qb.z, qb.w)), xyz(w2));
      Pb = xb + rb;
      im_b = b1.z;
      I_b = m3_cols(mk3(b1.w, b2.x, b2.y), mk3(b2.z, b2.w, b3.x), mk3(b3.y, b3.z, b3.w));
    }
    const V3 C = Pb - Pa;
    const float s = w1.w / A.h;
    bias = C * s;
    const V3 e0 = mk3(1.0f, 0.0f, 0.0f), e1 = mk3(0.0f, 1.0f, 0.0f), e2 = mk3(0.0f, 0.0f, 1.0f);
    const M3 K = m3_cols(joint_k_col(e0, im_a, I_a, ra) + joint_k_col(e0, im_b, I_b, rb), joint_k_col(e1, im_a, I_a, ra) + joint_k_col(e1, im_b, I_b, rb),
                         joint_k_col(e2, im_a, I_a, ra) + joint_k_col(e2, im_b, I_b, rb));
    const bool ok = invert(K, &Kinv);
    skip = !ok || !joint_finite3(ra) || !joint_finite3(rb) || !joint_finite3(bias) || !joint_finite3(Kinv.c[0]) || !joint_finite3(Kinv.c[1]) ||
           !joint_finite3(Kinv.c[2]);
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
          const V3 Va = va + cross(oa, ra);
          V3 Vb = vb + cross(ob, rb);
          if (!has_b) Vb = mk3(0.0f, 0.0f, 0.0f);
          const V3 P = Kinv * ((Vb - Va) + bias);
          va = va + P * im_a;
          oa = oa + I_a * cross(ra, P);
          s_dyn[2 * sa] = make_float4(va.x, va.y, va.z, oa.x);
          s_dyn[2 * sa + 1] = make_float4(oa.y, oa.z, a1.z, a1.w);
          if (has_b) {
            const V3 Pn = -P;
            vb = vb + Pn * im_b;
            ob = ob + I_b * cross(rb, Pn);
            s_dyn[2 * sb] = make_float4(vb.x, vb.y, vb.z, ob.x);
            s_dyn[2 * sb + 1] = make_float4(ob.y, ob.z, b1.z, b1.w);
          }
          acc = acc + P;
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
    st3(A.acc + 3 * (size_t)i, acc.x, acc.y, acc.z);
    if (A.out) st3(A.out + 3 * (size_t)i, acc.x, acc.y, acc.z);
  }
}

}  // namespace mgf
