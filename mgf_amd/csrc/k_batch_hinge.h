// Hinge joints between the bodies of a batch (mgf_batch_set_hinges, mgf_batch_set_hinge_targets, mgf_batch_solve_hinges,
// mgf_batch_solve_hinges_dev, and ahead of every tick of a rollout; host_batch_hinge.inc).
// (Part of the kernel set described in kernels.h.)
//
// A hinge is a ball joint (k_batch_joint.h) plus two angular rows that keep the two hinge axes parallel, an optional limit of the hinge
// angle and an optional velocity motor with a torque cap: (world, body, other, flags, pa, beta, pb, tmax, ax, cm, ua, sm, bx, ch, ub,
// sh), seven 16-byte words.  The definition stands in include/mgf_hip.h, every line a separate f32 operation; here in short.  SETUP per
// hinge, from the state before the call: ra, rb, Pa, Pb, C, s, bias, K and Kinv are the ball joint's lines;
//   A = rotate(q_a, ax);  T1 = rotate(q_a, ua);  T2 = cross(A, T1);  B = rotate(q_b, bx);  U1 = rotate(q_b, ub)   (other == -1: B = bx, U1 = ub)
//   n1 = cross(B, T1);  n2 = cross(B, T2);  g1 = dot(B, T1) * s;  g2 = dot(B, T2) * s;  J(n) = I_a * n + I_b * n
//   k_ij = dot(n_i, J(n_j));  d2 = k11 * k22 - k12 * k21;  m11 = k22 / d2;  m12 = -k12 / d2;  m21 = -k21 / d2;  m22 = k11 / d2;  Km = dot(A, J(A))
//   c = dot(U1, T1);  sn = dot(U1, T2);  cphi = c * cm + sn * sm;  sphi = sn * cm - c * sm
//   LIMIT and cphi <= ch:  err = fabs(sphi) * ch - cphi * sh;  sphi >= 0: side = +1, lb = -(err * s);  else side = -1, lb = err * s
//   MOTOR:  mmax = tmax * h;  w = the target row's entry i
// SWEEPS in list order, the rows of one hinge in the order motor, limit, angular, point, wd = omega_b - omega_a formed again ahead of
// each of the first three - the `hinge row` lines of the loop below.
// One launch, k_batch_hinge_solve<GATED>, with k_batch_joint_solve's shape and rules: a workgroup per world that has hinges, a lane per
// hinge (MGF_BATCH_MAX_WORLD_HINGES = kBatchBlock); the world's hinged bodies in LDS slots of 32 bytes - srec words 0 and 1 - and a
// progress word a slot; the plan is batch_joint_plan's (ranks, degrees, slots: nothing sorted or scanned here); the lane solves its hinge
// of sweep `it` once prog[sa] == it * deg[sa] + rank_a (and prog[sb] likewise), read with acquire loads at workgroup scope, ALL FOUR rows
// in one turn with both bodies' (v, omega) in registers between the rows, writes the velocities and release-stores both counters once.
// Every lane of a wave that has a sweep left takes every trip, the wave sleeps only where none of its lanes is ready (__any), the spin
// is bounded (kBatchSpinLimit): a lane that gives up sets err[1] and the workgroup's flag, and the store-back is skipped.  GATED (a
// rollout) is the train's gate done[k] == tick && act[k] == tick, the same for a whole workgroup: an early return ahead of the first
// barrier, and a template argument so that nothing wave-uniform is evaluated inside the loop (DESIGN.md section 9,
// tools/check_lane_masks.py).  The lane keeps ra, rb, bias, Kinv, im and I of both ends, A, n1, n2, g1, g2, m**, Km, lb, mmax, w and its
// seven accumulators in registers: a workgroup of 256 lanes is one wave per SIMD.  No float atomic, no scratch, vector stores only.
#pragma once
#include "k_batch_joint.h"

namespace mgf {

constexpr uint32_t kHingeLimit = 1u, kHingeMotor = 2u;  // MGF_HINGE_LIMIT, MGF_HINGE_MOTOR

struct BatchHingeArgs {
  Bodies B;                     // every world's bodies
  const uint32_t* w_off;        // the worlds' first bodies
  const uint4* items;           // item w: (world, first sorted position, count | slots << 16, first slot)
  const float4* rig;            // by the caller's index, seven words a record
  const uint4* plan;            // sorted position -> (the caller's index, slot_a | slot_b << 16, rank_a | rank_b << 16, 0); slots local to the item
  const uint2* slots;           // slot -> (body, deg): the hinges that name the body
  const float* w;               // the target table's row for this call: a float a hinge, by the caller's index
  float* acc;                   // the handle's: eight floats a hinge - (acc.x, acc.y, acc.z, a1, a2, al, am, 0) - by the caller's index
  float* out;                   // the caller's, the same rows; null: not asked for
  unsigned long long* skipped;  // hinges that were skipped, cumulative (counter "hinges_skipped")
  uint32_t* err;                // the handle's error words: [1] a lane gave up waiting for its turn
  const uint32_t* done;         // a rollout: ticks of the call world k has completed (BatchArgs::done); null: a call of its own
  const uint32_t* act;          // a rollout: ticks whose actuation world k has behind it (BatchRolloutArgs::act)
  float h;                      // the time step
  uint32_t iters, tick;
};

__device__ __forceinline__ bool hinge_finite(float a) { return __builtin_isfinite(a); }
// J(n) = I_a * n + I_b * n
__device__ __forceinline__ V3 hinge_j(const M3& I_a, const M3& I_b, V3 n) { return I_a * n + I_b * n; }
__device__ __forceinline__ void hinge_st8(float* p, V3 acc, float a1, float a2, float al, float am) {
  p[0] = acc.x; p[1] = acc.y; p[2] = acc.z; p[3] = a1; p[4] = a2; p[5] = al; p[6] = am; p[7] = 0.0f;
}

template <bool GATED>
__global__ __launch_bounds__(kBatchBlock) void k_batch_hinge_solve(BatchHingeArgs A) {
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
  // the lane's hinge: setup from the state before the call
  const bool mine = tid < cnt;
  uint32_t i = 0, sa = 0, sb = 0, need_a = 0, need_b = 0, deg_a = 0, deg_b = 0;
  bool has_b = false, skip = false, motor = false;
  int32_t side = 0;
  V3 ra = mk3(0.0f, 0.0f, 0.0f), rb = ra, bias = ra, acc = ra, hA = ra, n1 = ra, n2 = ra;
  float im_a = 0.0f, im_b = 0.0f, g1 = 0.0f, g2 = 0.0f, m11 = 0.0f, m12 = 0.0f, m21 = 0.0f, m22 = 0.0f, Km = 0.0f, lb = 0.0f, mmax = 0.0f, wt = 0.0f;
  float a1 = 0.0f, a2 = 0.0f, al = 0.0f, am = 0.0f;
  M3 I_a = m3_cols(ra, ra, ra), I_b = I_a, Kinv = I_a;
  if (mine) {
    const Bodies& B = A.B;
    const uint4 pl = A.plan[item.y + tid];
    i = pl.x;
    sa = pl.y & 0xFFFFu; sb = pl.y >> 16;
    need_a = pl.z & 0xFFFFu; need_b = pl.z >> 16;
    has_b = sb != kJointNoSlot;
    deg_a = slot[sa].y;
    const float4* rec = A.rig + 7 * (size_t)i;
    const float4 w0 = rec[0], w1 = rec[1], w2 = rec[2], w3 = rec[3], w4 = rec[4], w5 = rec[5], w6 = rec[6];
    const uint32_t flags = f2u(w0.w);
    motor = (flags & kHingeMotor) != 0u;
    const size_t ga = g0 + f2u(w0.y);
    const float4 qa = B.q[ga], s1 = B.srec[4 * ga + 1], s2 = B.srec[4 * ga + 2], s3 = B.srec[4 * ga + 3];
    const V3 xa = xyz(B.x[ga]) + xyz(B.delta[ga]);  // physics.rs:282, as k_batch_dev_gather
    const Quat Qa = mkq(qa.x, mk3(qa.y, qa.z, qa.w));
    ra = rotate(Qa, xyz(w1));
    const V3 Pa = xa + ra;
    im_a = s1.z;
    I_a = m3_cols(mk3(s1.w, s2.x, s2.y), mk3(s2.z, s2.w, s3.x), mk3(s3.y, s3.z, s3.w));
    hA = rotate(Qa, xyz(w3));
    const V3 T1 = rotate(Qa, xyz(w4));
    const V3 T2 = cross(hA, T1);
    V3 Pb = xyz(w2), Bx = xyz(w5), U1 = xyz(w6);
    if (has_b) {
      deg_b = slot[sb].y;
      const size_t gb = g0 + f2u(w0.z);
      const float4 qb = B.q[gb], b1 = B.srec[4 * gb + 1], b2 = B.srec[4 * gb + 2], b3 = B.srec[4 * gb + 3];
      const V3 xb = xyz(B.x[gb]) + xyz(B.delta[gb]);
      const Quat Qb = mkq(qb.x, mk3(qb.y, qb.z, qb.w));
      rb = rotate(Qb, xyz(w2));
      Pb = xb + rb;
      im_b = b1.z;
      I_b = m3_cols(mk3(b1.w, b2.x, b2.y), mk3(b2.z, b2.w, b3.x), mk3(b3.y, b3.z, b3.w));
      Bx = rotate(Qb, xyz(w5));
      U1 = rotate(Qb, xyz(w6));
    }
    const V3 C = Pb - Pa;
    const float s = w1.w / A.h;
    bias = C * s;
    const V3 e0 = mk3(1.0f, 0.0f, 0.0f), e1 = mk3(0.0f, 1.0f, 0.0f), e2 = mk3(0.0f, 0.0f, 1.0f);
    const M3 K = m3_cols(joint_k_col(e0, im_a, I_a, ra) + joint_k_col(e0, im_b, I_b, rb), joint_k_col(e1, im_a, I_a, ra) + joint_k_col(e1, im_b, I_b, rb),
                         joint_k_col(e2, im_a, I_a, ra) + joint_k_col(e2, im_b, I_b, rb));
    const bool ok = invert(K, &Kinv);
    n1 = cross(Bx, T1);
    n2 = cross(Bx, T2);
    g1 = dot(Bx, T1) * s;
    g2 = dot(Bx, T2) * s;
    const V3 j1 = hinge_j(I_a, I_b, n1), j2 = hinge_j(I_a, I_b, n2);
    const float k11 = dot(n1, j1), k12 = dot(n1, j2), k21 = dot(n2, j1), k22 = dot(n2, j2);
    const float d2 = k11 * k22 - k12 * k21;
    m11 = k22 / d2;
    m12 = -k12 / d2;
    m21 = -k21 / d2;
    m22 = k11 / d2;
    Km = dot(hA, hinge_j(I_a, I_b, hA));
    const float c = dot(U1, T1), sn = dot(U1, T2);
    const float cphi = c * w3.w + sn * w4.w, sphi = sn * w3.w - c * w4.w;
    if ((flags & kHingeLimit) != 0u && cphi <= w5.w) {
      const float e = fabs_rs(sphi) * w5.w - cphi * w6.w;
      if (sphi >= 0.0f) { side = 1; lb = -(e * s); }
      else { side = -1; lb = e * s; }
    }
    if (motor) {
      mmax = w2.w * A.h;
      wt = A.w[i];
    }
    skip = !ok || !joint_finite3(ra) || !joint_finite3(rb) || !joint_finite3(bias) || !joint_finite3(Kinv.c[0]) || !joint_finite3(Kinv.c[1]) ||
           !joint_finite3(Kinv.c[2]) || d2 == 0.0f || ((flags & (kHingeLimit | kHingeMotor)) != 0u && Km == 0.0f) || !joint_finite3(n1) || !joint_finite3(n2) ||
           !hinge_finite(g1) || !hinge_finite(g2) || !hinge_finite(m11) || !hinge_finite(m12) || !hinge_finite(m21) || !hinge_finite(m22) || !hinge_finite(Km) ||
           !hinge_finite(lb) || (motor && (mmax != mmax || !hinge_finite(wt)));
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
          const float4 a0 = s_dyn[2 * sa], aw = s_dyn[2 * sa + 1];
          V3 va = mk3(a0.x, a0.y, a0.z), oa = mk3(a0.w, aw.x, aw.y);
          float4 b0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), bw = b0;
          if (has_b) { b0 = s_dyn[2 * sb]; bw = s_dyn[2 * sb + 1]; }
          V3 vb = mk3(b0.x, b0.y, b0.z), ob = mk3(b0.w, bw.x, bw.y);
          if (motor) {  // hinge row: the motor
            const V3 wd = ob - oa;
            float lam = (wt - dot(wd, hA)) / Km;
            float t = am + lam;
            if (t < -mmax) t = -mmax;
            if (t > mmax) t = mmax;
            lam = t - am;
            am = t;
            const V3 imp = hA * lam;
            oa = oa - I_a * imp;
            if (has_b) ob = ob + I_b * imp;
          }
          if (side != 0) {  // hinge row: the limit
            const V3 wd = ob - oa;
            float lam = (lb - dot(wd, hA)) / Km;
            float t = al + lam;
            if (side < 0) { if (t < 0.0f) t = 0.0f; }
            else { if (t > 0.0f) t = 0.0f; }
            lam = t - al;
            al = t;
            const V3 imp = hA * lam;
            oa = oa - I_a * imp;
            if (has_b) ob = ob + I_b * imp;
          }
          {  // hinge row: the two angular rows
            const V3 wd = ob - oa;
            const float r1 = dot(wd, n1) + g1, r2 = dot(wd, n2) + g2;
            const float l1 = -(m11 * r1 + m12 * r2), l2 = -(m21 * r1 + m22 * r2);
            const V3 imp = n1 * l1 + n2 * l2;
            oa = oa - I_a * imp;
            if (has_b) ob = ob + I_b * imp;
            a1 = a1 + l1;
            a2 = a2 + l2;
          }
          {  // hinge row: the point, the ball joint's lines
            const V3 Va = va + cross(oa, ra);
            V3 Vb = vb + cross(ob, rb);
            if (!has_b) Vb = mk3(0.0f, 0.0f, 0.0f);
            const V3 P = Kinv * ((Vb - Va) + bias);
            va = va + P * im_a;
            oa = oa + I_a * cross(ra, P);
            if (has_b) {
              const V3 Pn = -P;
              vb = vb + Pn * im_b;
              ob = ob + I_b * cross(rb, Pn);
            }
            acc = acc + P;
          }
          s_dyn[2 * sa] = make_float4(va.x, va.y, va.z, oa.x);
          s_dyn[2 * sa + 1] = make_float4(oa.y, oa.z, aw.z, aw.w);
          if (has_b) {
            s_dyn[2 * sb] = make_float4(vb.x, vb.y, vb.z, ob.x);
            s_dyn[2 * sb + 1] = make_float4(ob.y, ob.z, bw.z, bw.w);
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
    hinge_st8(A.acc + 8 * (size_t)i, acc, a1, a2, al, am);
    if (A.out) hinge_st8(A.out + 8 * (size_t)i, acc, a1, a2, al, am);
  }
}

}  // namespace mgf
