// Slider joints between the bodies of a batch (mgf_batch_set_sliders, mgf_batch_set_slider_targets, mgf_batch_solve_sliders,
// mgf_batch_solve_sliders_dev, and ahead of every tick of a rollout; host_batch_slider.inc).
// (Part of the kernel set described in kernels.h.)
//
// A slider (prismatic joint) holds the frame of `other` onto the frame of `body` (three angular rows), holds other's anchor on the axis
// through body's anchor (two linear rows) and leaves the travel d along that axis free - or limits it, drives it with a velocity motor
// with a force cap, or locks it (a weld): (world, body, other, flags, pa, beta, pb, fmax, ax, lo, ua, hi, bx, pad0, ub, pad1), seven
// 16-byte words, the hinge's layout.  The definition stands in include/mgf_hip.h, every line a separate f32 operation; here in short.
// SETUP per slider, from the state before the call: ra, rb, Pa, Pb, C = Pb - Pa and s = beta / h are the ball joint's lines;
//   A = rotate(q_a, ax);  T1 = rotate(q_a, ua);  T2 = cross(A, T1);  B = rotate(q_b, bx);  U1 = rotate(q_b, ub)   (other == -1: B = bx, U1 = ub)
//   U2 = cross(B, U1);  ca = ra + C;  d = dot(C, A);  ims = im_a + im_b
//   sA = cross(ca, A);  sB = cross(rb, A);  Km = (ims + dot(sA, I_a * sA)) + dot(sB, I_b * sB)
//   pAi = cross(ca, Ti);  pBi = cross(rb, Ti);  gi = dot(C, Ti) * s;  k_ij, d2 and m** as the hinge's, over (pA, pB)
//   e = ((cross(A, B) + cross(T1, U1)) + cross(T2, U2)) * 0.5;  gw = e * s;  Kw = I_a + I_b;  Kwinv = invert(Kw)
//   LOCK: side = 2, lb = (lo - d) * s;  LIMIT and d < lo: side = -1, lb = (lo - d) * s;  LIMIT and d > hi: side = +1, lb = -((d - hi) * s)
//   MOTOR:  mmax = fmax * h;  w = the target row's entry i
// SWEEPS in list order, the rows of one slider in the order motor, axis (limit or lock), angular, off-axis, each reading the current
// velocities - the `slider row` lines of the loop below.
// One launch, k_batch_slider_solve<GATED>, with k_batch_hinge_solve's shape and rules (k_batch_hinge.h): a workgroup per world that has
// sliders, a lane per slider (MGF_BATCH_MAX_WORLD_SLIDERS = kBatchBlock); the world's named bodies in LDS slots of 32 bytes - srec words
// 0 and 1 - and a progress word a slot; the plan is batch_joint_plan's; the lane solves its slider of sweep `it` once
// prog[sa] == it * deg[sa] + rank_a (and prog[sb] likewise), read with acquire loads at workgroup scope, ALL rows in one turn with both
// bodies' (v, omega) in registers between the rows, writes the velocities and release-stores both counters once.  Every lane of a wave
// that has a sweep left takes every trip, the wave sleeps only where none of its lanes is ready (__any), the spin is bounded
// (kBatchSpinLimit): a lane that gives up sets err[1] and the workgroup's flag, and the store-back is skipped.  GATED (a rollout) is the
// train's gate done[k] == tick && act[k] == tick, the same for a whole workgroup: an early return ahead of the first barrier, and a
// template argument so that nothing wave-uniform is evaluated inside the loop.  The lane keeps im and I of both ends, A, T1, T2, sA, sB,
// pA1, pA2, pB1, pB2, g1, g2, gw, m**, Km, Kwinv, lb, mmax, w and its seven accumulators in registers: a workgroup of 256 lanes is one
// wave per SIMD.  No float atomic, no scratch, vector stores only.
#pragma once
#include "k_batch_hinge.h"

namespace mgf {

constexpr uint32_t kSliderLimit = 1u, kSliderMotor = 2u, kSliderLock = 4u;  // MGF_SLIDER_LIMIT, MGF_SLIDER_MOTOR, MGF_SLIDER_LOCK

struct BatchSliderArgs {
  Bodies B;                     // every world's bodies
  const uint32_t* w_off;        // the worlds' first bodies
  const uint4* items;           // item w: (world, first sorted position, count | slots << 16, first slot)
  const float4* rig;            // by the caller's index, seven words a record
  const uint4* plan;            // sorted position -> (the caller's index, slot_a | slot_b << 16, rank_a | rank_b << 16, 0); slots local to the item
  const uint2* slots;           // slot -> (body, deg): the sliders that name the body
  const float* w;               // the target table's row for this call: a float a slider, by the caller's index
  float* acc;                   // the handle's: eight floats a slider - (p1, p2, al, am, aw.x, aw.y, aw.z, 0) - by the caller's index
  float* out;                   // the caller's, the same rows; null: not asked for
  unsigned long long* skipped;  // sliders that were skipped, cumulative (counter "sliders_skipped")
  uint32_t* err;                // the handle's error words: [1] a lane gave up waiting for its turn
  const uint32_t* done;         // a rollout: ticks of the call world k has completed (BatchArgs::done); null: a call of its own
  const uint32_t* act;          // a rollout: ticks whose actuation world k has behind it (BatchRolloutArgs::act)
  float h;                      // the time step
  uint32_t iters, tick;
};

__device__ __forceinline__ void slider_st8(float* p, float p1, float p2, float al, float am, V3 aw) {
  p[0] = p1; p[1] = p2; p[2] = al; p[3] = am; p[4] = aw.x; p[5] = aw.y; p[6] = aw.z; p[7] = 0.0f;
}
// rate(n, a, b) = (dot(v_b - v_a, n) + dot(omega_b, b)) - dot(omega_a, a)
__device__ __forceinline__ float slider_rate(V3 va, V3 oa, V3 vb, V3 ob, V3 n, V3 a, V3 b) { return (dot(vb - va, n) + dot(ob, b)) - dot(oa, a); }

template <bool GATED>
__global__ __launch_bounds__(kBatchBlock) void k_batch_slider_solve(BatchSliderArgs A) {
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
  // the lane's slider: setup from the state before the call
  const bool mine = tid < cnt;
  uint32_t i = 0, sa = 0, sb = 0, need_a = 0, need_b = 0, deg_a = 0, deg_b = 0;
  bool has_b = false, skip = false, motor = false;
  int32_t side = 0;
  V3 hA = mk3(0.0f, 0.0f, 0.0f), T1 = hA, T2 = hA, sA = hA, sB = hA, pA1 = hA, pA2 = hA, pB1 = hA, pB2 = hA, gw = hA, aw = hA;
  float im_a = 0.0f, im_b = 0.0f, g1 = 0.0f, g2 = 0.0f, m11 = 0.0f, m12 = 0.0f, m21 = 0.0f, m22 = 0.0f, Km = 0.0f, lb = 0.0f, mmax = 0.0f, wt = 0.0f;
  float p1 = 0.0f, p2 = 0.0f, al = 0.0f, am = 0.0f;
  M3 I_a = m3_cols(hA, hA, hA), I_b = I_a, Kwinv = I_a;
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
    motor = (flags & kSliderMotor) != 0u;
    const size_t ga = g0 + f2u(w0.y);
    const float4 qa = B.q[ga], s1 = B.srec[4 * ga + 1], s2 = B.srec[4 * ga + 2], s3 = B.srec[4 * ga + 3];
    const V3 xa = xyz(B.x[ga]) + xyz(B.delta[ga]);  // physics.rs:282, as k_batch_dev_gather
    const Quat Qa = mkq(qa.x, mk3(qa.y, qa.z, qa.w));
    const V3 ra = rotate(Qa, xyz(w1));
    const V3 Pa = xa + ra;
    im_a = s1.z;
    I_a = m3_cols(mk3(s1.w, s2.x, s2.y), mk3(s2.z, s2.w, s3.x), mk3(s3.y, s3.z, s3.w));
    hA = rotate(Qa, xyz(w3));
    T1 = rotate(Qa, xyz(w4));
    T2 = cross(hA, T1);
    V3 rb = mk3(0.0f, 0.0f, 0.0f), Pb = xyz(w2), Bx = xyz(w5), U1 = xyz(w6);
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
    const V3 U2 = cross(Bx, U1);
    const V3 C = Pb - Pa;
    const float s = w1.w / A.h;
    const V3 ca = ra + C;
    const float d = dot(C, hA);
    const float ims = im_a + im_b;
    sA = cross(ca, hA);
    sB = cross(rb, hA);
    Km = (ims + dot(sA, I_a * sA)) + dot(sB, I_b * sB);
    pA1 = cross(ca, T1);
    pB1 = cross(rb, T1);
    g1 = dot(C, T1) * s;
    pA2 = cross(ca, T2);
    pB2 = cross(rb, T2);
    g2 = dot(C, T2) * s;
    const V3 ja1 = I_a * pA1, ja2 = I_a * pA2, jb1 = I_b * pB1, jb2 = I_b * pB2;
    const float k11 = (ims + dot(pA1, ja1)) + dot(pB1, jb1), k22 = (ims + dot(pA2, ja2)) + dot(pB2, jb2);
    const float k12 = dot(pA1, ja2) + dot(pB1, jb2), k21 = dot(pA2, ja1) + dot(pB2, jb1);
    const float d2 = k11 * k22 - k12 * k21;
    m11 = k22 / d2;
    m12 = -k12 / d2;
    m21 = -k21 / d2;
    m22 = k11 / d2;
    const V3 e = ((cross(hA, Bx) + cross(T1, U1)) + cross(T2, U2)) * 0.5f;
    gw = e * s;
    const M3 Kw = I_a + I_b;
    const bool ok = invert(Kw, &Kwinv);
    if ((flags & kSliderLock) != 0u) { side = 2; lb = (w3.w - d) * s; }
    else if ((flags & kSliderLimit) != 0u && d < w3.w) { side = -1; lb = (w3.w - d) * s; }
    else if ((flags & kSliderLimit) != 0u && d > w4.w) { side = 1; lb = -((d - w4.w) * s); }
    if (motor) {
      mmax = w2.w * A.h;
      wt = A.w[i];
    }
    skip = !ok || d2 == 0.0f || (flags != 0u && Km == 0.0f) || !joint_finite3(ra) || !joint_finite3(rb) || !joint_finite3(sA) || !joint_finite3(sB) ||
           !joint_finite3(pA1) || !joint_finite3(pA2) || !joint_finite3(pB1) || !joint_finite3(pB2) || !hinge_finite(g1) || !hinge_finite(g2) || !joint_finite3(gw) ||
           !hinge_finite(m11) || !hinge_finite(m12) || !hinge_finite(m21) || !hinge_finite(m22) || !hinge_finite(Km) || !joint_finite3(Kwinv.c[0]) ||
           !joint_finite3(Kwinv.c[1]) || !joint_finite3(Kwinv.c[2]) || !hinge_finite(lb) || (motor && (mmax != mmax || !hinge_finite(wt)));
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
          if (motor) {  // slider row: the motor
            float lam = (wt - slider_rate(va, oa, vb, ob, hA, sA, sB)) / Km;
            float t = am + lam;
            if (t < -mmax) t = -mmax;
            if (t > mmax) t = mmax;
            lam = t - am;
            am = t;
            va = va - hA * (lam * im_a);
            oa = oa - I_a * (sA * lam);
            if (has_b) {
              vb = vb + hA * (lam * im_b);
              ob = ob + I_b * (sB * lam);
            }
          }
          if (side != 0) {  // slider row: the axis - a limit, or the lock
            float lam = (lb - slider_rate(va, oa, vb, ob, hA, sA, sB)) / Km;
            float t = al + lam;
            if (side == -1) { if (t < 0.0f) t = 0.0f; }
            if (side == 1) { if (t > 0.0f) t = 0.0f; }
            lam = t - al;
            al = t;
            va = va - hA * (lam * im_a);
            oa = oa - I_a * (sA * lam);
            if (has_b) {
              vb = vb + hA * (lam * im_b);
              ob = ob + I_b * (sB * lam);
            }
          }
          {  // slider row: the three angular rows
            const V3 L = -(Kwinv * ((ob - oa) + gw));
            oa = oa - I_a * L;
            if (has_b) ob = ob + I_b * L;
            aw = aw + L;
          }
          {  // slider row: the two off-axis rows
            const float r1 = slider_rate(va, oa, vb, ob, T1, pA1, pB1) + g1, r2 = slider_rate(va, oa, vb, ob, T2, pA2, pB2) + g2;
            const float l1 = -(m11 * r1 + m12 * r2), l2 = -(m21 * r1 + m22 * r2);
            const V3 n = T1 * l1 + T2 * l2;
            va = va - n * im_a;
            oa = oa - I_a * (pA1 * l1 + pA2 * l2);
            if (has_b) {
              vb = vb + n * im_b;
              ob = ob + I_b * (pB1 * l1 + pB2 * l2);
            }
            p1 = p1 + l1;
            p2 = p2 + l2;
          }
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
    slider_st8(A.acc + 8 * (size_t)i, p1, p2, al, am, aw);
    if (A.out) slider_st8(A.out + 8 * (size_t)i, p1, p2, al, am, aw);
  }
}

}  // namespace mgf
