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
// velocities - the `slider row` lines of SliderRows::sweep.
// One launch, k_batch_slider_solve<GATED>: batch_joint_loop (k_batch_joint_loop.h) over SliderRows, a lane per slider
// (MGF_BATCH_MAX_WORLD_SLIDERS = kBatchBlock), ALL rows in one turn.  The lane keeps im and I of both ends, A, T1, T2, sA, sB, pA1, pA2,
// pB1, pB2, g1, g2, gw, m**, Km, Kwinv, lb, mmax, w and its seven accumulators in registers: a workgroup of 256 lanes is one wave per SIMD.
#pragma once
#include "k_batch_hinge.h"

namespace mgf {

constexpr uint32_t kSliderLimit = 1u, kSliderMotor = 2u, kSliderLock = 4u;  // MGF_SLIDER_LIMIT, MGF_SLIDER_MOTOR, MGF_SLIDER_LOCK

// rate(n, a, b) = (dot(v_b - v_a, n) + dot(omega_b, b)) - dot(omega_a, a)
__device__ __forceinline__ float slider_rate(V3 va, V3 oa, V3 vb, V3 ob, V3 n, V3 a, V3 b) { return (dot(vb - va, n) + dot(ob, b)) - dot(oa, a); }

struct SliderRows {
  static constexpr uint32_t kWords = 7, kFloats = 8;
  bool motor;
  int32_t side;
  V3 hA, T1, T2, sA, sB, pA1, pA2, pB1, pB2, gw, aw;
  float im_a, im_b, g1, g2, Km, lb, mmax, wt;
  JointInv2 M;
  float p1, p2, al, am;
  M3 I_a, I_b, Kwinv;

  __device__ __forceinline__ bool setup(const BatchJointArgs& A, const float4* rec, uint32_t i, size_t g0, bool has_b) {
    const float4 w0 = rec[0], w1 = rec[1], w2 = rec[2], w3 = rec[3], w4 = rec[4], w5 = rec[5], w6 = rec[6];
    const uint32_t flags = f2u(w0.w);
    motor = (flags & kSliderMotor) != 0u;
    JointEnd a, b;
    joint_ends(A.B, g0, w0, has_b, &a, &b);
    const HingeFrame F = hinge_frame(a, b, has_b, w1, w2, w3, w4, w5, w6);
    const V3 ra = F.ra, rb = F.rb, C = F.C;
    im_a = a.im;
    I_a = a.I;
    im_b = b.im;
    I_b = b.I;
    hA = F.A;
    T1 = F.T1;
    T2 = F.T2;
    const V3 U2 = cross(F.B, F.U1);
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
    M = joint_inv2(k11, k12, k21, k22);
    const V3 e = ((cross(hA, F.B) + cross(T1, F.U1)) + cross(T2, U2)) * 0.5f;
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
    return !ok || M.d2 == 0.0f || (flags != 0u && Km == 0.0f) || !joint_finite3(ra) || !joint_finite3(rb) || !joint_finite3(sA) || !joint_finite3(sB) ||
           !joint_finite3(pA1) || !joint_finite3(pA2) || !joint_finite3(pB1) || !joint_finite3(pB2) || !joint_finite(g1) || !joint_finite(g2) || !joint_finite3(gw) ||
           !joint_finite(M.m11) || !joint_finite(M.m12) || !joint_finite(M.m21) || !joint_finite(M.m22) || !joint_finite(Km) || !joint_finite9(Kwinv) ||
           !joint_finite(lb) || (motor && (mmax != mmax || !joint_finite(wt)));
  }

  // an impulse lam along the axis
  __device__ __forceinline__ void axis(V3& va, V3& oa, V3& vb, V3& ob, bool has_b, float lam) const {
    va = va - hA * (lam * im_a);
    oa = oa - I_a * (sA * lam);
    if (has_b) {
      vb = vb + hA * (lam * im_b);
      ob = ob + I_b * (sB * lam);
    }
  }

  __device__ __forceinline__ void sweep(V3& va, V3& oa, V3& vb, V3& ob, bool has_b) {
    if (motor)  // slider row: the motor
      axis(va, oa, vb, ob, has_b, joint_motor_lam(wt, slider_rate(va, oa, vb, ob, hA, sA, sB), Km, mmax, am));
    if (side != 0)  // slider row: the axis - a limit, or the lock
      axis(va, oa, vb, ob, has_b, joint_limit_lam(lb, slider_rate(va, oa, vb, ob, hA, sA, sB), Km, side, al));
    {  // slider row: the three angular rows
      const V3 L = -(Kwinv * ((ob - oa) + gw));
      oa = oa - I_a * L;
      if (has_b) ob = ob + I_b * L;
      aw = aw + L;
    }
    {  // slider row: the two off-axis rows
      const float r1 = slider_rate(va, oa, vb, ob, T1, pA1, pB1) + g1, r2 = slider_rate(va, oa, vb, ob, T2, pA2, pB2) + g2;
      const float l1 = -(M.m11 * r1 + M.m12 * r2), l2 = -(M.m21 * r1 + M.m22 * r2);
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
  }

  __device__ __forceinline__ void store(float* p) const {
    p[0] = p1; p[1] = p2; p[2] = al; p[3] = am; p[4] = aw.x; p[5] = aw.y; p[6] = aw.z; p[7] = 0.0f;
  }
};

template <bool GATED>
__global__ __launch_bounds__(kBatchBlock) void k_batch_slider_solve(BatchJointArgs A) {
  batch_joint_loop<SliderRows, GATED>(A);
}

}  // namespace mgf
