// Hinge joints between the bodies of a batch (mgf_batch_set_hinges, mgf_batch_set_hinge_targets, mgf_batch_solve_hinges,
// mgf_batch_solve_hinges_dev, and ahead of every tick of a rollout; host_batch_hinge.inc).
// (Part of the kernel set described in kernels.h.)
//
// A hinge is a ball joint (k_batch_joint.h) plus two angular rows that keep the two hinge axes parallel, an optional limit of the hinge
// angle and an optional velocity motor with a torque cap: (world, body, other, flags, pa, beta, pb, tmax, ax, cm, ua, sm, bx, ch, ub,
// sh), seven 16-byte words.  The definition stands in include/mgf_hip.h, every line a separate f32 operation; here in short.  SETUP per
// hinge, from the state before the call: ra, rb, Pa, Pb, C, s, bias, K and Kinv are the ball joint's lines (JointRows::point);
//   A = rotate(q_a, ax);  T1 = rotate(q_a, ua);  T2 = cross(A, T1);  B = rotate(q_b, bx);  U1 = rotate(q_b, ub)   (other == -1: B = bx, U1 = ub)
//   n1 = cross(B, T1);  n2 = cross(B, T2);  g1 = dot(B, T1) * s;  g2 = dot(B, T2) * s;  J(n) = I_a * n + I_b * n
//   k_ij = dot(n_i, J(n_j));  d2 = k11 * k22 - k12 * k21;  m11 = k22 / d2;  m12 = -k12 / d2;  m21 = -k21 / d2;  m22 = k11 / d2;  Km = dot(A, J(A))
//   c = dot(U1, T1);  sn = dot(U1, T2);  cphi = c * cm + sn * sm;  sphi = sn * cm - c * sm
//   LIMIT and cphi <= ch:  err = fabs(sphi) * ch - cphi * sh;  sphi >= 0: side = +1, lb = -(err * s);  else side = -1, lb = err * s
//   MOTOR:  mmax = tmax * h;  w = the target row's entry i
// SWEEPS in list order, the rows of one hinge in the order motor, limit, angular, point, wd = omega_b - omega_a formed again ahead of
// each of the first three - the `hinge row` lines of HingeRows::sweep.
// One launch, k_batch_hinge_solve<GATED>: batch_joint_loop (k_batch_joint_loop.h) over HingeRows, a lane per hinge
// (MGF_BATCH_MAX_WORLD_HINGES = kBatchBlock), ALL FOUR rows in one turn.  The lane keeps the point's registers (ra, rb, bias, Kinv, im and
// I of both ends), A, n1, n2, g1, g2, m**, Km, lb, mmax, w and its seven accumulators in registers: a workgroup of 256 lanes is one wave
// per SIMD.
#pragma once
#include "k_batch_hinge_frame.h"

namespace mgf {

// J(n) = I_a * n + I_b * n
__device__ __forceinline__ V3 hinge_j(const M3& I_a, const M3& I_b, V3 n) { return I_a * n + I_b * n; }

struct HingeRows {
  static constexpr uint32_t kWords = 7, kFloats = 8;
  JointRows P;  // the point: the ball joint's registers, acc among them
  bool motor;
  int32_t side;
  V3 hA, n1, n2;
  float g1, g2, Km, lb, mmax, wt;
  JointInv2 M;
  float a1, a2, al, am;

  __device__ __forceinline__ bool setup(const BatchJointArgs& A, const float4* rec, uint32_t i, size_t g0, bool has_b) {
    const float4 w0 = rec[0], w1 = rec[1], w2 = rec[2], w3 = rec[3], w4 = rec[4], w5 = rec[5], w6 = rec[6];
    const uint32_t flags = f2u(w0.w);
    motor = (flags & kHingeMotor) != 0u;
    JointEnd a, b;
    joint_ends(A.B, g0, w0, has_b, &a, &b);
    const HingeFrame F = hinge_frame(a, b, has_b, w1, w2, w3, w4, w5, w6);
    const float s = w1.w / A.h;
    const bool ok = P.point(a, b, F.ra, F.rb, F.C, s);
    hA = F.A;
    n1 = cross(F.B, F.T1);
    n2 = cross(F.B, F.T2);
    g1 = dot(F.B, F.T1) * s;
    g2 = dot(F.B, F.T2) * s;
    const V3 j1 = hinge_j(P.I_a, P.I_b, n1), j2 = hinge_j(P.I_a, P.I_b, n2);
    M = joint_inv2(dot(n1, j1), dot(n1, j2), dot(n2, j1), dot(n2, j2));
    Km = dot(hA, hinge_j(P.I_a, P.I_b, hA));
    const float c = dot(F.U1, F.T1), sn = dot(F.U1, F.T2);
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
    return !ok || !P.point_finite() || M.d2 == 0.0f || ((flags & (kHingeLimit | kHingeMotor)) != 0u && Km == 0.0f) || !joint_finite3(n1) || !joint_finite3(n2) ||
           !joint_finite(g1) || !joint_finite(g2) || !joint_finite(M.m11) || !joint_finite(M.m12) || !joint_finite(M.m21) || !joint_finite(M.m22) || !joint_finite(Km) ||
           !joint_finite(lb) || (motor && (mmax != mmax || !joint_finite(wt)));
  }

  __device__ __forceinline__ void sweep(V3& va, V3& oa, V3& vb, V3& ob, bool has_b) {
    if (motor) {  // hinge row: the motor
      const V3 wd = ob - oa;
      const V3 imp = hA * joint_motor_lam(wt, dot(wd, hA), Km, mmax, am);
      oa = oa - P.I_a * imp;
      if (has_b) ob = ob + P.I_b * imp;
    }
    if (side != 0) {  // hinge row: the limit
      const V3 wd = ob - oa;
      const V3 imp = hA * joint_limit_lam(lb, dot(wd, hA), Km, side, al);
      oa = oa - P.I_a * imp;
      if (has_b) ob = ob + P.I_b * imp;
    }
    {  // hinge row: the two angular rows
      const V3 wd = ob - oa;
      const float r1 = dot(wd, n1) + g1, r2 = dot(wd, n2) + g2;
      const float l1 = -(M.m11 * r1 + M.m12 * r2), l2 = -(M.m21 * r1 + M.m22 * r2);
      const V3 imp = n1 * l1 + n2 * l2;
      oa = oa - P.I_a * imp;
      if (has_b) ob = ob + P.I_b * imp;
      a1 = a1 + l1;
      a2 = a2 + l2;
    }
    P.sweep(va, oa, vb, ob, has_b);  // hinge row: the point, the ball joint's lines
  }

  __device__ __forceinline__ void store(float* p) const {
    p[0] = P.acc.x; p[1] = P.acc.y; p[2] = P.acc.z; p[3] = a1; p[4] = a2; p[5] = al; p[6] = am; p[7] = 0.0f;
  }
};

template <bool GATED>
__global__ __launch_bounds__(kBatchBlock) void k_batch_hinge_solve(BatchJointArgs A) {
  batch_joint_loop<HingeRows, GATED>(A);
}

}  // namespace mgf
