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
// One launch, k_batch_joint_solve<GATED>: batch_joint_loop (k_batch_joint_loop.h) over JointRows, a lane per joint
// (MGF_BATCH_MAX_WORLD_JOINTS = kBatchBlock).  The lane keeps ra, rb, bias, Kinv, im and I of both ends and its accumulator in registers.
#pragma once
#include "k_batch_joint_loop.h"

namespace mgf {

// column k of K for one end: e_k * im + cross(I * cross(r, e_k), r)
__device__ __forceinline__ V3 joint_k_col(V3 e, float im, const M3& I, V3 r) { return e * im + cross(I * cross(r, e), r); }

struct JointRows {
  static constexpr uint32_t kWords = 3, kFloats = 3;
  V3 ra, rb, bias, acc;
  float im_a, im_b;
  M3 I_a, I_b, Kinv;

  // the point's lines of SETUP behind the ends, the arms and the gap C, the hinge's too; false: K is singular
  __device__ __forceinline__ bool point(const JointEnd& a, const JointEnd& b, V3 ra_, V3 rb_, V3 C, float s) {
    ra = ra_;
    rb = rb_;
    im_a = a.im;
    I_a = a.I;
    im_b = b.im;
    I_b = b.I;
    bias = C * s;
    const V3 e0 = mk3(1.0f, 0.0f, 0.0f), e1 = mk3(0.0f, 1.0f, 0.0f), e2 = mk3(0.0f, 0.0f, 1.0f);
    const M3 K = m3_cols(joint_k_col(e0, im_a, I_a, ra) + joint_k_col(e0, im_b, I_b, rb), joint_k_col(e1, im_a, I_a, ra) + joint_k_col(e1, im_b, I_b, rb),
                         joint_k_col(e2, im_a, I_a, ra) + joint_k_col(e2, im_b, I_b, rb));
    return invert(K, &Kinv);
  }
  __device__ __forceinline__ bool point_finite() const { return joint_finite3(ra) && joint_finite3(rb) && joint_finite3(bias) && joint_finite9(Kinv); }

  __device__ __forceinline__ bool setup(const BatchJointArgs& A, const float4* rec, uint32_t, size_t g0, bool has_b) {
    const float4 w0 = rec[0], w1 = rec[1], w2 = rec[2];
    JointEnd a, b;
    joint_ends(A.B, g0, w0, has_b, &a, &b);
    const V3 r_a = rotate(a.q, xyz(w1));
    const V3 Pa = a.x + r_a;
    V3 r_b = mk3(0.0f, 0.0f, 0.0f), Pb = xyz(w2);
    if (has_b) {
      r_b = rotate(b.q, xyz(w2));
      Pb = b.x + r_b;
    }
    const bool ok = point(a, b, r_a, r_b, Pb - Pa, w1.w / A.h);
    return !ok || !point_finite();
  }

  __device__ __forceinline__ void sweep(V3& va, V3& oa, V3& vb, V3& ob, bool has_b) {
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

  __device__ __forceinline__ void store(float* p) const { st3(p, acc.x, acc.y, acc.z); }
};

template <bool GATED>
__global__ __launch_bounds__(kBatchBlock) void k_batch_joint_solve(BatchJointArgs A) {
  batch_joint_loop<JointRows, GATED>(A);
}

}  // namespace mgf
