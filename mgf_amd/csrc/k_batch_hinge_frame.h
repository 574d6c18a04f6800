// The frame lines of a hinge's SETUP (include/mgf_hip.h, "hinge joints between bodies"), written once for every kernel that forms a
// hinge's frames: the hinges' solver (k_batch_hinge.h), the sliders', whose frames are the same lines (k_batch_slider.h), and the
// encoders' skeleton, which forms them without solving (k_batch_joint_read.h).  (Part of the kernel set described in kernels.h.)
//
// Every helper is the header's line, the same helpers (rotate, cross, dot) in the same order, each a separately rounded f32 operation
// (-ffp-contract=off): the encoders read bit for bit what the solver's setup forms of the same state.  The ends are loaded by
// joint_ends (k_batch_joint_loop.h), the ball joints' too.
//   hinge_frame   ra, rb, C, A, T1, T2, B, U1 of the record's words; other == -1: rb = 0, Pb = pb, B = bx, U1 = ub
//   hinge_side    cphi, sphi and the limit's side: +1 or -1 by SETUP's rule with LIMIT and cphi <= ch, otherwise 0
#pragma once
#include "k_batch_joint.h"

namespace mgf {

constexpr uint32_t kHingeLimit = 1u, kHingeMotor = 2u;  // MGF_HINGE_LIMIT, MGF_HINGE_MOTOR

struct HingeFrame {
  V3 ra, rb, C, A, T1, T2, B, U1;
};

// a, b: the ends (joint_ends); w1 .. w6: the record's words (pa, beta), (pb, tmax), (ax, cm), (ua, sm), (bx, ch), (ub, sh); b is read
// where has_b alone
__device__ __forceinline__ HingeFrame hinge_frame(const JointEnd& a, const JointEnd& b, bool has_b, float4 w1, float4 w2, float4 w3, float4 w4, float4 w5,
                                                  float4 w6) {
  HingeFrame F;
  F.ra = rotate(a.q, xyz(w1));
  const V3 Pa = a.x + F.ra;
  F.A = rotate(a.q, xyz(w3));
  F.T1 = rotate(a.q, xyz(w4));
  F.T2 = cross(F.A, F.T1);
  F.rb = mk3(0.0f, 0.0f, 0.0f);
  V3 Pb = xyz(w2);
  F.B = xyz(w5);
  F.U1 = xyz(w6);
  if (has_b) {
    F.rb = rotate(b.q, xyz(w2));
    Pb = b.x + F.rb;
    F.B = rotate(b.q, xyz(w5));
    F.U1 = rotate(b.q, xyz(w6));
  }
  F.C = Pb - Pa;
  return F;
}

// c = dot(U1, T1), sn = dot(U1, T2); (cm, sm), (ch, sh) the record's
__device__ __forceinline__ float hinge_side(uint32_t flags, float c, float sn, float cm, float sm, float ch) {
  const float cphi = c * cm + sn * sm, sphi = sn * cm - c * sm;
  if ((flags & kHingeLimit) != 0u && cphi <= ch) return sphi >= 0.0f ? 1.0f : -1.0f;
  return 0.0f;
}

}  // namespace mgf
