// The frame lines of a hinge's SETUP (include/mgf_hip.h, "hinge joints between bodies"), written once for the kernels that form a hinge's
// frames without solving it (k_batch_hinge_read.h).  (Part of the kernel set described in kernels.h.)
//
// Every helper is the header's line, the same helpers (rotate, cross, dot) in the same order, each a separately rounded f32 operation
// (-ffp-contract=off): what they give is bit for bit what k_batch_hinge_solve's setup forms of the same state.  k_batch_hinge.h keeps
// its own copy of these lines, as it was written.
//   hinge_end     one end as the state stands: q, x + delta (physics.rs:282, as k_batch_dev_gather) and omega (srec words 0 and 1)
//   hinge_frame   ra, rb, Pa, Pb, C, A, T1, T2, B, U1 of the record's words; other == -1: B = bx, U1 = ub, Pb = pb
//   hinge_side    cphi, sphi and the limit's side: +1 or -1 by SETUP's rule with LIMIT and cphi <= ch, otherwise 0
#pragma once
#include "k_batch_hinge.h"

namespace mgf {

struct HingeEnd {
  Quat q;
  V3 x, om;
};
struct HingeFrame {
  V3 C, A, T1, T2, B, U1;
};

__device__ __forceinline__ HingeEnd hinge_end(const Bodies& B, size_t g) {
  const float4 q = B.q[g], s0 = B.srec[4 * g], s1 = B.srec[4 * g + 1];
  HingeEnd e;
  e.q = mkq(q.x, mk3(q.y, q.z, q.w));
  e.x = xyz(B.x[g]) + xyz(B.delta[g]);
  e.om = mk3(s0.w, s1.x, s1.y);
  return e;
}

// w1 .. w6: the record's words (pa, beta), (pb, tmax), (ax, cm), (ua, sm), (bx, ch), (ub, sh); b is read where has_b alone
__device__ __forceinline__ HingeFrame hinge_frame(const HingeEnd& a, const HingeEnd& b, bool has_b, float4 w1, float4 w2, float4 w3, float4 w4, float4 w5,
                                                  float4 w6) {
  HingeFrame F;
  const V3 ra = rotate(a.q, xyz(w1));
  const V3 Pa = a.x + ra;
  F.A = rotate(a.q, xyz(w3));
  F.T1 = rotate(a.q, xyz(w4));
  F.T2 = cross(F.A, F.T1);
  V3 Pb = xyz(w2);
  F.B = xyz(w5);
  F.U1 = xyz(w6);
  if (has_b) {
    const V3 rb = rotate(b.q, xyz(w2));
    Pb = b.x + rb;
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
