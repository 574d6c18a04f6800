// Hinge encoders of a batch (mgf_batch_read_hinges, mgf_batch_read_hinges_dev, and the readings table behind every tick of a rollout -
// mgf_batch_set_hinge_trace; host_batch_joint_read.inc under HingeKind).  (Part of the kernel set described in kernels.h.)
//
// A reading is eight floats, (c, sn, rate, side, gap.x, gap.y, gap.z, tilt2), formed from the state as it stands by the hinge's SETUP
// lines (include/mgf_hip.h; the frame lines are k_batch_hinge_frame.h's, written once):
//   c = dot(U1, T1);  sn = dot(U1, T2)      the angle is atan2(sn, c); no arctangent is evaluated here
//   rate = dot(omega_b - omega_a, A)        other == -1: omega_b = 0
//   side                                    +1 or -1 by SETUP's rule with LIMIT and cphi <= ch, otherwise 0: the next solve's limit row
//   gap = C                                 the anchors' gap in the world
//   e1 = dot(B, T1);  e2 = dot(B, T2);  tilt2 = e1 * e1 + e2 * e2     the squared sine of the angle between the two axes
// No division: no hinge is skipped and nothing is counted.  Non-finite state gives non-finite words.
// One launch, k_batch_read_hinges<GATED, FORMAT>: a single call of the encoders' skeleton (batch_joint_read, k_batch_joint_read.h, which
// holds the lane's walk, the gate, the loads and the stores in three formats) over HingeReading, which holds the lines above.  A full
// entry's eight impulse words are (acc.x, acc.y, acc.z, a1, a2, al, am, 0), as tick t's k_batch_hinge_solve wrote them.
// (The kernel is not called k_batch_hinge_read: tools/kernel_resources.py selects by substring, and the hinge solver's rows are asked
// for as "k_batch_hinge".)
#pragma once
#include "k_batch_joint_read.h"

namespace mgf {

struct HingeReading {
  struct Own {};  // the ends carry everything a hinge's reading needs
  __device__ __forceinline__ static Own load(const Bodies&, size_t, float4, bool) { return {}; }
  __device__ __forceinline__ static JointReadWords form(Own, float4 w0, float4 w3, float4 w4, float4 w5, const JointEnd& a, const JointEnd& b, const HingeFrame& F) {
    const float c = dot(F.U1, F.T1), sn = dot(F.U1, F.T2);
    const float rate = dot(b.om - a.om, F.A);
    const float side = hinge_side(f2u(w0.w), c, sn, w3.w, w4.w, w5.w);
    const float e1 = dot(F.B, F.T1), e2 = dot(F.B, F.T2);
    const float tilt2 = e1 * e1 + e2 * e2;
    return {make_float4(c, sn, rate, side), make_float4(F.C.x, F.C.y, F.C.z, tilt2)};
  }
};

template <bool GATED, int FORMAT>
__global__ __launch_bounds__(kBatchBlock) void k_batch_read_hinges(BatchJointReadArgs A) {
  batch_joint_read<HingeReading, GATED, FORMAT>(A);
}

}  // namespace mgf
